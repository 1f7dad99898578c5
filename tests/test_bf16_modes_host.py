"""Host side of the reduced-precision GEMM modes ('bf16x2' / 'bf16'): the weight packing against an independent split,
and the option plumbing from Model.gemm_precision to the plan.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_modes_ref import split_parts            # noqa: E402

PACK_SHAPES = [(1, 1, 576, 576), (3, 3, 96, 320), (1, 1, 48, 200), (3, 3, 32, 50), (1, 1, 70, 33)]


@pytest.mark.parametrize('parts', [1, 2, 3])
@pytest.mark.parametrize('shape', PACK_SHAPES)
def test_pack_conv_split_parts_against_torch_bfloat16(parts, shape, hip_lib):
    """unpack_conv_split(parts=P) returns the parts an independent split with torch.Tensor.bfloat16() makes, bit for bit;
    the padding is zero; the parts of a smaller mode are the leading parts of a larger one."""
    from deephar_amd.engine import packing
    kh, kw, cin, cout = shape
    rng = np.random.default_rng(kh * 1000 + cin + cout + parts)
    w = (rng.standard_normal(shape) * np.exp(rng.uniform(-6, 2, shape))).astype(np.float32)     # many binades
    w.flat[:4] = [0.0, -0.0, 1.0, 2.0 ** -100]
    pk, kp, np_ = packing.pack_conv_split(w, parts=parts)
    k = kh * kw * cin
    assert (kp, np_) == ((k + 31) // 32 * 32, (cout + 31) // 32 * 32) and pk.dtype == np.float32
    assert pk.view(np.uint16).size == parts * kp * np_
    tot, got = packing.unpack_conv_split(pk, kh, kw, cin, cout, parts=parts)
    assert got.shape == (kp // 8, parts, np_, 8)
    ref = split_parts(torch.from_numpy(w), parts)
    mask = np.zeros((kp, np_), bool)
    mask[:k, :cout] = True
    for q in range(parts):
        g = got[:, q].transpose(0, 2, 1).reshape(kp, np_)
        r = ref[q].numpy().reshape(k, cout)
        assert np.array_equal(g[:k, :cout].view(np.uint32), r.view(np.uint32)), 'part %d' % (q + 1)
        assert not g[~mask].any()
    assert np.array_equal(tot, sum(r.double() for r in ref).numpy())
    if parts == 3:
        assert np.array_equal(tot, w.astype(np.float64))          # three parts carry a float32 exactly
    else:
        lead = packing.unpack_conv_split(packing.pack_conv_split(w, parts=3)[0], kh, kw, cin, cout, parts=3)[1]
        assert np.array_equal(got.view(np.uint32), lead[:, :parts].view(np.uint32))


@pytest.mark.parametrize('shape', PACK_SHAPES)
def test_three_parts_is_the_existing_split_packing(shape, hip_lib):
    """parts = 3 equals pack_conv_split as it was (dh_conv2d_pack_weights_split_host) byte for byte, through the Python
    packer and through the new C entry point."""
    from deephar_amd.engine import packing
    kh, kw, cin, cout = shape
    w = np.random.default_rng(cin).standard_normal(shape).astype(np.float32)
    old, kp, np_ = packing.pack_conv_split(w)
    new, kp3, np3 = packing.pack_conv_split(w, parts=3)
    assert (kp, np_) == (kp3, np3) and old.tobytes() == new.tobytes()
    a = np.full(3 * kp * np_, 0xffff, np.uint16)
    b = np.full(3 * kp * np_, 0xeeee, np.uint16)
    assert hip_lib.dh_conv2d_pack_weights_split_host(w.ctypes.data, a.ctypes.data, kh, kw, cin, cout) == 0
    assert hip_lib.dh_conv2d_pack_weights_parts_host(w.ctypes.data, b.ctypes.data, kh, kw, cin, cout, 3) == 0
    assert a.tobytes() == b.tobytes() == old.tobytes()
    for bad in (0, 4, -1):
        assert hip_lib.dh_conv2d_pack_weights_parts_host(w.ctypes.data, b.ctypes.data, kh, kw, cin, cout, bad) != 0
    with pytest.raises(ValueError):
        packing.pack_conv_split(w, parts=4)


def _mpii(blocks=1):
    from deephar_amd import graph
    from deephar_amd.models import reception
    graph.reset_naming()
    return reception.build((256, 256, 3), 16, dim=2, num_blocks=blocks, ksize=(5, 5), num_context_per_joint=2)


def test_model_accepts_the_new_modes_and_replans():
    """Both new values are accepted, a typo still raises at assignment, changing the mode drops plan and executor, and the
    plan records the mode (the mirror of test_host_logic.test_engine_options_replan_the_model)."""
    m = _mpii(1)
    p1 = m.plan
    assert p1.gemm_precision == 'f32'
    for mode in ('bf16x2', 'bf16', 'bf16x3', 'bf16x2'):
        prev = m.plan
        m.gemm_precision = mode
        assert m._plan is None and m._exec is None
        assert m.plan is not prev and m.plan.gemm_precision == mode
        kept = m.plan
        m.gemm_precision = mode
        assert m.plan is kept                            # unchanged value: nothing is thrown away
    for typo in ('bf16x4', 'bf16x1', 'BF16', 'fp16', 2):
        with pytest.raises(ValueError):
            m.gemm_precision = typo
    assert m.gemm_precision == 'bf16x2'                  # a refused value changes nothing


def test_build_plan_records_the_mode():
    from deephar_amd.engine.planner import build_plan
    m = _mpii(1)
    for mode in ('f32', 'bf16x3', 'bf16x2', 'bf16'):
        assert build_plan(m.inputs, m.outputs, gemm_precision=mode).gemm_precision == mode
    with pytest.raises(ValueError):
        build_plan(m.inputs, m.outputs, gemm_precision='bf16x5')


def test_environment_default_passes_through(monkeypatch):
    monkeypatch.setenv('DEEPHAR_GEMM', 'bf16')
    assert _mpii(1).gemm_precision == 'bf16'
    monkeypatch.setenv('DEEPHAR_GEMM', 'bf16x2')
    assert _mpii(1).plan.gemm_precision == 'bf16x2'
    monkeypatch.setenv('DEEPHAR_GEMM', 'bf17')
    with pytest.raises(ValueError):
        _mpii(1)


def test_executor_maps_modes_to_weight_layout_codes():
    """One table from the plan's precision to dh_conv_args.w_split, one from w_split to the parts the packer makes."""
    from deephar_amd.engine import executor, packing
    assert executor.SPLIT_CODES == {'bf16x3': 1, 'bf16x2': 3, 'bf16': 4}
    assert packing.SPLIT_PARTS == {1: 3, 3: 2, 4: 1}


def test_split_eligibility_is_one_rule_for_every_mode(hip_lib):
    """dh_conv2d_split_eligible does not look at w_split: the same answer whichever split code the struct carries."""
    from deephar_amd import _lib
    a = _lib.ConvArgs()
    a.x = 4096
    a.N, a.H, a.W, a.OH, a.OW = 2, 32, 32, 32, 32
    a.KH = a.KW = a.SH = a.SW = 1
    for cin, cout, want in ((576, 576, 1), (48, 576, 1), (3, 32, 0)):
        a.Cin = a.ldx = cin
        a.Cout = a.ldy = cout
        a.K, a.Kp, a.Np = cin, (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
        for code in (0, 1, 3, 4):
            a.w_split = code
            assert hip_lib.dh_conv2d_split_eligible(C.byref(a)) == want, (cin, cout, code)
    a.w_split = 3
    a.H = a.W = a.OH = a.OW = 8
    a.Cin = a.ldx = a.K = a.Kp = 288
    a.Cout = a.ldy = a.Np = 128                                      # a skinny layer: never on the split family
    assert hip_lib.dh_conv2d_split_eligible(C.byref(a)) == 0
    assert hip_lib.dh_conv2d_uses_split_k(C.byref(a)) == 0           # split-packed weights never take that kernel either
