"""Conv2DTranspose((2, 2), strides=(2, 2)) on the split-bf16 precision ladder: dh_conv2d_transpose2x2_split_f32 (csrc/convt2x2s.hip)
and Model.gemm_precision = 'bf16x3' / 'bf16x2' / 'bf16' on downsampling_type='conv' models.

The contract is the one of tests/bf16_modes_ref.py, extended by the layer's BatchNormalization prologue: the activation operand is
a = relu?(fmaf(x, pre_scale, pre_shift)) in fp32 (the operand of the fp32 kernel), split AFTER the prologue and the ReLU into P
bf16 parts; the weight is the [Cin, 4 Cout] matrix split on the host; E_P = the products with i + j <= P + 1, exact, accumulated
in fp32; the depth-to-space epilogue (residual at the output resolution, ReLU) is the fp32 kernel's.  The tests:
  1. operands built so that every kept product and partial sum is exact in fp32: the kernel equals E_P bit for bit;
  2. random operands, every fused variant: within twice the shipped fp32 kernel's own error of E_P + epilogue in fp64;
  3. bit-equal across tilings, batch sizes, channel slabs and the scalar store path;
  4. whole models against the fp64 restatement, bar from a CPU emulation of the mode: max(1e-3 px, 2 x emu_px);
  5. an exported plan (blob version 4) run by the C executor reproduces predict bit for bit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_modes_ref as R                          # noqa: E402
import resample_ref as RS                           # noqa: E402
from oracle import ops as O                         # noqa: E402
from test_gpu_resampling_models import _mini_pyramid, _pose_spnet        # noqa: E402
from test_gpu_resampling_ops import CONVT_CASES, _convt_inputs           # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ('bf16x3', 'bf16x2', 'bf16')
CODES = {'bf16x3': 1, 'bf16x2': 3, 'bf16': 4}
UNSUPPORTED = 'rc=-2'


def _convt(a, k, strides=None, padding=None):
    """Conv2DTranspose as the `conv` of bf16_modes_ref.conv_ep: (operand, Keras kernel [2, 2, Cout, Cin]) -> output."""
    return RS.conv_transpose2x2(a, k)


def _operand(x, ps=None, pb=None, relu=False):
    """The fp32 activation operand of the kernels, relu?(fmaf(x, ps, pb)), as a float32 tensor: the product is exact in
    fp64 and the sum rounds once to 53 bits, then to 24 (a double rounding can differ from the fused one on a tie of the
    second rounding only: ~2^-29 per element, an ulp of one operand, far inside the bars below)."""
    a = torch.from_numpy(x).double()
    if ps is not None:
        a = (a * torch.from_numpy(ps).double() + torch.from_numpy(pb).double()).float().double()
    if relu:
        a = O.relu(a)
    return a.float()


def _eligible(hip_lib, case, prologue, ldx=None, ldy=None):
    from deephar_amd import _lib
    n, h, w, cin, cout = case
    a = _lib.ConvtArgs()
    a.x, a.w, a.y = 0x10000, 0x20000, 0x30000
    if prologue:
        a.pre_scale, a.pre_shift = 0x40000, 0x50000
    a.N, a.H, a.W, a.Cin, a.ldx = n, h, w, cin, ldx or cin
    a.Cout, a.ldy = cout, ldy or cout
    a.Kp, a.Np = (cin + 31) // 32 * 32, (4 * cout + 31) // 32 * 32
    return bool(hip_lib.dh_conv2d_transpose2x2_split_eligible(C.byref(a)))


def _tilings(hip_lib, run):
    """run(cfg) on the library's pick and on every tiling of the kernel -> {cfg: result}; no tiling may refuse."""
    outs = {cfg: run(cfg) for cfg in range(-1, hip_lib.dh_conv2d_transpose2x2_num_split_tile_cfgs())}
    torch.cuda.synchronize()
    return outs


def test_the_first_four_cases_are_eligible(hip_lib):
    for case in CONVT_CASES[:4]:
        assert _eligible(hip_lib, case, True) and _eligible(hip_lib, case, False), case


# ---- 1. known answers, no tolerance ------------------------------------------------------------------------------------
def _exact_operand(rng, shape):
    """hi + lo with hi in {+-1, +-1.5}, lo in +-{4 .. 7} * 2^-12: the RNE split is exactly (hi, lo, 0) (test_gpu_bf16_modes.py)."""
    hi = rng.choice(np.array([1.0, -1.0, 1.5, -1.5], np.float32), shape)
    lo = (rng.integers(4, 8, shape) * rng.choice(np.array([1, -1]), shape)).astype(np.float32) * np.float32(2.0 ** -12)
    return hi, lo


# K <= 288: with a scale of 2 on the activation every kept term of P <= 2 is a multiple of 2^-13 and
# sum |terms| <= 288 * (3 * 1.5 + 2 * 3 * 7 * 2^-12 ...) < 2^24 * 2^-13 = 2048: any fp32 accumulation order is exact.
EXACT_CASES = [(2, 8, 8, 288, 96), (2, 3, 5, 48, 20), (1, 1, 1, 32, 16), (3, 4, 4, 36, 24)]


@pytest.mark.parametrize('mode', ['bf16x2', 'bf16'])
@pytest.mark.parametrize('case', EXACT_CASES)
def test_known_answers_bit_for_bit(case, mode, hip_lib, cuda):
    from deephar_amd import functional as F
    n, h, w, cin, cout = case
    assert cin <= 288 and _eligible(hip_lib, case, True)
    rng = np.random.default_rng(sum(case))
    xh, xl = _exact_operand(rng, (n, h, w, cin))
    wh, wl = _exact_operand(rng, (2, 2, cout, cin))
    ps = rng.choice(np.array([1.0, 2.0], np.float32), cin)
    pb = np.zeros(cin, np.float32)
    x, k = xh + xl, wh + wl
    t = lambda a: torch.from_numpy(a).double()
    # the construction does what it says: the post-prologue operand relu(ps * x) splits to (relu-masked ps * hi, ps * lo, 0)
    a = _operand(x, ps, pb, True)
    pos = (x > 0).astype(np.float32)
    ah, al = xh * ps * pos, xl * ps * pos
    p = R.split_parts(a, 3)
    assert torch.equal(p[0], torch.from_numpy(ah)) and torch.equal(p[1], torch.from_numpy(al)) and not p[2].any()
    p = R.split_parts(torch.from_numpy(k), 3)
    assert torch.equal(p[0], torch.from_numpy(wh)) and torch.equal(p[1], torch.from_numpy(wl)) and not p[2].any()
    e = {'bf16': _convt(t(ah), t(wh)), 'exact': _convt(a.double(), t(k))}
    e['bf16x2'] = e['bf16'] + _convt(t(al), t(wh)) + _convt(t(ah), t(wl))
    for name in ('bf16', 'bf16x2'):
        assert torch.equal(e[name], R.conv_ep(_convt, a.double(), t(k), None, None, R.PARTS[name])), name
        assert torch.equal(e[name].float().double(), e[name])      # representable: the fp32 result can be the fp64 one
    d = lambda v: torch.from_numpy(v).to(cuda)
    outs = _tilings(hip_lib, lambda cfg: F.conv2d_transpose(d(x), k, pre_scale=d(ps), pre_shift=d(pb), pre_relu=True,
                                                            precision=mode, tile_cfg=cfg))
    assert len(outs) >= 3
    for cfg, y in outs.items():
        y = y.cpu().double()
        bad = int((y != e[mode]).sum())
        assert bad == 0, '%s tiling %d: %d of %d outputs differ from E_P, worst %.3e' % (
            mode, cfg, bad, y.numel(), float((y - e[mode]).abs().max()))
    y = outs[-1].cpu().double()
    for other in e:
        if other != mode:
            frac = float((y != e[other]).double().mean())
            assert frac > 0.9, 'E(%s) equals E(%s) on %.1f %% of the outputs: the case cannot tell them apart' % (
                mode, other, 100 - 100 * frac)


# ---- 2. random operands, every fused variant ---------------------------------------------------------------------------
VARIANTS = [('plain', ()), ('bn relu', ('bn',)), ('res', ('res',)), ('res relu', ('res', 'post')), ('bn relu res', ('bn', 'res'))]


@pytest.mark.parametrize('case', CONVT_CASES)
def test_random_operands_every_fused_variant(case, hip_lib, cuda):
    """Against E_P of the post-prologue operand + epilogue in fp64.  Bar: twice the distance of the shipped fp32 transposed
    convolution from fp64 on the same inputs, + 1e-6 (the convention of test_gpu_bf16_modes.py: with the mode's rounding
    inside the reference what remains is the same fp32 accumulation).  Every tiling gives the same bits."""
    from deephar_amd import functional as F
    from deephar_amd._lib import DeepharHipError
    n, h, w, cin, cout = case
    x, k, ps, pb, res = _convt_inputs(case)
    t = lambda v: torch.from_numpy(v).double()
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(cuda)
    failures = []
    for name, flags in VARIANTS:
        bn, has_res, post = 'bn' in flags, 'res' in flags, 'post' in flags
        kw = dict(pre_scale=d(ps) if bn else None, pre_shift=d(pb) if bn else None, pre_relu=bn,
                  res=d(res) if has_res else None, post_relu=post)
        if not _eligible(hip_lib, case, bn):
            for mode in MODES:                       # refused, never run on another kernel
                with pytest.raises(DeepharHipError, match=UNSUPPORTED):
                    F.conv2d_transpose(d(x), k, precision=mode, **kw)
            continue

        def epilogue(y):
            y = y + t(res) if has_res else y
            return O.relu(y) if post else y
        truth = RS.conv_transpose2x2(t(x), t(k), t(ps) if bn else None, t(pb) if bn else None, bn, t(res) if has_res else None,
                                     post)
        a = _operand(x, ps if bn else None, pb if bn else None, bn).double()
        f32 = F.conv2d_transpose(d(x), k, **kw)
        e_f32 = (f32.cpu().double() - truth).abs().max().item()
        for mode in MODES:
            ref = epilogue(R.conv_ep(_convt, a, t(k), None, None, R.PARTS[mode]))
            outs = _tilings(hip_lib, lambda cfg: F.conv2d_transpose(d(x), k, precision=mode, tile_cfg=cfg, **kw))
            first = outs[-1]
            for cfg, y in outs.items():
                assert torch.equal(y, first), '%s %s tiling %d differs' % (name, mode, cfg)
            e_mode = (first.cpu().double() - ref).abs().max().item()
            e_true = (first.cpu().double() - truth).abs().max().item()
            print('convT %s %s %s: |hip - E_P| = %.3e   |fp32 kernel - fp64| = %.3e   |hip - fp64| = %.3e' % (
                case, name, mode, e_mode, e_f32, e_true))
            if not e_mode <= 2.0 * e_f32 + 1e-6:
                failures.append((name, mode, 'bar', e_mode, e_f32))
            if R.PARTS[mode] <= 2:
                # the mode is engaged: nearer to E_P than to the fp64 truth, and not the fp32 kernel's answer
                if not e_mode < e_true:
                    failures.append((name, mode, 'not E_P', e_mode, e_true))
                assert not torch.equal(first, f32), (name, mode)
    assert not failures, failures


def test_other_part_counts_and_geometries_are_refused(hip_lib, cuda):
    from deephar_amd import functional as F, _lib
    x = torch.zeros((1, 4, 4, 32), device=cuda)
    k = np.zeros((2, 2, 16, 32), np.float32)
    with pytest.raises(ValueError):
        F.conv2d_transpose(x, k, precision='bf16x4')
    with pytest.raises(NotImplementedError):
        F.conv2d_transpose(x, np.zeros((3, 3, 16, 32), np.float32), precision='bf16')
    assert torch.equal(F.conv2d_transpose(x + 1, k + 1), F.conv2d_transpose(x + 1, k + 1, precision='f32'))
    # an fp32 packing handed to a split mode has the wrong size only by accident of the caller: parts out of range is EINVAL
    wt, kp, np_ = F.pack_convt_weight(k, cuda, parts=2)
    a = _lib.ConvtArgs()
    y = torch.zeros((1, 8, 8, 16), device=cuda)
    a.x, a.w, a.y = x.data_ptr(), wt.data_ptr(), y.data_ptr()
    a.N, a.H, a.W, a.Cin, a.ldx, a.Cout, a.ldy, a.Kp, a.Np = 1, 4, 4, 32, 32, 16, 16, kp, np_
    s = torch.cuda.current_stream().cuda_stream
    assert hip_lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), 0, -1, s) == -1
    assert hip_lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), 4, -1, s) == -1
    assert hip_lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), 2, hip_lib.dh_conv2d_transpose2x2_num_split_tile_cfgs(), s) == -1
    assert hip_lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), 2, -1, s) == 0
    torch.cuda.synchronize()


# ---- 3. invariance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', [(3, 4, 4, 576, 480), (3, 8, 8, 480, 384), (3, 3, 5, 48, 20), (3, 4, 4, 36, 24)])
def test_bits_depend_on_the_mode_and_the_geometry_only(case, mode, hip_lib, cuda):
    from deephar_amd import functional as F
    n, h, w, cin, cout = case
    assert _eligible(hip_lib, case, True)
    x, k, ps, pb, res = _convt_inputs(case, seed=5)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(cuda)
    kw = dict(pre_scale=d(ps), pre_shift=d(pb), pre_relu=True, precision=mode)
    full = F.conv2d_transpose(d(x), k, res=d(res), **kw)
    one = F.conv2d_transpose(d(x[:1]), k, res=d(res[:1]), **kw)
    last = F.conv2d_transpose(d(x[-1:]), k, res=d(res[-1:]), **kw)
    assert torch.equal(full[:1], one) and torch.equal(full[-1:], last)
    ncfg = hip_lib.dh_conv2d_transpose2x2_num_split_tile_cfgs()
    assert ncfg >= 3
    for cfg in range(ncfg):
        assert torch.equal(F.conv2d_transpose(d(x), k, res=d(res), tile_cfg=cfg, **kw), full), cfg
        assert torch.equal(F.conv2d_transpose(d(x[:1]), k, res=d(res[:1]), tile_cfg=cfg, **kw), one), cfg
    plain = F.conv2d_transpose(d(x), k, **kw)
    # channel slabs: ldx > Cin (the padded k slots of a pixel hold the slab's neighbours), ldy > Cout; the padding stays
    xw = np.concatenate([x, np.full((n, h, w, 8), 3.0, np.float32)], axis=-1)
    for pad_y in (12, 1, 5):                                 # (a pitch that is no multiple of four: the scalar store path)
        for cfg in (-1, 0, ncfg - 1):
            out = torch.full((n, 2 * h, 2 * w, cout + pad_y), 7.0, device=cuda)
            F.conv2d_transpose(d(xw), k, channels=cin, out=out, tile_cfg=cfg, **kw)
            assert torch.equal(out[..., :cout], plain), (pad_y, cfg)
            assert torch.all(out[..., cout:] == 7.0), (pad_y, cfg)
    # a packed weight handed in gives the same bits as packing on the fly
    packed = F.pack_convt_weight(k, cuda, parts=R.PARTS[mode])
    assert torch.equal(F.conv2d_transpose(d(x), k, packed=packed, **kw), plain)


# ---- 4. models ----------------------------------------------------------------------------------------------------------
def _emulate(mp, parts):
    """The fp64 restatement as the mode: oracle.ops.conv2d (bf16_modes_ref.emulate) AND the transposed convolution of
    tests/resample_ref.py evaluated as E_P (its caller has applied BN and ReLU: the operand is the post-prologue one)."""
    R.emulate(mp, parts)
    orig = RS.conv_transpose2x2

    def conv_transpose2x2(x, w, pre_scale=None, pre_shift=None, pre_relu=False, res=None, post_relu=False):
        if pre_scale is not None:
            x = x * pre_scale + pre_shift
        if pre_relu:
            x = O.relu(x)
        y = R.conv_ep(lambda a, b, s, p: orig(a, b), x, w, None, None, parts)
        if res is not None:
            y = y + res
        return O.relu(y) if post_relu else y

    mp.setattr(RS, 'conv_transpose2x2', conv_transpose2x2)


def _model_case(name):
    """-> (model, x, restatement(dtype) -> list of arrays, read-out(outputs) -> the arrays the distance is taken over)"""
    if name == 'mini':
        m, wd = _mini_pyramid()
        x = np.random.default_rng(21).standard_normal((2, 16, 16, 96)).astype(np.float32)
        return m, x, lambda dt: [RS.mini_pyramid(wd, x, dtype=dt)], lambda o: list(o)
    # The 1e-3 px floor is the project's bar for read-outs conditioned like a trained network's (tests/wellcond.py): on noise
    # frames with un-fitted heads the fp32 CPU restatement itself is 1 .. 1.5e-3 px from fp64.  So, as
    # test_gpu_resampling_models.py does for its clip model: two frames of one smooth video, heads fitted to one peak per
    # joint, conditioning asserted on the fp64 restatement.
    import wellcond
    from deephar_amd import weights
    layout = {'spnet2d': 'pa16j2d', 'spnet3d': 'pa17j3d'}[name]
    m, rcfg = _pose_spnet(layout)
    x = wellcond.video_cuts(1, 2, 128, 13)
    x = np.ascontiguousarray(x.reshape((2,) + x.shape[2:]))
    RS.fit_pose_heads(m, rcfg, x, wellcond.scene_positions(1, 2, rcfg['num_joints'], 13))
    wd = weights.as_dict(m)
    t64 = {}
    RS.spnet_pose_forward(wd, x, rcfg, dtype=torch.float64, taps=t64)
    wellcond.assert_well_conditioned(t64, name)
    return m, x, lambda dt: RS.spnet_pose_forward(wd, x, rcfg, dtype=dt), lambda o: [v[..., :rcfg['dim']] for v in o]


@pytest.mark.parametrize('name', ['mini', 'spnet2d', 'spnet3d'])
def test_models_within_the_emulated_bar(name, hip_lib, cuda, monkeypatch):
    """The rule of test_gpu_bf16_modes.test_models_within_the_emulated_bar on the learned-resampling builders of
    tests/test_gpu_resampling_models.py: per mode emu_px = distance of the CPU emulation of the mode from the fp64 restatement,
    the engine must stay within max(1e-3 px, 2 x emu_px) of the fp64 restatement (px = 256 x the worst absolute difference:
    normalised pose coordinates of the SPNets; for the mini pyramid, whose output is an O(1) feature map, the same 256 x)."""
    m, x, restate, readout = _model_case(name)
    n = len(x)
    o64 = restate(torch.float64)
    m.gemm_precision = 'f32'
    m.executor.autotune = False                      # (every tiling gives the same bits; keeps the test to seconds)
    f32 = m.predict(x, batch_size=n)
    f32 = f32 if isinstance(f32, list) else [f32]
    nct = sum(1 for s in m.plan.steps if s.kind == 'convtranspose')
    assert nct >= 3 and all(s.attrs.get('w_split') == 0 for s in m.plan.steps if s.kind == 'convtranspose')
    failures = []
    for mode in MODES:
        with monkeypatch.context() as mp:
            _emulate(mp, R.PARTS[mode])
            emu = restate(torch.float64)
        emu_px = R.px(readout(emu), readout(o64))
        assert np.isfinite(emu_px)
        m.gemm_precision = mode
        m.executor.autotune = False
        hip = m.predict(x, batch_size=n)
        hip = hip if isinstance(hip, list) else [hip]
        ct = [s for s in m.plan.steps if s.kind == 'convtranspose']
        assert len(ct) == nct and all(s.attrs.get('w_split') == CODES[mode] for s in ct), [s.attrs.get('w_split') for s in ct]
        assert all(np.all(np.isfinite(v)) for v in hip)
        hip_px, vs_f32 = R.px(readout(hip), readout(o64)), R.px(readout(hip), readout(f32))
        bar = max(1e-3, 2.0 * emu_px)
        print(json.dumps(dict(case=name, mode=mode, emu_px=emu_px, bar_px=bar, hip_vs_o64_px=hip_px, hip_vs_f32_path_px=vs_f32,
                              f32_path_vs_o64_px=R.px(readout(f32), readout(o64)))))
        assert any(not np.array_equal(a, b) for a, b in zip(hip, f32)), 'the %s plan returned the fp32 plan\'s bits' % mode
        if hip_px > bar:
            failures.append('%s %s: %.3e px from the fp64 restatement, bar %.3e px (emulation %.3e px)' % (name, mode, hip_px, bar, emu_px))
    assert not failures, failures


def test_a_layer_the_library_refuses_falls_back_to_fp32(hip_lib, cuda, monkeypatch):
    """The binding asks dh_conv2d_transpose2x2_split_eligible with the final struct: a refusal binds the fp32 entry point."""
    from deephar_amd import _lib
    m, _ = _mini_pyramid()
    m.gemm_precision = 'bf16x2'
    x = np.random.default_rng(3).standard_normal((1, 16, 16, 96)).astype(np.float32)
    lib = _lib.load()
    engaged = m.predict(x, batch_size=1)
    assert all(s.attrs['w_split'] == 3 for s in m.plan.steps if s.kind == 'convtranspose')

    class Refusing:
        def __getattr__(self, name):
            return (lambda *a: 0) if name == 'dh_conv2d_transpose2x2_split_eligible' else getattr(lib, name)
    m2, _ = _mini_pyramid()
    m2.gemm_precision = 'bf16x2'
    from deephar_amd.engine import executor
    monkeypatch.setattr(executor._lib, 'load', lambda: Refusing())
    refused = m2.predict(x, batch_size=1)
    ct = [s for s in m2.plan.steps if s.kind == 'convtranspose']
    assert len(ct) == 3 and all(s.attrs['w_split'] == 0 for s in ct)
    # the convolutions are bound as in the engaged plan (in this small pyramid they are skinny or BN-prologue layers: fp32)
    convs = lambda mm: [(s.name, s.attrs.get('w_split')) for s in mm.plan.steps if s.kind == 'conv']
    assert convs(m2) == convs(m) and len(convs(m)) >= 3
    assert np.all(np.isfinite(refused)) and not np.array_equal(refused, engaged)


# ---- 5. exported plan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES + ('f32',))
def test_c_plan_reproduces_predict(mode, hip_lib, cuda, tmp_path):
    m, _ = _pose_spnet('pa16j2d')
    x = np.random.default_rng(17).uniform(-1, 1, (2, 128, 128, 3)).astype(np.float32)
    m.gemm_precision = mode
    m.executor.autotune = False
    n = len(x)
    ref = m.predict(x, batch_size=n)
    code = CODES.get(mode, 0)
    ct = [s for s in m.plan.steps if s.kind == 'convtranspose']
    assert len(ct) >= 3 and all(s.attrs['w_split'] == code for s in ct)
    path = str(tmp_path / 'model.dhplan')
    nbytes = m.export_plan(path, n)
    blob = open(path, 'rb').read()
    assert len(blob) == nbytes and blob[:4] == b'DHPL'
    assert int.from_bytes(blob[4:8], 'little') == (3 if mode == 'f32' else 4)
    plan = C.c_void_p()
    assert hip_lib.dh_plan_create(blob, len(blob), C.byref(plan)) == 0
    try:
        assert hip_lib.dh_plan_batch(plan) == n and hip_lib.dh_plan_num_outputs(plan) == len(ref)
        xd = torch.from_numpy(x).to(cuda)
        outs = [torch.full(r.shape, float('nan'), device=cuda) for r in ref]
        ins_p = (C.c_void_p * 1)(xd.data_ptr())
        outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        assert hip_lib.dh_forward(plan, ins_p, n, outs_p, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        for o, r in zip(outs, ref):
            assert np.array_equal(o.cpu().numpy(), r)
        host = [np.full(r.shape, np.nan, np.float32) for r in ref]
        ins_h = (C.c_void_p * 1)(x.ctypes.data)
        outs_h = (C.c_void_p * len(host))(*[h_.ctypes.data for h_ in host])
        assert hip_lib.dh_forward_host(plan, ins_h, n, outs_h) == 0
        for h_, r in zip(host, ref):
            assert np.array_equal(h_, r)
    finally:
        assert hip_lib.dh_plan_destroy(plan) == 0
