"""Host-side tests of Conv2DTranspose on the split-bf16 precision ladder (dh_conv2d_transpose2x2_split_f32, csrc/convt2x2s.hip;
Model.gemm_precision = 'bf16x3' / 'bf16x2' / 'bf16' on a downsampling_type='conv' SPNet): exported symbols, the parts packing of
the [Cin, 4 Cout] matrix, the eligibility rule and the plan blob's function table.  No GPU needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_modes_ref as R                          # noqa: E402

NEW_SYMBOLS = ('dh_conv2d_transpose2x2_split_f32', 'dh_conv2d_transpose2x2_split_eligible',
               'dh_conv2d_transpose2x2_num_split_tile_cfgs')
DH_EINVAL = -1
# (N, H, W, Cin, Cout): the up-scaling geometries of a 256-px SPNet, then the odd ones of tests/test_gpu_resampling_ops.py
SPNET_GEOMETRIES = [(2, 4, 4, 576, 480), (2, 8, 8, 480, 384), (1, 16, 16, 384, 288)]
K_MAX_PRE = 4096                                    # csrc/conv_common.h: kMaxPreKp


def _args(case, prologue=True, x=0x10000, ldx=None, ldy=None):
    """dh_conv_transpose for a geometry, with fake (never dereferenced) 16-byte aligned pointers."""
    from deephar_amd import _lib
    n, h, w, cin, cout = case
    a = _lib.ConvtArgs()
    a.x, a.w, a.y = x, 0x20000, 0x30000
    if prologue:
        a.pre_scale, a.pre_shift = 0x40000, 0x50000
    a.N, a.H, a.W, a.Cin, a.ldx = n, h, w, cin, cin if ldx is None else ldx
    a.Cout, a.ldy, a.ldr = cout, cout if ldy is None else ldy, 0
    a.Kp, a.Np = (cin + 31) // 32 * 32, (4 * cout + 31) // 32 * 32
    a.pre_relu, a.post_relu = 1, 0
    return a


# ---- symbols -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(hip_lib):
    from deephar_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'deephar_hip.h')).read()
    declared = set(re.findall(r'\b(dh_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.dh_conv2d_transpose2x2_num_split_tile_cfgs() >= 2
    assert 'no reduced-precision form' not in hdr


@pytest.mark.parametrize('parts', [0, 4, -1, 6])
def test_other_part_counts_are_invalid_without_a_launch(parts, hip_lib):
    """Answered before anything touches a device: the pointers are fake and this host has no GPU."""
    a = _args(SPNET_GEOMETRIES[0])
    assert hip_lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), parts, -1, None) == DH_EINVAL


# ---- packing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cout,cin', [(20, 48), (16, 32), (24, 36), (288, 384)])
def test_pack_convt_parts(cout, cin, hip_lib):
    from deephar_amd.engine import packing
    rng = np.random.default_rng(cout + cin)
    w = (rng.standard_normal((2, 2, cout, cin)) * rng.choice([1e-3, 1.0, 37.0], (2, 2, cout, cin))).astype(np.float32)
    b = packing.convt_matrix(w)
    assert b.shape == (1, 1, cin, 4 * cout)
    f32, kp, np_ = packing.pack_convt(w)
    none, kp0, np0 = packing.pack_convt(w, parts=None)
    ref32, _, _ = packing.pack_conv(b)
    assert (kp, np_) == (kp0, np0) and f32.dtype == np.float32
    assert f32.tobytes() == none.tobytes() == ref32.tobytes()           # parts=None: today's fp32 packing, bit for bit
    for parts in (1, 2, 3):
        got, kp_p, np_p = packing.pack_convt(w, parts=parts)
        ref, _, _ = packing.pack_conv_split(b, parts=parts)
        assert (kp_p, np_p) == (kp, np_) and got.tobytes() == ref.tobytes()
        assert got.view(np.uint16).size == parts * kp * np_
        tot, pt = packing.unpack_conv_split(got, 1, 1, cin, 4 * cout, parts=parts)
        want = sum(p.double() for p in R.split_parts(torch.from_numpy(b), parts)).numpy()
        assert np.array_equal(tot, want)                                  # fp64 sums of exactly representable parts
        if parts == 3:
            assert np.array_equal(tot.astype(np.float32), b)
        # the padding (k >= Cin, n >= 4 Cout) is zero in every part
        full = pt.astype(np.float64).transpose(1, 0, 3, 2).reshape(parts, kp, np_)
        assert not full[:, cin:].any() and not full[:, :, 4 * cout:].any()
    with pytest.raises(ValueError):
        packing.pack_convt(w, parts=4)


# ---- eligibility -------------------------------------------------------------------------------------------------------
def test_eligibility_is_a_rule_on_geometry_and_alignment(hip_lib):
    el = hip_lib.dh_conv2d_transpose2x2_split_eligible
    for case in SPNET_GEOMETRIES + [(2, 3, 5, 48, 20)]:
        for prologue in (True, False):
            assert el(C.byref(_args(case, prologue))) == 1, (case, prologue)
        # never the batch size: 1 .. 4096 frames of the same layer answer alike
        for n in (1, 3, 64, 4096):
            assert el(C.byref(_args((n,) + case[1:]))) == 1, (case, n)
    case = SPNET_GEOMETRIES[1]
    assert el(C.byref(_args(case, x=0x10004))) == 0                        # x not 16-byte aligned
    assert el(C.byref(_args(case, ldx=case[3] + 2))) == 0                  # ldx % 4 != 0
    assert el(C.byref(_args(case, ldx=case[3] + 8))) == 1                  # a channel slab of a wider buffer
    assert el(C.byref(_args(case, ldy=case[4] + 1))) == 1                  # (the scalar store path is still this kernel)
    big = (1, 4, 4, K_MAX_PRE + 32, 64)                                     # scale / shift tables beyond the LDS budget
    assert el(C.byref(_args(big, prologue=True))) == 0
    assert el(C.byref(_args(big, prologue=False))) == 1
    assert el(C.byref(_args((1, 4, 4, K_MAX_PRE, 64), prologue=True))) == 1
    assert el(C.byref(_args((1, 4, 4, 34, 16)))) == 0                      # Cin % 4 != 0
    assert el(None) == 0
    half = _args(case)
    half.pre_shift = None                                                  # scale without shift: not a valid call
    assert el(C.byref(half)) == 0


# ---- serialisation -----------------------------------------------------------------------------------------------------
def test_function_table_appends_the_split_entry_point_as_version_4(hip_lib):
    from deephar_amd.engine import serialize as S
    assert S.ALL_FUNCTIONS[:21] == S.FUNCTIONS[:21] and len(S.FUNCTIONS) == 21
    assert S.FUNCTIONS[:21] == [
        'dh_conv2d_f32', 'dh_dwconv2d_f32', 'dh_pool2d_f32', 'dh_upsample2x_add_f32', 'dh_eltwise_f32', 'dh_softargmax2d_f32',
        'dh_context_aggregation_f32', 'dh_depth_means_f32', 'dh_softargmax1d_f32', 'dh_kronecker_f32',
        'dh_global_maxmin_softmax_f32', 'dh_copy_channels_f32', 'dh_zeropad2d_f32', 'dh_depth_from_maps_f32',
        'dh_softargmax2d_context_f32', 'dh_normalize_u8_f32', 'dh_conv2d_dw_group_f32', 'dh_conv2d_pair_f32', 'dh_conv2d_seg_f32',
        'dh_dwconv2d_strided_f32', 'dh_conv2d_transpose2x2_f32']
    new = S.ALL_FUNCTIONS.index('dh_conv2d_transpose2x2_split_f32')
    assert new == 21 and len(S.ALL_FUNCTIONS) == 22
    assert S.blob_version([0, 1, new, 20]) == 4                            # the new id makes version 4 ...
    assert S.blob_version([0, 19, 20]) == 3 and S.blob_version([0, 4, 18]) == 2 and S.blob_version([]) == 2   # ... nothing else does
    # the C executor's table has the same order, and the same versions (dh_plan_record: csrc/plan_blob.h)
    from deephar_amd import _lib
    records = [_lib.plan_record(hip_lib, fn) for fn in range(len(S.ALL_FUNCTIONS))]
    assert [r[0] for r in records] == S.ALL_FUNCTIONS and _lib.plan_record(hip_lib, len(S.ALL_FUNCTIONS)) is None
    assert [r[1] for r in records[18:]] == [1, 3, 3, 4] and {r[1] for r in records[:19]} == {1}


def test_the_ctypes_signature_serialises_as_struct_plus_two_integers():
    """serialize.dump_plan writes the struct byte for byte and one u64 per further argument: parts, tile_cfg."""
    from deephar_amd import _lib
    sig = _lib.SIGNATURES['dh_conv2d_transpose2x2_split_f32'][1]
    assert sig[0]._type_ is _lib.ConvtArgs and sig[1:] == [C.c_int, C.c_int, C.c_void_p]
    assert C.sizeof(_lib.ConvtArgs) == 96
