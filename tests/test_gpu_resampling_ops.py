"""GPU op tests of the learned-resampling kernels (downsampling_type='conv'): the stride-2 depthwise convolution
(dh_dwconv2d_strided_f32), the transposed 2x2 / stride-2 convolution (dh_conv2d_transpose2x2_f32) and the stride-2 pointwise
shortcut through dh_conv2d_f32, against the restatements of tests/resample_ref.py / oracle.ops."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R                           # noqa: E402
from oracle import ops as O                        # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 2e-5


def _rand(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _close(got, ref, atol, rtol=RTOL, what=''):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    ref = ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    tol = atol + rtol * np.abs(ref)
    print('%s: max err %.3e' % (what, err.max()))
    assert np.all(err <= tol), '%s: max err %.3e (tol %.3e) at %s' % (
        what, err.max(), tol.flat[err.argmax()], np.unravel_index(err.argmax(), err.shape))


# ---- 5. strided depthwise ------------------------------------------------------------------------------------------
DW_CASES = [(2, 8, 8, 40, 5), (2, 6, 10, 96, 5), (1, 7, 9, 32, 5), (3, 4, 4, 288, 5), (2, 2, 2, 64, 5), (2, 8, 8, 40, 3)]


@pytest.mark.parametrize('case', DW_CASES)
def test_strided_depthwise(case, hip_lib, cuda):
    """Against the restatement (tolerance of test_dwconv: atol 1e-5, rtol 2e-5), for the three prologues and for channel
    slabs of wider buffers (ldx, ldy > C: nothing outside the slab is read into the result or written)."""
    from deephar_amd import functional as F
    n, h, w, c, k = case
    rng = np.random.default_rng(sum(case))
    x = _rand(rng, (n, h, w, c))
    dw = _rand(rng, (k, k, c, 1), 1.0 / k)
    ps, pb = rng.uniform(0.5, 1.5, c).astype(np.float32), _rand(rng, (c,), 0.3)
    t = lambda a: torch.from_numpy(a)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    variants = [('plain', dict(), dict()), ('relu', dict(pre_relu=True), dict(pre_relu=True)),
                ('bn relu', dict(pre_scale=d(ps), pre_shift=d(pb), pre_relu=True),
                 dict(pre_scale=t(ps), pre_shift=t(pb), pre_relu=True))]
    for name, kw, rkw in variants:
        ref = R.dwconv_strided(t(x), t(dw), (2, 2), **rkw)
        got = F.dwconv2d_strided(d(x), dw, (2, 2), **kw)
        assert tuple(got.shape) == (n, -(-h // 2), -(-w // 2), c)
        _close(got, ref, atol=1e-5, what='strided dw %s %s' % (name, case))
    # slabs: the input is the first c channels of a (c + 8)-channel tensor, the output the first c of a (c + 4)-channel one
    for pad_x, pad_y in ((8, 4), (3, 5)):                   # (a pitch that is no multiple of four takes the scalar kernel)
        xw = np.concatenate([x, np.full((n, h, w, pad_x), 1e3, np.float32)], axis=-1)
        out = torch.full((n, -(-h // 2), -(-w // 2), c + pad_y), 7.0, device=cuda)
        F.dwconv2d_strided(d(xw), dw, (2, 2), pre_scale=d(ps), pre_shift=d(pb), pre_relu=True, channels=c, out=out)
        ref = R.dwconv_strided(t(x), t(dw), (2, 2), pre_scale=t(ps), pre_shift=t(pb), pre_relu=True)
        _close(out[..., :c], ref, atol=1e-5, what='strided dw slab %s' % (case,))
        assert torch.all(out[..., c:] == 7.0)
        # the vector and the scalar kernel sum in the same order: same bits whatever the alignment
        assert torch.equal(out[..., :c], F.dwconv2d_strided(d(x), dw, (2, 2), pre_scale=d(ps), pre_shift=d(pb), pre_relu=True))


@pytest.mark.parametrize('case', [c for c in DW_CASES if c[4] == 5])
def test_strided_depthwise_equals_the_stride_1_kernel_at_the_same_windows(case, hip_lib, cuda):
    """TF-SAME at stride 2 pads (1, 2) on an even extent, (2, 2) on an odd one; at stride 1, (2, 2): output i of the strided
    convolution is output 2i + 1 (even extents) / 2i (odd extents) of the stride-1 one -- the SAME window, summed in the
    same order, so the values are bit-identical to dh_dwconv2d_f32's."""
    from deephar_amd import functional as F
    n, h, w, c, k = case
    rng = np.random.default_rng(sum(case) + 1)
    x = _rand(rng, (n, h, w, c))
    dw = _rand(rng, (k, k, c, 1), 1.0 / k)
    ps, pb = rng.uniform(0.5, 1.5, c).astype(np.float32), _rand(rng, (c,), 0.3)
    d = lambda a: torch.from_numpy(a).to(cuda)
    assert h % 2 == w % 2
    o = 1 if h % 2 == 0 else 0
    for kw in (dict(), dict(pre_relu=True), dict(pre_scale=d(ps), pre_shift=d(pb), pre_relu=True)):
        y1 = F.dwconv2d(d(x), dw, **kw).cpu().numpy()
        y2 = F.dwconv2d_strided(d(x), dw, (2, 2), **kw).cpu().numpy()
        assert np.array_equal(y2, y1[:, o::2, o::2]), sorted(kw)


def test_strided_depthwise_refuses_other_geometries(hip_lib, cuda):
    from deephar_amd import functional as F, _lib
    x = torch.zeros((1, 8, 8, 8), device=cuda)
    with pytest.raises(_lib.DeepharHipError):
        F.dwconv2d_strided(x, np.zeros((5, 5, 8, 1), np.float32), (3, 3))
    with pytest.raises(_lib.DeepharHipError):
        F.dwconv2d_strided(x, np.zeros((7, 7, 8, 1), np.float32), (2, 2))


# ---- 6. transposed convolution ---------------------------------------------------------------------------------------
CONVT_CASES = [(2, 4, 4, 576, 480), (2, 8, 8, 480, 384), (1, 16, 16, 384, 288), (2, 3, 5, 48, 20), (1, 1, 1, 32, 16),
               (3, 4, 4, 36, 24)]
TAP_PATTERN = np.array([[1.0, -0.5], [2.0, -1.5]], np.float32)      # a swapped (a, b) changes sign or scale


def _convt_inputs(case, seed=0):
    n, h, w, cin, cout = case
    rng = np.random.default_rng(sum(case) + seed)
    x = _rand(rng, (n, h, w, cin))
    k = _rand(rng, (2, 2, cout, cin), np.sqrt(1.0 / cin)) * TAP_PATTERN[:, :, None, None]
    ps, pb = rng.uniform(0.5, 1.5, cin).astype(np.float32), _rand(rng, (cin,), 0.3)
    res = _rand(rng, (n, 2 * h, 2 * w, cout))
    return x, k, ps, pb, res


@pytest.mark.parametrize('case', CONVT_CASES)
def test_conv2d_transpose(case, hip_lib, cuda):
    """Against conv_transpose2d (tolerance of the fused-conv tests: atol 3e-5, rtol 2e-5 against the fp32 restatement) and no
    further from fp64 than a few times the fp32 CPU result (as test_conv2d_plain), for every fused variant."""
    from deephar_amd import functional as F
    n, h, w, cin, cout = case
    x, k, ps, pb, res = _convt_inputs(case)
    t = lambda a: torch.from_numpy(a)
    t64 = lambda a: torch.from_numpy(a).double()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    variants = [('plain', {}), ('bn relu', dict(pre_scale=ps, pre_shift=pb, pre_relu=True)), ('res', dict(res=res)),
                ('res relu', dict(res=res, post_relu=True)),
                ('bn relu res', dict(pre_scale=ps, pre_shift=pb, pre_relu=True, res=res))]
    for name, kw in variants:
        conv = lambda f: {key: (f(v) if isinstance(v, np.ndarray) else v) for key, v in kw.items()}
        ref = R.conv_transpose2x2(t(x), t(k), **conv(t))
        ref64 = R.conv_transpose2x2(t64(x), t64(k), **conv(t64))
        got = F.conv2d_transpose(d(x), k, **conv(d))
        torch.cuda.synchronize()
        assert tuple(got.shape) == (n, 2 * h, 2 * w, cout)
        _close(got, ref, atol=3e-5, what='convT %s %s' % (name, case))
        e_hip = (got.cpu().double() - ref64).abs().max().item()
        e_cpu = (ref.double() - ref64).abs().max().item()
        print('convT %s %s: |hip - f64| %.3e, |cpu32 - f64| %.3e' % (name, case, e_hip, e_cpu))
        assert e_hip <= 4 * e_cpu + 1e-6, (name, e_hip, e_cpu)
    # channel slabs: ldx > Cin, ldy > Cout, the residual inside a wider tensor as well
    xw = np.concatenate([x, np.full((n, h, w, 8), 3.0, np.float32)], axis=-1)
    rw = np.concatenate([res, np.full(res.shape[:3] + (4,), 1e3, np.float32)], axis=-1)
    ref = R.conv_transpose2x2(t(x), t(k), t(ps), t(pb), True, t(res))
    for pad_y in (12, 5):                                    # (a pitch that is no multiple of four: the scalar store path)
        out = torch.full((n, 2 * h, 2 * w, cout + pad_y), 7.0, device=cuda)
        F.conv2d_transpose(d(xw), k, pre_scale=d(ps), pre_shift=d(pb), pre_relu=True, channels=cin, out=out)
        _close(out[..., :cout], R.conv_transpose2x2(t(x), t(k), t(ps), t(pb), True), atol=3e-5, what='convT slab %s' % (case,))
        assert torch.all(out[..., cout:] == 7.0)
    out = torch.full((n, 2 * h, 2 * w, cout + 12), 7.0, device=cuda)
    _convt_with_res_pitch(F, d(xw), k, d(ps), d(pb), d(rw), cin, out)
    _close(out[..., :cout], ref, atol=3e-5, what='convT slab + residual slab %s' % (case,))
    assert torch.all(out[..., cout:] == 7.0)


def _convt_with_res_pitch(F, x, k, ps, pb, res_wide, cin, out):
    """functional.conv2d_transpose with a residual whose pixel pitch is wider than Cout (res_wide [N, 2H, 2W, ldr])."""
    import ctypes as C
    from deephar_amd import _lib
    cout = k.shape[2]
    wt, kp, np_ = F.pack_convt_weight(k, x.device)
    a = _lib.ConvtArgs()
    a.x, a.w, a.y, a.pre_scale, a.pre_shift, a.res = x.data_ptr(), wt.data_ptr(), out.data_ptr(), ps.data_ptr(), pb.data_ptr(), \
        res_wide.data_ptr()
    a.N, a.H, a.W, a.Cin, a.ldx = x.shape[0], x.shape[1], x.shape[2], cin, x.shape[3]
    a.Cout, a.ldy, a.ldr, a.Kp, a.Np, a.pre_relu, a.post_relu = cout, out.shape[3], res_wide.shape[3], kp, np_, 1, 0
    _lib.check(_lib.load().dh_conv2d_transpose2x2_f32(C.byref(a), -1, torch.cuda.current_stream().cuda_stream), 'convT')
    torch.cuda.synchronize()


def test_conv2d_transpose_refuses_other_geometries(hip_lib, cuda):
    from deephar_amd import functional as F
    x = torch.zeros((1, 4, 4, 8), device=cuda)
    with pytest.raises(NotImplementedError, match=r'kernel_size=\(2, 2\), strides=\(2, 2\)'):
        F.conv2d_transpose(x, np.zeros((3, 3, 8, 8), np.float32))
    with pytest.raises(NotImplementedError, match=r'kernel_size=\(2, 2\), strides=\(2, 2\)'):
        F.conv2d_transpose(x, np.zeros((2, 2, 8, 8), np.float32), strides=(1, 1))


# ---- 7. batch and tiling independence ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(3, 4, 4, 576, 480), (3, 8, 8, 480, 384), (3, 3, 5, 48, 20), (3, 4, 4, 36, 24)])
def test_conv2d_transpose_bits_depend_on_neither_batch_nor_tiling(case, hip_lib, cuda):
    from deephar_amd import functional as F
    n, h, w, cin, cout = case
    x, k, ps, pb, res = _convt_inputs(case, seed=5)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    kw = dict(pre_scale=d(ps), pre_shift=d(pb), pre_relu=True)
    full = F.conv2d_transpose(d(x), k, res=d(res), **kw)
    one = F.conv2d_transpose(d(x[:1]), k, res=d(res[:1]), **kw)
    assert torch.equal(full[:1], one)
    ncfg = hip_lib.dh_conv2d_transpose2x2_num_tile_cfgs()
    assert ncfg >= 2
    for cfg in range(ncfg):
        assert torch.equal(F.conv2d_transpose(d(x), k, res=d(res), tile_cfg=cfg, **kw), full), cfg
        assert torch.equal(F.conv2d_transpose(d(x[:1]), k, res=d(res[:1]), tile_cfg=cfg, **kw), one), cfg
    # ... nor on the store path: a pitch that is no multiple of four takes the scalar epilogue
    out = torch.zeros((n, 2 * h, 2 * w, cout + 1), device=cuda)
    F.conv2d_transpose(d(x), k, out=out, **kw)
    assert torch.equal(out[..., :cout], F.conv2d_transpose(d(x), k, **kw))


@pytest.mark.parametrize('case', [(3, 8, 8, 40, 5), (3, 7, 9, 32, 5)])
def test_strided_depthwise_bits_do_not_depend_on_the_batch(case, hip_lib, cuda):
    from deephar_amd import functional as F
    n, h, w, c, k = case
    rng = np.random.default_rng(3)
    x, dw = _rand(rng, (n, h, w, c)), _rand(rng, (k, k, c, 1), 1.0 / k)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    assert torch.equal(F.dwconv2d_strided(d(x), dw, pre_relu=True)[:1], F.dwconv2d_strided(d(x[:1]), dw, pre_relu=True))


# ---- 8. the stride-2 pointwise shortcut --------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(2, 8, 8, 288, 384), (1, 7, 9, 32, 24)])
def test_pointwise_stride_2_conv(case, hip_lib, cuda):
    """The shortcut of the stride-2 residual unit (common.py:33-52 with strides=(2, 2)): a 1x1 convolution that reads pixels
    (2i, 2j) -- dh_conv2d_f32 must route it to a kernel that honours SH / SW, with the BN + ReLU prologue it carries."""
    from deephar_amd import functional as F
    n, h, w, cin, cout = case
    rng = np.random.default_rng(sum(case))
    x = _rand(rng, (n, h, w, cin))
    k = _rand(rng, (1, 1, cin, cout), np.sqrt(1.0 / cin))
    ps, pb = rng.uniform(0.5, 1.5, cin).astype(np.float32), _rand(rng, (cin,), 0.3)
    t = lambda a: torch.from_numpy(a)
    d = lambda a: torch.from_numpy(a).to(cuda)
    ref = O.conv2d(t(x), t(k), (2, 2), 'same')
    assert tuple(ref.shape) == (n, -(-h // 2), -(-w // 2), cout)
    assert torch.equal(ref, O.conv2d(t(np.ascontiguousarray(x[:, ::2, ::2])), t(k)))      # (it IS the sub-sampled pixels)
    _close(F.conv2d(d(x), k, (2, 2), 'same'), ref, atol=2e-5, what='1x1 stride 2 %s' % (case,))
    ref = O.conv2d(O.relu(t(x) * t(ps) + t(pb)), t(k), (2, 2), 'same')
    _close(F.conv2d(d(x), k, (2, 2), 'same', pre_scale=d(ps), pre_shift=d(pb), pre_relu=True), ref, atol=3e-5,
           what='1x1 stride 2, bn relu %s' % (case,))
