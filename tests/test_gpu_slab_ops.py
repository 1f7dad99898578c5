"""Op-level tests of the non-convolution kernels on channel-slab views (tests/slabview.py).

The planner hands nearly every kernel a (pointer, pitch) view: concat producers write into the concatenation's slab, the
soft-argmax reads its maps inside a slab of pitch 2 J, z lands in a column of a pose buffer; with 17 joints the channel
offsets are no multiples of four and the kernels of spatial.hip / decoder.hip drop from their float4 path to the scalar
one.  deephar_amd/functional.py only ever passes ld == C and an aligned base, so tests/test_gpu_ops.py sees the dense,
aligned variant of each kernel; here every entry point between dh_pool2d_f32 and dh_depth_from_maps_f32 (and
dh_normalize_u8_f32) runs on a non-dense view, an unaligned base, or both:

  * inputs lie in NaN-filled slabs (a read outside the view that reaches the result poisons it), outputs in slabs that
    hold a canary, checked bit for bit after every launch (SV.assert_untouched, inside _Out.get);
  * every operation is compared with a plain fp64 NumPy / torch-CPU statement, or bit for bit where it is exact;
  * where the vector and the scalar variant do the same arithmetic per element, all layouts must give identical bits.

Bars: the project's existing ones (3.9e-6 on coordinates; the tolerances of the dense tests in
test_gpu_ops.py) and, for the element-wise kernel against fp64, 2**-22 * S with S the sum of the absolute values of the
terms: at most four roundings of partial sums no larger than S, contracted into an fma or not.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slabview as SV                              # noqa: E402
from oracle import ops as O                        # noqa: E402

pytestmark = pytest.mark.gpu

DH_EINVAL = -1
BAR = 3.9e-6          # 1e-3 px of a 256-px crop in normalised units
RTOL = 2e-5           # test_gpu_ops.RTOL


def _lib():
    from deephar_amd import _lib as lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(rc, what):
    _lib().check(rc, what)
    torch.cuda.synchronize()


def _rand(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _close(got, ref, atol, rtol=RTOL, what=''):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    tol = atol + rtol * np.abs(ref)
    print('%s: max err %.3e' % (what, np.nanmax(err)))
    assert np.all(err <= tol), '%s: max err %.3e (tol %.3e) at %s' % (
        what, np.nanmax(err), tol.flat[np.nanargmax(err)], np.unravel_index(np.nanargmax(err), err.shape))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class _In:
    """An input view: `values` [..., C] inside a NaN-filled slab."""

    def __init__(self, values, ld, off):
        self.t, self.ptr = SV.slab(values, ld, off, np.nan)
        self.ld, self.off = ld, off


class _Out:
    """An output view of `shape` = [..., C] inside a slab of canaries; get() checks the canaries and returns the values."""

    def __init__(self, shape, ld, off, as_shape=None):
        self.t, self.ptr = SV.out_slab(shape, ld, off)
        self.ld, self.off, self.C, self.as_shape = ld, off, shape[-1], as_shape

    def get(self, what=''):
        SV.assert_untouched(self.t, self.off, self.C, what=what)
        v = SV.view(self.t, self.off, self.C)
        return v.reshape(self.as_shape) if self.as_shape is not None else v


def _in(values, name, k=0):
    return _In(values, *SV.layout(np.shape(values)[-1], name, k))


def _out(shape, name, k=0):
    return _Out(shape, *SV.layout(shape[-1], name, k))


def _flat_in(values, lead):
    """A DENSE input tensor whose base lies `lead` floats into a NaN-filled buffer (lead % 4 != 0: not 16-byte aligned)."""
    v = np.asarray(values, np.float32).reshape(1, -1)
    return _In(v, v.size + lead + 3, lead)


def _flat_out(shape, lead):
    """A DENSE output tensor of `shape` at `lead` floats into a buffer of canaries."""
    n = int(np.prod(shape))
    return _Out((1, n), n + lead + 3, lead, as_shape=tuple(shape))


def _all_same_bits(results, what):
    names = list(results)
    for n in names[1:]:
        assert SV.same_bits(results[names[0]], results[n]), '%s: layout %s differs from %s in bits' % (what, n, names[0])


# ------------------------------------------------------------------------------------------------------------------------
# 1. dh_eltwise_f32
# ------------------------------------------------------------------------------------------------------------------------
ELT_CASES = {
    # name: (op, b, c, affine, relu, bcast_b)
    'bn_relu': (0, False, False, True, 1, 0),        # the planner's BN-ReLU write-out
    'add': (0, True, False, False, 0, 0),
    'add3': (0, True, True, False, 0, 0),
    'add_bcast': (0, True, False, False, 0, 1),
    'affine_add3': (0, True, True, True, 0, 0),
    'mul': (1, True, False, False, 0, 0),
    'mul_bcast': (1, True, False, False, 0, 1),
    'sigmoid': (2, False, False, False, 0, 0),
    'sigmoid_add': (2, True, False, False, 0, 0),
}


def _elt_data(npix, ch, case):
    op, has_b, has_c, affine, relu, bcast = ELT_CASES[case]
    rng = np.random.default_rng(1000 + sorted(ELT_CASES).index(case))
    d = dict(a=_rand(rng, (npix, ch)), b=None, c=None, scale=None, shift=None)
    if has_b:
        d['b'] = _rand(rng, (npix, 1 if bcast else ch))
    if has_c:
        d['c'] = _rand(rng, (npix, ch))
    if affine:
        d['scale'], d['shift'] = _rand(rng, (ch,)), _rand(rng, (ch,))
    return d


def _elt_ref(d, case):
    """fp64 result and the bound on |fp32 result - it|: 2**-22 * S for op 0 / 1, 1e-5 relative for the sigmoid."""
    op, has_b, has_c, affine, relu, bcast = ELT_CASES[case]
    f8 = lambda v: np.asarray(v, np.float64)
    t = f8(d['a'])
    S = np.abs(t)
    if affine:
        S = np.abs(t * f8(d['scale'])) + np.abs(f8(d['shift']))
        t = t * f8(d['scale']) + f8(d['shift'])
    b = f8(d['b']) if has_b else 0.0           # [npix, 1] broadcasts over the channels
    c = f8(d['c']) if has_c else 0.0
    if op == 0:
        r = t + b + c
        S = S + np.abs(b) + np.abs(c)
        if relu:
            r = np.maximum(r, 0.0)             # 1-Lipschitz: the bound holds behind it
        return r, 2.0 ** -22 * S
    if op == 1:
        return t * b, 2.0 ** -22 * np.abs(t * b)
    r = 1.0 / (1.0 + np.exp(-(t + b)))
    return r, 1e-5 * np.abs(r)


def _elt_launch(hip_lib, cuda, d, case, name):
    op, has_b, has_c, affine, relu, bcast = ELT_CASES[case]
    npix, ch = d['a'].shape
    a = _lib().EltArgs()
    xa = _in(d['a'], name, 0)
    xb = _in(d['b'], name, 1) if has_b else None
    xc = _in(d['c'], name, 2) if has_c else None
    y = _out((npix, ch), name, 1)
    sc = _dev(d['scale'], cuda) if affine else None
    sh = _dev(d['shift'], cuda) if affine else None
    a.a, a.lda, a.y, a.ldy = xa.ptr, xa.ld, y.ptr, y.ld
    if xb is not None:
        a.b, a.ldb = xb.ptr, xb.ld
    if xc is not None:
        a.c, a.ldc = xc.ptr, xc.ld
    if affine:
        a.scale, a.shift = sc.data_ptr(), sh.data_ptr()
    a.npix, a.C, a.relu, a.op, a.bcast_b = npix, ch, relu, op, bcast
    _run(hip_lib.dh_eltwise_f32(C.byref(a), _stream()), 'dh_eltwise_f32 %s %s' % (case, name))
    return y.get('eltwise %s %s' % (case, name))


@pytest.mark.parametrize('case', sorted(ELT_CASES))
def test_eltwise_on_views(case, hip_lib, cuda):
    """keras add / multiply / sigmoid / stand-alone BN + ReLU on 126 pixels x 17 channels, every operand at its own pitch
    and offset: against fp64 within 2**-22 * S (sigmoid: 1e-5 relative), identical bits in the three layouts."""
    d = _elt_data(126, 17, case)
    ref, bound = _elt_ref(d, case)
    got = {}
    for name in SV.LAYOUTS:
        got[name] = _elt_launch(hip_lib, cuda, d, case, name)
        err = np.abs(got[name].astype(np.float64) - ref)
        print('eltwise %s %s: max err / bound %.3f' % (case, name, np.nanmax(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (case, name, np.nanmax(err))
    _all_same_bits(got, 'eltwise ' + case)


def test_eltwise_grid_stride(hip_lib, cuda):
    """2 048 x 576 elements are more than 4 096 work-groups x 256 threads: the kernel strides."""
    d = _elt_data(2048, 576, 'affine_add3')
    assert d['a'].size > 4096 * 256
    ref, bound = _elt_ref(d, 'affine_add3')
    got = _elt_launch(hip_lib, cuda, d, 'affine_add3', 'aligned')
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= bound), np.nanmax(err)


def test_eltwise_refusals(hip_lib, cuda):
    d = _elt_data(126, 17, 'affine_add3')
    xa, xb, y = _in(d['a'], 'dense'), _in(d['b'], 'dense'), _out((126, 17), 'dense')
    sc = _dev(d['scale'], cuda)

    def args(**kw):
        a = _lib().EltArgs()
        a.a, a.lda, a.y, a.ldy, a.b, a.ldb = xa.ptr, 17, y.ptr, 17, xb.ptr, 17
        a.npix, a.C = 126, 17
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert hip_lib.dh_eltwise_f32(C.byref(args(npix=0)), _stream()) == DH_EINVAL
    assert hip_lib.dh_eltwise_f32(C.byref(args(op=1, b=None)), _stream()) == DH_EINVAL
    # a scale table without a shift table: the kernel would read shift[c] through a null pointer
    assert hip_lib.dh_eltwise_f32(C.byref(args(scale=sc.data_ptr(), shift=None)), _stream()) == DH_EINVAL
    torch.cuda.synchronize()
    y.get('eltwise refusals')


# ------------------------------------------------------------------------------------------------------------------------
# 2. dh_copy_channels_f32      3. dh_zeropad2d_f32
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('npix,ch,layouts', [(1, 1, SV.LAYOUTS), (126, 17, SV.LAYOUTS), (126, 20, SV.LAYOUTS),
                                             (8192, 576, ('aligned',))])
def test_copy_channels_on_views(npix, ch, layouts, hip_lib, cuda):
    """keras concatenate / channel slicing: bit-exact; (126, 20) runs the float4 kernel with a pitch and the scalar one,
    (8 192, 576) needs the grid stride on the float4 path (8 192 x 144 quads > 4 096 x 256)."""
    v = _rand(np.random.default_rng(npix + ch), (npix, ch))
    for name in layouts:
        x, y = _in(v, name, 0), _out((npix, ch), name, 1)
        _run(hip_lib.dh_copy_channels_f32(x.ptr, x.ld, y.ptr, y.ld, npix, ch, _stream()), 'dh_copy_channels_f32')
        assert SV.same_bits(y.get('copy %s' % name), v), name


@pytest.mark.parametrize('oh,ow,pt,pl', [(8, 20, 0, 0), (11, 20, 1, 2)])
def test_zeropad2d(oh, ow, pt, pl, hip_lib, cuda):
    """ZeroPadding2D (spnet.py:98-107) of [2, 8, 17, 5]: 17 joints padded to 20 at the right (PT = PL = 0), and all four
    sides at once; dense tensors as the planner guarantees, at bases that are not 16-byte aligned."""
    b, h, w, ch = 2, 8, 17, 5
    v = _rand(np.random.default_rng(oh + ow), (b, h, w, ch))
    x, y = _flat_in(v, 1), _flat_out((b, oh, ow, ch), 3)
    _run(hip_lib.dh_zeropad2d_f32(x.ptr, y.ptr, b, h, w, ch, oh, ow, pt, pl, _stream()), 'dh_zeropad2d_f32')
    ref = np.pad(v, ((0, 0), (pt, oh - h - pt), (pl, ow - w - pl), (0, 0)))
    assert SV.same_bits(y.get('zeropad'), ref)
    assert hip_lib.dh_zeropad2d_f32(x.ptr, y.ptr, b, h, w, ch, h + pt - 1, ow, pt, pl, _stream()) == DH_EINVAL


# ------------------------------------------------------------------------------------------------------------------------
# 4. dh_depth_from_maps_f32
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f,hw,j', [(3, 32 * 32, 17), (2, 7 * 9, 16), (2, 3, 5)])
def test_depth_from_maps_on_views(f, hw, j, hip_lib, cuda):
    """spnet.py:201-205: z = sum_p sigmoid(d) * h with h a channel soft-max (z is a coordinate in [0, 1]); d and h in slabs
    of different pitch, z in the third column of an [F, J, 3] pose buffer.  17 joints: two channel groups, the second
    ragged; 3 pixels: fewer than pixel lanes."""
    rng = np.random.default_rng(f + hw + j)
    d = _rand(rng, (f, hw, j), 2.0)
    m = rng.standard_normal((f, hw, j)) * 2.0
    e = np.exp(m - m.max(axis=1, keepdims=True))
    h = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    ref = (1.0 / (1.0 + np.exp(-d.astype(np.float64))) * h.astype(np.float64)).sum(axis=1)
    assert 0.0 <= ref.min() and ref.max() <= 1.0
    for name in SV.LAYOUTS:
        xd, xh, z = _in(d, name, 0), _in(h, name, 1), _Out((f, j, 1), 3, 2)
        _run(hip_lib.dh_depth_from_maps_f32(xd.ptr, xd.ld, xh.ptr, xh.ld, z.ptr, 3, f, hw, j, _stream()),
             'dh_depth_from_maps_f32')
        got = z.get('depth_from_maps %s' % name)[..., 0]
        err = np.abs(got.astype(np.float64) - ref).max()
        print('depth_from_maps %s %s: %.3e' % ((f, hw, j), name, err))
        assert err <= BAR, (name, err)


# ------------------------------------------------------------------------------------------------------------------------
# 5. dh_softargmax2d_f32
# ------------------------------------------------------------------------------------------------------------------------
SAM_OUTPUTS = ('xy', 'conf_raw', 'conf_prob', 'prob', 'gmax')


@functools.lru_cache(maxsize=None)
def _sam_case(shape):
    """N(0, 4^2) maps and the CPU oracle's read-outs, computed once per shape.  Precondition, on the reference alone: the
    fp32 oracle's coordinates lie within a quarter of the bar of the fp64 ones."""
    h = _rand(np.random.default_rng(sum(shape)), shape, 4.0)
    t = torch.from_numpy(h)
    p, p64 = O.channel_softmax_2d(t, 1.0), O.channel_softmax_2d(t.double(), 1.0)
    r = dict(h=h, prob=p.numpy(), xy=O.softargmax2d_from_prob(p).numpy(), xy64=O.softargmax2d_from_prob(p64).numpy(),
             conf_raw=O.joints_probability(4.0 * t).numpy(), conf_prob=O.joints_probability(p).numpy(),
             conf_prob64=O.joints_probability(p64).numpy(), gmax=torch.amax(t, dim=(1, 2)).numpy())
    e = np.abs(r['xy'].astype(np.float64) - r['xy64']).max()
    print('softargmax2d %s: fp32 CPU oracle vs fp64 %.3e' % (shape, e))
    assert e <= BAR / 4, (shape, e)
    return r


def _sam_launch(hip_lib, cuda, h, ldh, offh, want=SAM_OUTPUTS, ldxy=2, ldcr=1, ldcp=1, ldp=None, offp=0, flag=0):
    """One dh_softargmax2d_f32 launch (alpha 1, conf_scale 4) on maps at channel `offh` of `ldh`-float pixels; outputs not
    in `want` are NULL.  conf_raw / conf_prob land in the LAST column of their pitch."""
    f, hh, ww, ch = h.shape
    x = _In(h, ldh, offh)
    gx, gy = _dev(np.linspace(0.0, 1.0, num=ww).astype(np.float32), cuda), _dev(np.linspace(0.0, 1.0, num=hh).astype(np.float32), cuda)
    outs = dict(xy=_Out((f, ch, 2), ldxy, 0), conf_raw=_Out((f, ch, 1), ldcr, ldcr - 1),
                conf_prob=_Out((f, ch, 1), ldcp, ldcp - 1), prob=_Out((f, hh, ww, ch), ldp or ch, offp),
                gmax=_flat_out((f, ch), 0))
    outs = {k: v for k, v in outs.items() if k in want}
    a = _lib().SamArgs()
    a.h, a.gx, a.gy = x.ptr, gx.data_ptr(), gy.data_ptr()
    for k, o in outs.items():
        setattr(a, k, o.ptr)
    a.F, a.H, a.W, a.C, a.ldh, a.ldxy, a.ldcr, a.ldcp, a.ldp = f, hh, ww, ch, ldh, ldxy, ldcr, ldcp, ldp or ch
    a.alpha, a.conf_scale, a.xy_times_conf = 1.0, 4.0, flag
    _run(hip_lib.dh_softargmax2d_f32(C.byref(a), _stream()), 'dh_softargmax2d_f32')
    return {k: o.get('softargmax2d ' + k) for k, o in outs.items()}


def _sam_check(out, r, what):
    """The assertions and bars of test_gpu_ops.test_softargmax2d, on the outputs the launch produced."""
    if 'xy' in out:
        e64 = np.abs(out['xy'].astype(np.float64) - r['xy64']).max()
        print('%s: xy vs fp64 %.3e' % (what, e64))
        assert e64 <= BAR / 2, (what, e64)
        assert np.abs(out['xy'] - r['xy']).max() <= BAR, what
    if 'prob' in out:
        _close(out['prob'], r['prob'], atol=1e-9, rtol=1e-5, what=what + ' prob')
    if 'conf_raw' in out:
        _close(out['conf_raw'], r['conf_raw'], atol=1e-5, what=what + ' conf_raw')
    if 'conf_prob' in out:
        _close(out['conf_prob'], r['conf_prob'], atol=1e-9, rtol=1e-5, what=what + ' conf_prob')
    if 'gmax' in out:
        assert SV.same_bits(out['gmax'], r['gmax']), what + ' gmax'


@pytest.mark.parametrize('shape', [s for s in SV.SAM_VARIANT_SHAPES if s != (3, 16, 16, 17)])
def test_softargmax2d_every_instantiation(shape, hip_lib, cuda):
    """<16, true> (also with a second channel group of one live channel), <16, false> and <4, false>: the shapes of
    slabview.SAM_VARIANT_SHAPES (tests/test_slab_ops_host.py holds them to the library's answer)."""
    assert SV.sam_variant(hip_lib, *shape) == SV.SAM_VARIANT_SHAPES[shape]
    r = _sam_case(shape)
    out = _sam_launch(hip_lib, cuda, r['h'], shape[3], 0)
    _sam_check(out, r, 'softargmax2d %s' % (shape,))


SAM_VIEW = (3, 16, 16, 17)
SAM_VIEWS = {'dense': (17, 0), 'r4b': (34, 17), 'aligned': (36, 0)}     # (ldh, channel offset)


def test_softargmax2d_on_views(hip_lib, cuda):
    """<4, true> on the R4b layout -- 17 maps at channel 17 of a 34-channel slab: unaligned, the scalar staging with its
    clamped tail -- and at channel 0 of a 36-channel slab (float4 staging, scalar for the ragged last group); xy into
    [F, J, 3], the confidences into the second column of [F, J, 2], the probability maps into a 36-channel slab.  Per
    channel the variants do the same arithmetic: identical bits."""
    r = _sam_case(SAM_VIEW)
    got = {}
    for name, (ld, off) in SAM_VIEWS.items():
        got[name] = _sam_launch(hip_lib, cuda, r['h'], ld, off, ldxy=3, ldcr=2, ldcp=2, ldp=36, offp=2)
        _sam_check(got[name], r, 'softargmax2d view ' + name)
    for k in SAM_OUTPUTS:
        _all_same_bits({n: g[k] for n, g in got.items()}, 'softargmax2d ' + k)
    only = _sam_launch(hip_lib, cuda, r['h'], 34, 17, want=('xy',), ldxy=3)       # every other output NULL
    _sam_check(only, r, 'softargmax2d xy only')
    assert SV.same_bits(only['xy'], got['r4b']['xy'])


def test_softargmax2d_xy_times_conf(hip_lib, cuda):
    """dh_sam_args.xy_times_conf (multiply([p, c]) of spnet.py:108 folded into the read-out), with conf_prob requested and
    with conf_prob = NULL: against fp64 xy * conf_prob, and bit for bit the fp32 product of the xy and conf_prob the same
    launch returns with the flag off (the same two fp32 factors, one multiplication)."""
    r = _sam_case(SAM_VIEW)
    ref64 = r['xy64'] * r['conf_prob64']
    e = np.abs((r['xy'] * r['conf_prob']).astype(np.float64) - ref64).max()
    print('xy * conf_prob: fp32 CPU oracle vs fp64 %.3e' % e)
    off = _sam_launch(hip_lib, cuda, r['h'], 34, 17, want=('xy', 'conf_prob'), ldxy=3, ldcp=2)
    want = off['xy'] * off['conf_prob']                      # float32 x float32 -> float32: one rounding
    assert want.dtype == np.float32
    for outputs in (('xy', 'conf_prob'), ('xy',)):
        on = _sam_launch(hip_lib, cuda, r['h'], 34, 17, want=outputs, ldxy=3, ldcp=2, flag=1)
        e = np.abs(on['xy'].astype(np.float64) - ref64).max()
        print('xy_times_conf %s: vs fp64 %.3e' % (outputs, e))
        assert e <= BAR, (outputs, e)
        assert SV.same_bits(on['xy'], want), outputs
        if 'conf_prob' in on:
            assert SV.same_bits(on['conf_prob'], off['conf_prob'])


def test_softargmax2d_context_on_a_view(hip_lib, cuda):
    """dh_softargmax2d_context_f32 needs 16-byte aligned quads, so its view is the aligned one: 8 joints + 16 context maps
    at channel 4 of a 32-channel slab, the pose into [F, J, 3], the confidences into the second column of [F, J, 2]."""
    f, hh, ww, j, nctx = 2, 16, 16, 8, 2
    ch = j * (1 + nctx)
    h = _rand(np.random.default_rng(77), (f, hh, ww, ch), 4.0) + 1.0      # (positive offset: context confidences away from 0)
    t = torch.from_numpy(h).double()
    hs, hc = t[..., :j], t[..., j:]
    pc = O.joints_probability(hc)
    assert float(pc.reshape(f, j, nctx).sum(-1).min()) > 1.0
    ref = O.context_aggregation(O.softargmax2d(hs), O.softargmax2d(hc), pc, j, nctx, 0.8).numpy()
    gx, gy = _dev(np.linspace(0.0, 1.0, num=ww).astype(np.float32), cuda), _dev(np.linspace(0.0, 1.0, num=hh).astype(np.float32), cuda)
    got = {}
    for name, (ld, off) in (('dense', (ch, 0)), ('aligned', (32, 4))):
        x, y, conf = _In(h, ld, off), _Out((f, j, 2), 3, 0), _Out((f, j, 1), 2, 1)
        a = _lib().SamArgs()
        a.h, a.gx, a.gy, a.conf_raw = x.ptr, gx.data_ptr(), gy.data_ptr(), conf.ptr
        a.F, a.H, a.W, a.C, a.ldh, a.ldcr = f, hh, ww, ch, ld, 2
        a.alpha, a.conf_scale = 1.0, 1.0
        _run(hip_lib.dh_softargmax2d_context_f32(C.byref(a), j, nctx, 0.8, y.ptr, 3, _stream()), 'dh_softargmax2d_context_f32')
        got[name] = (y.get('context pose'), conf.get('context conf'))
        assert np.abs(got[name][0].astype(np.float64) - ref).max() <= BAR, name
        _close(got[name][1], O.joints_probability(hs).numpy(), atol=1e-5, what='joint confidence ' + name)
    for i in range(2):
        assert SV.same_bits(got['dense'][i], got['aligned'][i])


# ------------------------------------------------------------------------------------------------------------------------
# 6. dh_pool2d_f32      7. dh_upsample2x_add_f32
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,pool,mode', [((2, 16, 17, 20), 2, 0), ((2, 16, 17, 20), 2, 1), ((1, 9, 7, 20), 3, 0)])
def test_pool2d_on_views(shape, pool, mode, hip_lib, cuda):
    """MaxPooling2D / layers.max_min_pooling with stride 2, 'same', reading and writing channel slabs (the max + min of a
    concatenation, action.py:61, reads one): bit-exact against the oracle, identical in the three layouts."""
    v = _rand(np.random.default_rng(sum(shape) + pool + mode), shape)
    t = torch.from_numpy(v)
    ref = (O.max_min_pooling(t, (pool, pool), 'same') if mode else O.maxpool2d(t, (pool, pool), (2, 2), 'same')).numpy()
    n, h, w, ch = shape
    (pt, _, oh), (pl, _, ow) = O.same_pad(h, pool, 2), O.same_pad(w, pool, 2)
    assert ref.shape == (n, oh, ow, ch)
    for name in SV.LAYOUTS:
        x, y = _in(v, name, 0), _out((n, oh, ow, ch), name, 1)
        a = _lib().PoolArgs()
        a.x, a.y = x.ptr, y.ptr
        a.N, a.H, a.W, a.C, a.ldx, a.OH, a.OW, a.ldy = n, h, w, ch, x.ld, oh, ow, y.ld
        a.KH, a.KW, a.SH, a.SW, a.PT, a.PL, a.mode = pool, pool, 2, 2, pt, pl, mode
        _run(hip_lib.dh_pool2d_f32(C.byref(a), _stream()), 'dh_pool2d_f32')
        assert SV.same_bits(y.get('pool %s' % name), ref), name


@pytest.mark.parametrize('with_a', [True, False])
def test_upsample2x_add_on_views(with_a, hip_lib, cuda):
    """UpSampling2D((2, 2)) [+ add] of [2, 8, 6, 20] to 16 x 12 with a, b and y at three different pitches: bit-exact."""
    rng = np.random.default_rng(8 + with_a)
    va, vb = _rand(rng, (2, 16, 12, 20)), _rand(rng, (2, 8, 6, 20))
    ref = O.upsample2d(torch.from_numpy(vb))
    ref = (torch.from_numpy(va) + ref if with_a else ref).numpy()
    for name in SV.LAYOUTS:
        xa, xb, y = _in(va, name, 0), _in(vb, name, 1), _out((2, 16, 12, 20), name, 2)
        _run(hip_lib.dh_upsample2x_add_f32(xa.ptr if with_a else None, xa.ld, xb.ptr, xb.ld, y.ptr, y.ld, 2, 16, 12, 20,
                                           _stream()), 'dh_upsample2x_add_f32')
        assert SV.same_bits(y.get('upsample %s' % name), ref), name


# ------------------------------------------------------------------------------------------------------------------------
# 8. dh_depth_means_f32      9. dh_softargmax1d_f32
# ------------------------------------------------------------------------------------------------------------------------
def test_depth_means_on_views(hip_lib, cuda):
    """reception.py:193-222 on 96 frames of 7 x 9 x (4 x 5) maps: the one-pass kernel with a ragged last 64-pixel chunk, on
    dense maps and in a slab of pitch 24; at an odd channel offset the launcher falls back to the two-kernel path.  The
    file's header comment states ONE summation order for all of them: all three return the same bits, inside the bounds
    of test_gpu_ops.test_depth_means_paths_share_one_summation_order."""
    f, hw, dd, j = 96, 7 * 9, 4, 5
    h = _rand(np.random.default_rng(120 + dd + j), (f, hw, dd * j), 30.0) + 100.0
    h5 = h.astype(np.float64).reshape(f, hw, dd, j)
    got = {}
    for name, (ld, off) in (('dense', (20, 0)), ('aligned', (24, 4)), ('odd', (24, 3))):
        x, hxy, hz = _In(h, ld, off), _flat_out((f, hw, j), 0), _flat_out((f, dd, j), 1)
        _run(hip_lib.dh_depth_means_f32(x.ptr, ld, hxy.ptr, hz.ptr, f, hw, dd, j, _stream()), 'dh_depth_means_f32')
        got[name] = (hxy.get('hxy %s' % name), hz.get('hz %s' % name))
        exy = np.abs(got[name][0].astype(np.float64) - h5.mean(axis=2)).max()
        ez = np.abs(got[name][1].astype(np.float64) - h5.mean(axis=1)).max()
        print('depth_means %s: hxy %.3e hz %.3e' % (name, exy, ez))
        assert exy <= 4 * 130 * 2.0 ** -24 and ez <= 3 * 130 * 2.0 ** -24, (name, exy, ez)
    for i, what in enumerate(('hxy', 'hz')):
        _all_same_bits({n: g[i] for n, g in got.items()}, 'depth_means ' + what)


def test_softargmax1d_into_a_pose_column(hip_lib, cuda):
    """blocks.build_softargmax_1d on 16 x 17 = 272 rows (two work-groups, the second partial): z into the third column of an
    [F, J, 3] pose buffer, vz the fp32 maximum bit for bit; z = NULL and vz = NULL each once."""
    from deephar_amd.engine.executor import grid_depth
    f, dd, j = 16, 16, 17
    hz = _rand(np.random.default_rng(9), (f, dd, j), 3.0)
    ref = O.softargmax1d(torch.from_numpy(hz).double()).numpy()
    x, grid = _flat_in(hz, 1), _dev(grid_depth(dd), cuda)
    for want_z, want_vz in ((True, True), (False, True), (True, False)):
        z, vz = _Out((f, j, 1), 3, 2), _flat_out((f, j), 3)
        _run(hip_lib.dh_softargmax1d_f32(x.ptr, grid.data_ptr(), z.ptr if want_z else None, 3, vz.ptr if want_vz else None,
                                         f, dd, j, _stream()), 'dh_softargmax1d_f32')
        gz, gv = z.get('z'), vz.get('vz')
        if want_z:
            assert np.abs(gz.astype(np.float64) - ref).max() <= BAR
        else:
            assert np.all(gz == SV.CANARY)
        if want_vz:
            assert SV.same_bits(gv, hz.max(axis=1))
        else:
            assert np.all(gv == SV.CANARY)


# ------------------------------------------------------------------------------------------------------------------------
# 10. dh_global_maxmin_softmax_f32      11. dh_kronecker_f32      12. dh_context_aggregation_f32
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,p,ch,ld,off', [(3, 80, 300, 307, 5), (2, 1, 1, 3, 1), (2, 5, 60, 67, 3), (2, 5, 60, 60, 0)])
def test_global_maxmin_softmax_pitched(b, p, ch, ld, off, hip_lib, cuda):
    """layers.global_max_min_pooling (+ soft-max) reading a slab: max + min bit-exact, the soft-max at the tolerances of
    test_gpu_ops.test_kronecker_and_action_top against fp64."""
    v = _rand(np.random.default_rng(b + p + ch), (b, p, ch), 2.0)
    s32 = v.max(axis=1) + v.min(axis=1)
    s = v.astype(np.float64).max(axis=1) + v.astype(np.float64).min(axis=1)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    ref = e / e.sum(axis=1, keepdims=True)
    x = _In(v, ld, off)
    for softmax in (0, 1):
        y = _flat_out((b, ch), 1)
        _run(hip_lib.dh_global_maxmin_softmax_f32(x.ptr, ld, y.ptr, b, p, ch, softmax, _stream()), 'dh_global_maxmin_softmax_f32')
        got = y.get('global_maxmin')
        if softmax:
            _close(got, ref, atol=1e-8, rtol=1e-5, what='action_top %s' % ((b, p, ch),))
        else:
            assert SV.same_bits(got, s32)
    y = _flat_out((b, ch), 1)
    assert hip_lib.dh_global_maxmin_softmax_f32(x.ptr, ld, y.ptr, b, p, 8193, 1, _stream()) == DH_EINVAL
    torch.cuda.synchronize()
    y.get('global_maxmin refusal')


@pytest.mark.parametrize('offx', [4, 3])
def test_kronecker_pitched_inputs(offx, hip_lib, cuda):
    """layers.kronecker_prod of [2, 8, 8, 17] heat-maps at channel 17 of a 34-channel slab with 60 features at pitch 64, the
    rows written at pitch 63; features at an odd offset take the one-channel-per-thread kernel."""
    b, p, j, ch = 2, 64, 17, 60
    rng = np.random.default_rng(17 + offx)
    hm = rng.random((b, p, j)).astype(np.float32)
    hm /= hm.sum(axis=1, keepdims=True)
    v = _rand(rng, (b, p, ch))
    ref = np.einsum('bpj,bpc->bjc', hm.astype(np.float64), v.astype(np.float64))
    xh, xv, y = _In(hm, 34, 17), _In(v, 64, offx), _Out((b, j, ch), 63, 3)
    _run(hip_lib.dh_kronecker_f32(xh.ptr, 34, xv.ptr, 64, y.ptr, 63, b, p, j, ch, _stream()), 'dh_kronecker_f32')
    _close(y.get('kronecker'), ref, atol=2e-6, rtol=1e-5, what='kron offx %d' % offx)


def test_context_aggregation_into_a_pose_buffer(hip_lib, cuda):
    """blocks.build_context_aggregation with ldy = 3: the pose lands in the first two columns of [F, J, 3]."""
    rng = np.random.default_rng(11)
    ys, yc = rng.random((5, 16, 2)).astype(np.float32), rng.random((5, 32, 2)).astype(np.float32)
    pc = rng.uniform(0.5, 3.0, (5, 32, 1)).astype(np.float32)
    d = lambda a: torch.from_numpy(a).double()
    ref = O.context_aggregation(d(ys), d(yc), d(pc), 16, 2, 0.8).numpy()
    xs, xc, xp, y = _flat_in(ys, 1), _flat_in(yc, 3), _flat_in(pc, 1), _Out((5, 16, 2), 3, 0)
    _run(hip_lib.dh_context_aggregation_f32(xs.ptr, xc.ptr, xp.ptr, y.ptr, 5, 16, 2, 0.8, 3, _stream()),
         'dh_context_aggregation_f32')
    _close(y.get('context aggregation'), ref, atol=2e-7, rtol=1e-6, what='agg')


# ------------------------------------------------------------------------------------------------------------------------
# 13. dh_normalize_u8_f32
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('npix,ch', [(1000, 5), (300, 1)])
def test_normalize_u8(npix, ch, hip_lib, cuda):
    """The stand-alone normalisation, a table gather: bit-exact.  With 5 channels the fifth reads its table from global
    memory, not LDS; frames and result at bases that are not 16-byte aligned."""
    rng = np.random.default_rng(npix + ch)
    frames = rng.integers(0, 256, (npix, ch), dtype=np.uint8)
    frames[0], frames[-1] = 0, 255
    lut = _rand(rng, (ch, 256))
    buf = torch.zeros(npix * ch + 8, dtype=torch.uint8, device=cuda)
    buf[3:3 + npix * ch] = torch.from_numpy(frames.reshape(-1)).to(cuda)
    y, lut_d = _flat_out((npix, ch), 1), _dev(lut, cuda)
    _run(hip_lib.dh_normalize_u8_f32(buf.data_ptr() + 3, lut_d.data_ptr(), y.ptr, npix, ch, _stream()), 'dh_normalize_u8_f32')
    assert SV.same_bits(y.get('normalize_u8'), lut[np.arange(ch)[None, :], frames])
