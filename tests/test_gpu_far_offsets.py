"""Every kernel at its 2^31- and 2^32-byte addressing limits (tests/farview.py holds the audit and the device-side views;
tests/test_far_offsets_host.py sweeps the same rules on fake pointers).

The kernels mix 32-bit forms (buffer descriptors with unsigned byte offsets, signed voffset + soffset in the direct epilogue,
the first-layer kernel and the LDS depthwise kernel, int element offsets in the skinny kernel) with 64-bit ones, and host
rules pick the form at hard thresholds.  Here each threshold gets a launch one step below it and one at or above it on REAL
memory: a map of ~2048 pixels whose pitch puts the last pixel where a batch of thousands would.  For every launch

  * the library says beforehand which form it takes (dh_conv2d_route / convview.paths, dh_dwconv2d_uses_lds_kernel), and
    that is the form the case is there for;
  * the result has the bits of the COMPACT launch of the same tiling, which is held once to the fp64 statement by the
    family's existing bar (fp32: e_hip <= 4 e_cpu + 1e-6, three-part split: e_split <= 2 e_f32 + 1e-6); where the two sides
    of a threshold are different kernels with different last bits (first-layer kernel / register-gather kernel) each side is
    held to fp64 by the bar;
  * every float of the output buffer outside the view still holds its canary, guard runs included; a refused launch has
    written nothing.

All buffers are allocated and filled on the device; references are computed on the compact data only.  No test holds more than
9 GiB; farview.need is the only skip.

Which rules depend on N.  The `0xf0000000` rules (x descriptors: N*H*W*ldx*4) and the `0x7fffffff` rules of the direct epilogue
and of the first-layer kernel (N*OH*OW*ld*4) bound the WHOLE tensor: a layer moves to the other form as the batch grows.  The
skinny rule (H*W*ldx floats) and the LDS depthwise rule (H*W*ld*4) bound one FRAME; the frame base is 64-bit.

A note on 262148: N*H*W*ldx*4 is the first span past 2^31 there, but the descriptor's num_records = ((P-1)*ldx + Cin)*4 gets
bit 31 only from ldx = 262276 on (P = 2048), so both pitches run.
"""
import ctypes as C
import functools
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convview as CV                              # noqa: E402
import farview as FV                               # noqa: E402
import resample_ref as R                           # noqa: E402
import slabview as SV                              # noqa: E402
import test_gpu_conv_views as TCV                  # noqa: E402  (the fp64 / fp32 statement of a convolution case)
import test_gpu_slab_ops as TSO                    # noqa: E402  (references and bars of the non-conv kernels)
from oracle import ops as O                        # noqa: E402

pytestmark = pytest.mark.gpu

NAN = np.nan
FAR32 = 524292                    # 2048 pixels * 524292 floats * 4 B = 2^32 + 32 KiB
_rand, _stream, _same = TCV._rand, TCV._stream, TCV._same


def _far_ld(pixels, limit=1 << 32):
    """The first pitch (a multiple of 4 floats) at which `pixels` pixels span more than `limit` bytes."""
    return (limit // (4 * pixels) // 4 + 1) * 4


@functools.lru_cache(maxsize=None)
def _data(name):
    """Seeded operands of a farview case (shared by every launch of it, never modified)."""
    case = FV.CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    d = {}
    if case.x_u8:
        from deephar_amd.engine.executor import normalization_lut
        d['x_u8'] = rng.integers(0, 256, case.shape_of('x'), dtype=np.uint8)
        d['lut'] = normalization_lut(3, 1)
        d['x'] = d['lut'][np.arange(3)[None, None, None, :], d['x_u8']].astype(np.float32)
    else:
        d['x'] = _rand(rng, case.shape_of('x'))
    d['w'] = _rand(rng, (case.k, case.k, case.Cin, case.Cout), np.sqrt(1.0 / case.K))
    if case.pre_bn:
        d['pre_scale'], d['pre_shift'] = rng.uniform(0.5, 1.5, case.Cin).astype(np.float32), _rand(rng, (case.Cin,), 0.3)
    if case.bn:
        d['post_scale'], d['post_shift'] = rng.uniform(0.5, 1.5, case.Cout).astype(np.float32), _rand(rng, (case.Cout,), 0.3)
    for o in ('res1', 'res2'):
        if o in case.operands():
            d[o] = _rand(rng, case.shape_of(o))
    return d


@functools.lru_cache(maxsize=None)
def _truth(name):
    """(fp64 statement, max error of the fp32 CPU oracle against it) -- computed once per layer."""
    case, d = FV.CASES[name], _data(name)
    ref = TCV._statement(case, d, torch.float64)
    return ref, float(np.abs(TCV._statement(case, d, torch.float32) - ref).max())


def _fp32_bar(name, y, what):
    ref, e_cpu = _truth(name)
    e_hip = float(np.abs(y.astype(np.float64) - ref).max())
    print('%s: |hip - fp64| = %.3e   |fp32 cpu - fp64| = %.3e' % (what, e_hip, e_cpu))
    assert e_hip <= 4 * e_cpu + 1e-6, (what, e_hip, e_cpu)


def _compact(hip_lib, name, cfg, lay='aligned'):
    """The compact launch of a case at `cfg`, held to the fp64 statement by the family's bar -> (route, y)."""
    case, d = FV.CASES[name], _data(name)
    w = FV.pack(case, d['w'])
    rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, cfg, lay=lay, what=name + ' compact')
    assert rc == 0, (name, cfg, rc)
    if case.w_split in (0, 2):
        _fp32_bar(name, y, name + ' compact')
    elif case.w_split in (1, 5):                  # three parts: within twice the shipped fp32 kernel's own error
        twin = CV.Case(name + '_f32', (case.N, case.H, case.W, case.Cin), case.Cout, k=case.k, stride=case.stride, pre=case.pre,
                       bn=case.bn, relu=case.relu, res1=case.res1)
        rc, _, _, f32 = FV.conv_launch(hip_lib, twin, d, FV.pack(twin, d['w']), -1, what=name + ' fp32 twin')
        assert rc == 0
        ref, _ = _truth(name)
        e_split, e_f32 = float(np.abs(y.astype(np.float64) - ref).max()), float(np.abs(f32.astype(np.float64) - ref).max())
        print('%s: |split - fp64| = %.3e   |fp32 mfma - fp64| = %.3e' % (name, e_split, e_f32))
        assert e_split <= 2 * e_f32 + 1e-6, (name, e_split, e_f32)
    return r, w, y


def _bytes(case, far):
    return sum(FV.slab_bytes(case.shape_of(o), ld) for o, ld in far.items())


# ------------------------------------------------------------------------------------------------------------------------
# 3. convolutions
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['direct', 'direct_down', 'halo'])
def test_direct_epilogue_at_the_31_bit_bound(name, hip_lib, cuda):
    """M * ld * 4 < 0x7fffffff for y and res1 ((M / 4) * ldr2 * 4 for the half-resolution res2): 262140 floats at M = 2048
    is 2^31 - 32768 bytes and must report and take the direct epilogue (signed voffset + soffset up to 2^31 - 32768 + 4 Cout),
    262144 must report the staged one (size_t).  Each operand alone, then y and res1 together."""
    case, d = FV.CASES[name], _data(name)
    cfg = case.cfgs[0]
    r0, w, want = _compact(hip_lib, name, cfg)
    assert r0.tm == 1 and r0.epi & 2
    runs = []
    for o in ('y', 'res1') + (('res2',) if case.res2 else ()):
        mul = 4 if o == 'res2' else 1
        runs += [({o: 262140 * mul}, True), ({o: 262144 * mul}, False)]
    runs.append((dict(y=262140, res1=262140), True))
    for far, direct in runs:
        what = '%s %s' % (name, far)
        FV.need(_bytes(case, far))
        rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, cfg, far=far, what=what)
        assert rc == 0 and r.kernel == r0.kernel and r.tile_cfg == r0.tile_cfg, (what, rc, r.kernel)
        p = CV.paths(hip_lib, case, a, cfg)
        assert bool(r.epi & 2) == direct and ('direct' in p) == direct, (what, r.epi, p)
        assert 'staged_vec' in p or name == 'direct_down', (what, p)           # (the ragged column tiles of Cout = 96 / 72)
        if case.res2:
            assert ('down_direct' in p) == direct and ('down_staged_pow2' in p) == (not direct), (what, p)
        _same(y, want, what)
        del y, a
        FV.release()


X_CASES = ['pw_ktail', 'pw_bn', 'kxk', 'split1', 'split3', 'split4', 'ext_pw', 'ext_kxk', 'halo']


@pytest.mark.parametrize('name', X_CASES)
def test_x_descriptor_at_the_buffer_bound(name, hip_lib, cuda):
    """N*H*W*ldx*4 <= 0xf0000000 for every kernel that reads x through a buffer descriptor.  262148: the first span past 2^31;
    262276: (int)num_records negative; 491520: exactly 0xf0000000, voffset + soffset within 4 Kp of it; 491524: refused
    (DH_EUNSUPPORTED, nothing written), or with tile_cfg = -1 on an fp32 layer the register-gather kernel, with that
    kernel's bits."""
    case, d = FV.CASES[name], _data(name)
    cfg = case.cfgs[0]
    r0, w, want = _compact(hip_lib, name, cfg)
    assert r0.kernel in FV.THIRTYTWO_BIT
    for ld in (262148, 262276, 491520):
        what = '%s ldx %d' % (name, ld)
        FV.need(_bytes(case, dict(x=ld)))
        rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, cfg, far=dict(x=ld), what=what)
        assert rc == 0 and r.kernel == r0.kernel and r.tile_cfg == r0.tile_cfg, (what, rc, r.kernel)
        for nm, value, bound, inclusive in FV.largest_offsets(a, r):
            assert value <= bound if inclusive else value < bound, (what, nm)
        _same(y, want, what)
        del y, a
        FV.release()
    FV.need(_bytes(case, dict(x=491524)))
    rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, cfg, far=dict(x=491524), what=name + ' ldx 491524')
    assert rc == CV.DH_EUNSUPPORTED and y is None, (name, rc)                  # (conv_launch: every canary of y intact)
    if case.w_split == 0:
        rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, -1, far=dict(x=491524), what=name + ' ldx 491524 tile_cfg -1')
        assert rc == 0 and r.kernel == FV.CV_KERNEL['general'], (name, rc, r.kernel)
        rc, rg, _, yg = FV.conv_launch(hip_lib, case, d, w, r.tile_cfg, what=name + ' general compact')
        assert rc == 0 and rg.kernel == FV.CV_KERNEL['general']
        _same(y, yg, name + ' ldx 491524: the general kernel')
        _fp32_bar(name, yg, name + ' general compact')
    del y, a
    FV.release()


@pytest.mark.parametrize('cout', CV.CONVT_COUTS)
@pytest.mark.parametrize('parts', [0, 3])
def test_transposed_conv_x_at_the_buffer_bound(cout, parts, hip_lib, cuda):
    """dh_conv2d_transpose2x2_f32 / _split_f32 at convview.CONVT_SHAPE (M = 60 input pixels), x pitches scaled to M: the first span
    past 2^31, the first negative num_records, exactly 0xf0000000, and one step above (DH_EUNSUPPORTED, nothing written)."""
    from deephar_amd import _lib, functional as F
    n, h, w, cin = CV.CONVT_SHAPE
    M = n * h * w
    rng = np.random.default_rng(cout + parts)
    x, k = _rand(rng, (n, h, w, cin)), _rand(rng, (2, 2, cout, cin), np.sqrt(1.0 / cin))
    ps, pb = rng.uniform(0.5, 1.5, cin).astype(np.float32), _rand(rng, (cin,), 0.3)
    res = _rand(rng, (n, 2 * h, 2 * w, cout))
    wt, kp, np_ = F.pack_convt_weight(k, 'cuda', parts=parts or None)
    t = lambda a_, dt: torch.from_numpy(a_).to(dt)
    st = lambda dt: R.conv_transpose2x2(t(x, dt), t(k, dt), t(ps, dt), t(pb, dt), True, t(res, dt), True).double().numpy()
    ref = st(torch.float64)
    e_cpu = float(np.abs(st(torch.float32) - ref).max())
    keep = [CV.table(ps, False), CV.table(pb, False)]

    def run(ldx, split, weight=None):
        Lx, Ly, Lr = SV.layout(cin, 'aligned', 0), SV.layout(cout, 'aligned', 1), SV.layout(cout, 'aligned', 2)
        if ldx:
            FV.need(FV.slab_bytes(x.shape, ldx))
            tx, px = FV.far_slab(x, ldx, Lx[1], CV.LOUD)
        else:
            tx, px = SV.slab(x, Lx[0], Lx[1], CV.LOUD)
        tr, pr = SV.slab(res, Lr[0], Lr[1], NAN)
        ty, py = SV.out_slab((n, 2 * h, 2 * w, cout), Ly[0], Ly[1])
        a = _lib.ConvtArgs()
        a.x, a.w, a.y, a.pre_scale, a.pre_shift, a.res = px, (wt if weight is None else weight).data_ptr(), py, keep[0][1], keep[1][1], pr
        a.N, a.H, a.W, a.Cin, a.ldx, a.Cout, a.ldy, a.ldr = n, h, w, cin, ldx or Lx[0], cout, Ly[0], Lr[0]
        a.Kp, a.Np, a.pre_relu, a.post_relu = kp, np_, 1, 1
        ok = M * a.ldx * 4 <= FV.MAX_BUFFER_BYTES
        if split:
            assert hip_lib.dh_conv2d_transpose2x2_split_eligible(C.byref(a)) == int(ok)
            rc = hip_lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), parts, -1, _stream())
        else:
            rc = hip_lib.dh_conv2d_transpose2x2_f32(C.byref(a), -1, _stream())
        torch.cuda.synchronize()
        assert rc == (0 if ok else CV.DH_EUNSUPPORTED), (ldx, rc)
        SV.assert_untouched(ty, Ly[1] if ok else 0, cout if ok else 0, what='convT ldx %d' % ldx)
        return SV.view(ty, Ly[1], cout) if ok else None

    want = run(0, bool(parts))
    e_hip = float(np.abs(want - ref).max())
    if parts:
        f32 = run(0, False, weight=F.pack_convt_weight(k, 'cuda')[0])
        e_f32 = float(np.abs(f32 - ref).max())
        assert e_hip <= 2 * e_f32 + 1e-6, (e_hip, e_f32)
    else:
        assert e_hip <= 4 * e_cpu + 1e-6, (e_hip, e_cpu)
    past31, negative, exact = _far_ld(M, 1 << 31), _far_ld(M - 1, 1 << 31), FV.MAX_BUFFER_BYTES // (4 * M)
    assert (past31, negative, exact) == (8947852, 9099508, 16777216) and exact * M * 4 == FV.MAX_BUFFER_BYTES
    for ldx in (past31, negative, exact):
        assert ((M - 1) * ldx + kp) * 4 < FV.OOB
        _same(run(ldx, bool(parts)), want, 'convT -> %d parts %d ldx %d' % (cout, parts, ldx))
        FV.release()
    assert run(exact + 4, bool(parts)) is None
    FV.release()


@pytest.mark.parametrize('name', ['general_1x1', 'general_3x3'])
def test_general_kernel_and_staged_epilogue_past_4_gib(name, hip_lib, cuda):
    """The register-gather kernel and the staged epilogue hold size_t addresses: x, y and res1 each on a span just past 2^32
    bytes (2048 pixels at 524292 floats)."""
    case, d = FV.CASES[name], _data(name)
    cfg = case.cfgs[0]
    r0, w, want = _compact(hip_lib, name, cfg)
    assert r0.kernel == FV.CV_KERNEL['general'] and r0.vec4 == 1
    for o in ('x', 'y', 'res1'):
        what = '%s far %s' % (name, o)
        assert case.M * FAR32 * 4 > 1 << 32
        FV.need(_bytes(case, {o: FAR32}))
        rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, cfg, far={o: FAR32}, what=what)
        assert rc == 0 and r.kernel == r0.kernel and r.vec4 == 1, (what, rc)
        p = CV.paths(hip_lib, case, a, cfg)
        assert 'direct' not in p and 'staged_vec' in p, (what, p)
        _same(y, want, what)
        del y, a
        FV.release()


@pytest.mark.parametrize('name', ['stem', 'stem_u8'])
def test_first_layer_kernel_at_the_31_bit_bound(name, hip_lib, cuda):
    """N*OH*OW*ldy*4 < 0x7fffffff (a rule on the whole tensor: it depends on N).  Frames of [2, 4, 256, 3]: M = 512;
    ldy = 1048572 must be the first-layer kernel (the compact launch's bits), 1048576 what the route says instead -- the
    register-gather kernel, which pairs the k values differently: each side is held to fp64 by the bar."""
    case, d = FV.CASES[name], _data(name)
    lay = dict(x='dense', y='aligned')
    r0, w, want = _compact(hip_lib, name, -1, lay=lay)
    assert r0.kernel == FV.CV_KERNEL['stem']
    for ld, stem in ((1048572, True), (1048576, False)):
        what = '%s ldy %d' % (name, ld)
        FV.need(_bytes(case, dict(y=ld)))
        rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, -1, far=dict(y=ld), lay=lay, what=what)
        assert rc == 0 and r.kernel == (FV.CV_KERNEL['stem'] if stem else FV.CV_KERNEL['general']), (what, rc, r.kernel)
        assert hip_lib.dh_conv2d_uses_first_layer_kernel(C.byref(a)) == int(stem)
        if stem:
            _same(y, want, what)
        _fp32_bar(name, y, what)
        del y, a
        FV.release()


@pytest.mark.parametrize('name', ['skinny', 'skinny_rs2'])
def test_skinny_kernel_at_the_31_bit_element_bound(name, hip_lib, cuda):
    """H*W*ldx <= 0x7fffffff floats per frame (int element offsets): 8 x 8 x 64 -> 24 at ldx = 33554428 is 2^31 - 256 floats, an
    8 GiB view; with x_resample = 2 the frame read is 16 x 16 and the bound is on four times the map: ldx = 8388604.  (The pitch
    one step above is refused before any allocation: tests/test_far_offsets_host.py.)"""
    case, d = FV.CASES[name], _data(name)
    r0, w, want = _compact(hip_lib, name, -1)
    assert r0.kernel == FV.CV_KERNEL['skinny'] and r0.vec4 == 1
    frame = case.H * case.W * (4 if case.x_resample >= 2 else 1)
    ld = [l for l, ok in FV.steps_around(FV.INT31, frame, True) if ok][-1]
    assert ld == (33554428 if name == 'skinny' else 8388604) and frame * ld == (1 << 31) - 4 * frame
    FV.need(_bytes(case, dict(x=ld)))
    rc, r, a, y = FV.conv_launch(hip_lib, case, d, w, -1, far=dict(x=ld), what='%s ldx %d' % (name, ld))
    assert rc == 0 and r.kernel == FV.CV_KERNEL['skinny'] and r.vec4 == 1, (name, rc)
    _same(y, want, name)
    del y, a
    FV.release()


# ------------------------------------------------------------------------------------------------------------------------
# 4. the other kernels
# ------------------------------------------------------------------------------------------------------------------------
class _FarIn:
    def __init__(self, values, ld, off=4, fill=NAN):
        FV.need(FV.slab_bytes(np.shape(values), ld))
        self.t, self.ptr = FV.far_slab(values, ld, off, fill)
        self.ld, self.off = ld, off


class _FarOut:
    def __init__(self, shape, ld, off=4):
        FV.need(FV.slab_bytes(shape, ld))
        self.t, self.ptr = FV.far_out_slab(shape, ld, off)
        self.ld, self.off, self.C = ld, off, shape[-1]

    def get(self, what=''):
        bad = FV.far_untouched(self.t, self.off, self.C)
        assert bad == 0, '%s: %d floats written outside the view' % (what, bad)
        return FV.far_view(self.t, self.off, self.C)


def _place(values_or_shape, far, k, out=False):
    """An operand on a far view (pitch `far`) or, far = 0, on the aligned slabview layout number k."""
    if out:
        return _FarOut(values_or_shape, far) if far else TSO._out(values_or_shape, 'aligned', k)
    return _FarIn(values_or_shape, far) if far else TSO._in(values_or_shape, 'aligned', k)


def _dw_launch(hip_lib, x, dwk, ps, pb, k, ldx=0, ldy=0, want_lds=None):
    n, h, w, c = x.shape
    xi, yo = _place(x, ldx, 0), _place((n, h, w, c), ldy, 1, out=True)
    keep = [CV.table(ps, False), CV.table(pb, False)] if ps is not None else []
    dwt = torch.from_numpy(np.ascontiguousarray(dwk.reshape(k * k, c))).cuda()
    g = TCV._dw_struct(xi.ptr, xi.ld, dwt.data_ptr(), yo.ptr, yo.ld, n, h, w, c, k,
                       dict(pre_scale=keep[0][1], pre_shift=keep[1][1]) if keep else {})
    if want_lds is not None:
        assert hip_lib.dh_dwconv2d_uses_lds_kernel(C.byref(g)) == int(want_lds), (x.shape, k, ldx, ldy)
    rc = hip_lib.dh_dwconv2d_f32(C.byref(g), _stream())
    torch.cuda.synchronize()
    assert rc == 0, (x.shape, k, ldx, ldy, rc)
    return yo.get('dwconv %s k %d ldx %d ldy %d' % (x.shape, k, ldx, ldy))


def _dw_case(shape, k, affine=True):
    """affine: BN + ReLU prologue (that variant of the LDS kernel zeroes padding taps itself, after the affine); without it
    a padding tap is whatever the buffer load returns for its offset -- zero only while the offset stays out of the
    descriptor's range."""
    rng = np.random.default_rng(sum(shape) + k)
    c = shape[-1]
    x, dwk = _rand(rng, shape), _rand(rng, (k, k, c, 1), 1.0 / k)
    ps, pb = rng.uniform(0.5, 1.5, c).astype(np.float32), _rand(rng, (c,), 0.3)
    t = lambda a_: torch.from_numpy(a_).double()
    if not affine:
        return x, dwk, None, None, O.depthwise_conv2d(t(x), t(dwk)).numpy()
    ref = O.depthwise_conv2d(O.relu(t(x) * t(ps) + t(pb)), t(dwk)).numpy()
    return x, dwk, ps, pb, ref


def _dw_bar(got, ref, what):
    err = np.abs(got - ref)
    print('%s: max err %.3e' % (what, err.max()))
    assert np.all(err <= 1e-5 + 2e-5 * np.abs(ref)), (what, err.max())            # test_dwconv's bar


@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('hw', [16, 32])
@pytest.mark.parametrize('k', [5, 3])
def test_depthwise_at_the_frame_bound(hw, k, affine, hip_lib, cuda):
    """H*W*ld*4 < 0x7fffffff per frame, for x and for y: ld = 2^31 / (4 H W) - 4 is the LDS kernel (int voffset up to
    2^31 - 4 H W * 4 + 4 C, the second frame's base past 2^31 in size_t), ld = 2^31 / (4 H W) the register kernel (size_t).  Both
    sides by test_dwconv's bar, and -- one summation order in all stride-1 kernels -- the bits of the compact launch.  With the
    BN + ReLU prologue and without (then the padding taps are the zeros of out-of-range buffer loads)."""
    x, dwk, ps, pb, ref = _dw_case((2, hw, hw, 32), k, affine)
    want = _dw_launch(hip_lib, x, dwk, ps, pb, k, want_lds=True)
    _dw_bar(want, ref, 'dw %d k %d compact' % (hw, k))
    at = (1 << 31) // (4 * hw * hw)
    for ld, lds in ((at - 4, True), (at, False)):
        for far in (dict(ldx=ld), dict(ldy=ld)):
            got = _dw_launch(hip_lib, x, dwk, ps, pb, k, want_lds=lds, **far)
            _dw_bar(got, ref, 'dw %d k %d %s' % (hw, k, far))
            _same(got, want, 'dw %d k %d %s' % (hw, k, far))
            del got
            FV.release()


@pytest.mark.parametrize('affine', [False, True])
def test_depthwise_one_row_map_near_the_frame_bound(affine, hip_lib, cuda):
    """What the audit found (farview's docstring): on a one-row map the LDS kernel's window rows behind the frame would wrap
    past 2^32 into the frame at a pitch near the frame bound, and without a prologue (whose variant zeroes padding taps
    itself) a padding tap would read the slab's fill.  The rule sends the launch to the register kernel; a small pitch keeps
    the LDS kernel.  Same bits, test_dwconv's bar."""
    x, dwk, ps, pb, ref = _dw_case((2, 1, 8, 32), 5, affine)
    want = _dw_launch(hip_lib, x, dwk, ps, pb, 5, want_lds=True)
    _dw_bar(want, ref, 'dw 1 x 8 compact')
    ld = (1 << 31) // (4 * 8) - 4
    got = _dw_launch(hip_lib, x, dwk, ps, pb, 5, ldx=ld, want_lds=False)
    _dw_bar(got, ref, 'dw 1 x 8 ldx %d' % ld)
    _same(got, want, 'dw 1 x 8 ldx %d' % ld)
    del got
    FV.release()


def test_grouped_conv_dw_launch_with_a_far_depthwise_output(hip_lib, cuda):
    """dh_conv2d_dw_group_f32 (2, 16, 16, 96 -> 264 beside a 5 x 5 depthwise convolution) with the depthwise output at the LDS
    kernel's last pitch: the bits of the two single launches.  One step above the group refuses (its depthwise half is the LDS
    kernel only) and writes nothing."""
    cout = 264
    case = CV.Case('far_group', (2, 16, 16, 96), cout, pre='bnrelu', bn=True, res1=True)
    rng = np.random.default_rng(cout)
    d = dict(x=_rand(rng, (2, 16, 16, 96)), w=_rand(rng, (1, 1, 96, cout), np.sqrt(1.0 / 96)),
             pre_scale=rng.uniform(0.5, 1.5, 96).astype(np.float32), pre_shift=_rand(rng, (96,), 0.3),
             post_scale=rng.uniform(0.5, 1.5, cout).astype(np.float32), post_shift=_rand(rng, (cout,), 0.3),
             res1=_rand(rng, (2, 16, 16, cout)))
    dwt = torch.from_numpy(_rand(rng, (25, 96), 0.2)).cuda()
    wt, kp, np_ = CV.pack(case, d['w'])
    L = dict(x=SV.layout(96, 'aligned', 0), y=SV.layout(cout, 'aligned', 1), res1=SV.layout(cout, 'aligned', 2))
    tx, px = SV.slab(d['x'], L['x'][0], L['x'][1], NAN)
    tr, pr = SV.slab(d['res1'], L['res1'][0], L['res1'][1], NAN)
    keep, tab = TCV._tables(case, d)
    at = (1 << 31) // (4 * 256)
    outs = {}
    for which, ld in (('group', at - 4), ('single', at - 4), ('refused', at)):
        ty, py = SV.out_slab((2, 16, 16, cout), *L['y'])
        yd = _FarOut((2, 16, 16, 96), ld)
        a = CV.fill_args(case, dict(x=px, y=py, res1=pr), dict(x=L['x'][0], y=L['y'][0], res1=L['res1'][0]), wt.data_ptr(), tab)
        g = TCV._dw_struct(px, L['x'][0], dwt.data_ptr(), yd.ptr, ld, 2, 16, 16, 96, 5, tab)
        assert hip_lib.dh_dwconv2d_uses_lds_kernel(C.byref(g)) == int(which != 'refused')
        if which == 'single':
            assert hip_lib.dh_conv2d_f32(C.byref(a), -1, _stream()) == 0
            assert hip_lib.dh_dwconv2d_f32(C.byref(g), _stream()) == 0
        else:
            rc = hip_lib.dh_conv2d_dw_group_f32(C.byref(a), C.byref(g), _stream())
            assert rc == (CV.DH_EUNSUPPORTED if which == 'refused' else 0), (which, rc)
        torch.cuda.synchronize()
        if which == 'refused':
            SV.assert_untouched(ty, 0, 0, what='refused group: conv output')
            assert FV.far_untouched(yd.t, 0, 0) == 0
        else:
            SV.assert_untouched(ty, L['y'][1], cout, what=which)
            outs[which] = (SV.view(ty, L['y'][1], cout), yd.get(which))
        del yd, g
        FV.release()
    _same(outs['group'][0], outs['single'][0], 'far group: conv half')
    _same(outs['group'][1], outs['single'][1], 'far group: depthwise half')


@pytest.mark.parametrize('far', ['x', 'y'])
def test_depthwise_register_kernel_past_4_gib(far, hip_lib, cuda):
    """C = 20 is no multiple of 32: the float4 register kernel (size_t addresses), 2048 pixels at 524292 floats."""
    x, dwk, ps, pb, ref = _dw_case((2, 32, 32, 20), 3)
    want = _dw_launch(hip_lib, x, dwk, ps, pb, 3, want_lds=False)
    got = _dw_launch(hip_lib, x, dwk, ps, pb, 3, want_lds=False, **{'ld' + far: FAR32})
    _dw_bar(got, ref, 'dw register far ' + far)
    _same(got, want, 'dw register far ' + far)
    del got
    FV.release()


@pytest.mark.parametrize('far', ['x', 'y'])
def test_strided_depthwise_past_4_gib(far, hip_lib, cuda):
    """dh_dwconv2d_strided_f32, 5 x 5 stride 2 on [2, 32, 32, 20]: x at 524292 (2048 pixels), y at 2097156 (512 pixels)."""
    from deephar_amd import _lib
    n, h, w, c, k = 2, 32, 32, 20, 5
    rng = np.random.default_rng(5)
    x, dwk = _rand(rng, (n, h, w, c)), _rand(rng, (k, k, c, 1), 1.0 / k)
    t = lambda a_: torch.from_numpy(a_).double()
    ref = R.dwconv_strided(t(x), t(dwk), (2, 2)).numpy()
    (pt, _, oh), (pl, _, ow) = O.same_pad(h, k, 2), O.same_pad(w, k, 2)
    xi = _place(x, FAR32 if far == 'x' else 0, 0)
    yo = _place((n, oh, ow, c), _far_ld(n * oh * ow) if far == 'y' else 0, 1, out=True)
    assert (xi.t.numel() if far == 'x' else yo.t.numel()) * 4 > 1 << 32
    dwt = torch.from_numpy(np.ascontiguousarray(dwk.reshape(k * k, c))).cuda()
    a = _lib.DwsArgs()
    a.x, a.w, a.y = xi.ptr, dwt.data_ptr(), yo.ptr
    a.N, a.H, a.W, a.C, a.ldx, a.ldy, a.OH, a.OW = n, h, w, c, xi.ld, yo.ld, oh, ow
    a.KH, a.KW, a.SH, a.SW, a.PT, a.PL = k, k, 2, 2, pt, pl
    TSO._run(hip_lib.dh_dwconv2d_strided_f32(C.byref(a), _stream()), 'dh_dwconv2d_strided_f32')
    TSO._close(yo.get('strided dw far ' + far), ref, atol=1e-5, what='strided dw far ' + far)
    del xi, yo
    FV.release()


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('far', ['x', 'y'])
def test_pool2d_past_4_gib(far, mode, hip_lib, cuda):
    """MaxPooling2D / max + min pooling, 2 x 2 stride 2 on [2, 32, 32, 20]: bit-exact against the oracle."""
    from deephar_amd import _lib
    n, h, w, c = 2, 32, 32, 20
    v = _rand(np.random.default_rng(mode), (n, h, w, c))
    tt = torch.from_numpy(v)
    ref = (O.max_min_pooling(tt, (2, 2), 'same') if mode else O.maxpool2d(tt, (2, 2), (2, 2), 'same')).numpy()
    xi = _place(v, FAR32 if far == 'x' else 0, 0)
    yo = _place((n, h // 2, w // 2, c), _far_ld(n * h * w // 4) if far == 'y' else 0, 1, out=True)
    a = _lib.PoolArgs()
    a.x, a.y = xi.ptr, yo.ptr
    a.N, a.H, a.W, a.C, a.ldx, a.OH, a.OW, a.ldy = n, h, w, c, xi.ld, h // 2, w // 2, yo.ld
    a.KH, a.KW, a.SH, a.SW, a.PT, a.PL, a.mode = 2, 2, 2, 2, 0, 0, mode
    TSO._run(hip_lib.dh_pool2d_f32(C.byref(a), _stream()), 'dh_pool2d_f32')
    assert SV.same_bits(yo.get('pool far ' + far), ref)
    del xi, yo
    FV.release()


@pytest.mark.parametrize('far', ['a', 'b', 'y'])
def test_upsample2x_add_past_4_gib(far, hip_lib, cuda):
    rng = np.random.default_rng(8)
    va, vb = _rand(rng, (2, 32, 32, 20)), _rand(rng, (2, 16, 16, 20))
    ref = (torch.from_numpy(va) + O.upsample2d(torch.from_numpy(vb))).numpy()
    xa = _place(va, FAR32 if far == 'a' else 0, 0)
    xb = _place(vb, _far_ld(512) if far == 'b' else 0, 1)
    yo = _place((2, 32, 32, 20), FAR32 if far == 'y' else 0, 2, out=True)
    TSO._run(hip_lib.dh_upsample2x_add_f32(xa.ptr, xa.ld, xb.ptr, xb.ld, yo.ptr, yo.ld, 2, 32, 32, 20, _stream()), 'dh_upsample2x_add_f32')
    assert SV.same_bits(yo.get('upsample far ' + far), ref)
    del xa, xb, yo
    FV.release()


@pytest.mark.parametrize('far', ['a', 'b', 'c', 'y'])
def test_eltwise_past_4_gib(far, hip_lib, cuda):
    """affine + add3 on 2048 pixels x 17 channels: test_eltwise_on_views' bound 2^-22 * S against fp64."""
    from deephar_amd import _lib
    d = TSO._elt_data(2048, 17, 'affine_add3')
    ref, bound = TSO._elt_ref(d, 'affine_add3')
    ops = {o: _place(d[o], FAR32 if far == o else 0, i) for i, o in enumerate('abc')}
    yo = _place((2048, 17), FAR32 if far == 'y' else 0, 1, out=True)
    sc, sh = TSO._dev(d['scale'], cuda), TSO._dev(d['shift'], cuda)
    a = _lib.EltArgs()
    a.a, a.lda, a.b, a.ldb, a.c, a.ldc = ops['a'].ptr, ops['a'].ld, ops['b'].ptr, ops['b'].ld, ops['c'].ptr, ops['c'].ld
    a.y, a.ldy, a.scale, a.shift = yo.ptr, yo.ld, sc.data_ptr(), sh.data_ptr()
    a.npix, a.C, a.relu, a.op, a.bcast_b = 2048, 17, 0, 0, 0
    TSO._run(hip_lib.dh_eltwise_f32(C.byref(a), _stream()), 'dh_eltwise_f32')
    err = np.abs(yo.get('eltwise far ' + far).astype(np.float64) - ref)
    assert np.all(err <= bound), np.nanmax(err)
    del ops, yo
    FV.release()


@pytest.mark.parametrize('ch', [20, 17])
@pytest.mark.parametrize('far', ['x', 'y'])
def test_copy_channels_past_4_gib(far, ch, hip_lib, cuda):
    """The float4 kernel (20 channels) and the scalar one (17): bit-exact."""
    v = _rand(np.random.default_rng(ch), (2048, ch))
    xi = _place(v, FAR32 if far == 'x' else 0, 0)
    yo = _place((2048, ch), FAR32 if far == 'y' else 0, 1, out=True)
    TSO._run(hip_lib.dh_copy_channels_f32(xi.ptr, xi.ld, yo.ptr, yo.ld, 2048, ch, _stream()), 'dh_copy_channels_f32')
    assert SV.same_bits(yo.get('copy far ' + far), v)
    del xi, yo
    FV.release()


@pytest.mark.parametrize('shape', [(3, 16, 16, 17), (2, 64, 64, 5)])
@pytest.mark.parametrize('far', ['h', 'prob'])
def test_softargmax2d_past_4_gib(far, shape, hip_lib, cuda):
    """softargmax2d_kernel<4, staged> on 768 pixels and <4, unstaged> on 8192, the maps or the probability output on a span
    just past 2^32 bytes: the assertions and bars of test_gpu_slab_ops (_sam_check)."""
    assert SV.sam_variant(hip_lib, *shape) == SV.SAM_VARIANT_SHAPES[shape]
    r = TSO._sam_case(shape)
    f, hh, ww, ch = shape
    ld = _far_ld(f * hh * ww)
    x = _place(r['h'], ld if far == 'h' else 0, 0)
    route = SV.sam_route(hip_lib, f, hh, ww, ch, ldh=x.ld)                  # the instantiation does not depend on the pitch
    assert route.rc == 0 and (route.channels, bool(route.staged)) == SV.SAM_VARIANT_SHAPES[shape]
    prob = _place(shape, ld if far == 'prob' else 0, 1, out=True)
    gx = TSO._dev(np.linspace(0.0, 1.0, num=ww).astype(np.float32), cuda)
    gy = TSO._dev(np.linspace(0.0, 1.0, num=hh).astype(np.float32), cuda)
    xy, cr = TSO._Out((f, ch, 2), 3, 0), TSO._Out((f, ch, 1), 2, 1)
    a = TSO._lib().SamArgs()
    a.h, a.gx, a.gy, a.xy, a.conf_raw, a.prob = x.ptr, gx.data_ptr(), gy.data_ptr(), xy.ptr, cr.ptr, prob.ptr
    a.F, a.H, a.W, a.C, a.ldh, a.ldxy, a.ldcr, a.ldcp, a.ldp = f, hh, ww, ch, x.ld, 3, 2, 1, prob.ld
    a.alpha, a.conf_scale, a.xy_times_conf = 1.0, 4.0, 0
    TSO._run(hip_lib.dh_softargmax2d_f32(C.byref(a), _stream()), 'dh_softargmax2d_f32')
    out = dict(xy=xy.get('xy'), conf_raw=cr.get('conf_raw'), prob=prob.get('prob').reshape(shape))
    TSO._sam_check(out, r, 'softargmax2d %s far %s' % (shape, far))
    del x, prob
    FV.release()


def test_softargmax2d_context_past_4_gib(hip_lib, cuda):
    """dh_softargmax2d_context_f32, 8 joints + 16 context maps on 512 pixels at 2097156 floats: test_gpu_slab_ops' statement."""
    f, hh, ww, j, nctx = 2, 16, 16, 8, 2
    ch = j * (1 + nctx)
    h = _rand(np.random.default_rng(77), (f, hh, ww, ch), 4.0) + 1.0
    t = torch.from_numpy(h).double()
    hs, hc = t[..., :j], t[..., j:]
    ref = O.context_aggregation(O.softargmax2d(hs), O.softargmax2d(hc), O.joints_probability(hc), j, nctx, 0.8).numpy()
    gx = TSO._dev(np.linspace(0.0, 1.0, num=ww).astype(np.float32), cuda)
    gy = TSO._dev(np.linspace(0.0, 1.0, num=hh).astype(np.float32), cuda)
    x, y, conf = _FarIn(h, _far_ld(f * hh * ww)), TSO._Out((f, j, 2), 3, 0), TSO._Out((f, j, 1), 2, 1)
    a = TSO._lib().SamArgs()
    a.h, a.gx, a.gy, a.conf_raw = x.ptr, gx.data_ptr(), gy.data_ptr(), conf.ptr
    a.F, a.H, a.W, a.C, a.ldh, a.ldcr = f, hh, ww, ch, x.ld, 2
    a.alpha, a.conf_scale = 1.0, 1.0
    TSO._run(hip_lib.dh_softargmax2d_context_f32(C.byref(a), j, nctx, 0.8, y.ptr, 3, _stream()), 'dh_softargmax2d_context_f32')
    assert np.abs(y.get('context pose').astype(np.float64) - ref).max() <= TSO.BAR
    TSO._close(conf.get('context conf'), O.joints_probability(hs).numpy(), atol=1e-5, what='joint confidence')
    del x
    FV.release()


@pytest.mark.parametrize('off', [4, 3])
def test_depth_means_past_4_gib(off, hip_lib, cuda):
    """The one-pass kernel (aligned view) and the two-kernel path (odd offset) on 6048 pixels: test_depth_means_on_views' bounds."""
    f, hw, dd, j = 96, 7 * 9, 4, 5
    h = _rand(np.random.default_rng(120 + dd + j), (f, hw, dd * j), 30.0) + 100.0
    h5 = h.astype(np.float64).reshape(f, hw, dd, j)
    x = _FarIn(h, _far_ld(f * hw), off)
    hxy, hz = TSO._flat_out((f, hw, j), 0), TSO._flat_out((f, dd, j), 1)
    TSO._run(hip_lib.dh_depth_means_f32(x.ptr, x.ld, hxy.ptr, hz.ptr, f, hw, dd, j, _stream()), 'dh_depth_means_f32')
    exy = np.abs(hxy.get('hxy').astype(np.float64) - h5.mean(axis=2)).max()
    ez = np.abs(hz.get('hz').astype(np.float64) - h5.mean(axis=1)).max()
    assert exy <= 4 * 130 * 2.0 ** -24 and ez <= 3 * 130 * 2.0 ** -24, (exy, ez)
    del x
    FV.release()


@pytest.mark.parametrize('far', ['d', 'h'])
def test_depth_from_maps_past_4_gib(far, hip_lib, cuda):
    f, hw, j = 3, 32 * 32, 17
    rng = np.random.default_rng(f + hw + j)
    d = _rand(rng, (f, hw, j), 2.0)
    m = rng.standard_normal((f, hw, j)) * 2.0
    e = np.exp(m - m.max(axis=1, keepdims=True))
    h = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    ref = (1.0 / (1.0 + np.exp(-d.astype(np.float64))) * h.astype(np.float64)).sum(axis=1)
    ld = _far_ld(f * hw)
    xd, xh, z = _place(d, ld if far == 'd' else 0, 0), _place(h, ld if far == 'h' else 0, 1), TSO._Out((f, j, 1), 3, 2)
    TSO._run(hip_lib.dh_depth_from_maps_f32(xd.ptr, xd.ld, xh.ptr, xh.ld, z.ptr, 3, f, hw, j, _stream()), 'dh_depth_from_maps_f32')
    err = np.abs(z.get('depth_from_maps')[..., 0].astype(np.float64) - ref).max()
    assert err <= TSO.BAR, err
    del xd, xh
    FV.release()


@pytest.mark.parametrize('far', ['hm', 'x'])
def test_kronecker_past_4_gib(far, hip_lib, cuda):
    b, p, j, ch = 2, 64, 17, 60
    rng = np.random.default_rng(17)
    hm = rng.random((b, p, j)).astype(np.float32)
    hm /= hm.sum(axis=1, keepdims=True)
    v = _rand(rng, (b, p, ch))
    ref = np.einsum('bpj,bpc->bjc', hm.astype(np.float64), v.astype(np.float64))
    ld = _far_ld(b * p)
    xh, xv, y = _place(hm, ld if far == 'hm' else 0, 0), _place(v, ld if far == 'x' else 0, 1), TSO._Out((b, j, ch), 63, 3)
    TSO._run(hip_lib.dh_kronecker_f32(xh.ptr, xh.ld, xv.ptr, xv.ld, y.ptr, 63, b, p, j, ch, _stream()), 'dh_kronecker_f32')
    TSO._close(y.get('kronecker'), ref, atol=2e-6, rtol=1e-5, what='kron far ' + far)
    del xh, xv
    FV.release()


def test_global_maxmin_softmax_past_4_gib(hip_lib, cuda):
    b, p, ch = 3, 80, 300
    v = _rand(np.random.default_rng(b + p + ch), (b, p, ch), 2.0)
    s32 = v.max(axis=1) + v.min(axis=1)
    s = v.astype(np.float64).max(axis=1) + v.astype(np.float64).min(axis=1)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    ref = e / e.sum(axis=1, keepdims=True)
    x = _FarIn(v, _far_ld(b * p), 5)
    for softmax in (0, 1):
        y = TSO._flat_out((b, ch), 1)
        TSO._run(hip_lib.dh_global_maxmin_softmax_f32(x.ptr, x.ld, y.ptr, b, p, ch, softmax, _stream()), 'dh_global_maxmin_softmax_f32')
        got = y.get('global_maxmin')
        if softmax:
            TSO._close(got, ref, atol=1e-8, rtol=1e-5, what='action_top far')
        else:
            assert SV.same_bits(got, s32)
    del x
    FV.release()
