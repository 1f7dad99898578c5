"""Op-level tests of the convolution kernels on channel-slab views (tests/convview.py, tests/slabview.py).

The planner never hands a convolution a dense tensor if it can avoid it: R4 makes it write into its slab of a concatenation
buffer (ldy > Cout, a channel offset), R10 / R10c make its input a run of channels of a joint buffer (ldx > Cin), residuals and
the pooled second output carry pitches of their own, and with 17-joint heads the offsets are no multiples of four, so the
launcher drops to the register-gather kernel, the scalar A load and the scalar epilogue.  deephar_amd/functional.conv2d only
ever passes dense, 16-byte aligned tensors; here every operand of every kernel family sits on a view:

  * inputs in slabs filled with NaN (LOUD = 2**100 where the LDS-DMA family reads padded k slots from the neighbouring
    channels and multiplies them by zero weights), outputs in slabs of canaries checked bit for bit after every launch;
  * layout sets dense / aligned / odd, one set per operand with that operand alone odd, and the unaligned BN tables;
  * every set gives the bits of the dense launch of the same tiling (and all tilings of a layer the same bits); the dense
    result is held once to the fp64 statement of the layer by the family's existing bar (tests/test_gpu_ops.py):
    fp32 families e_hip <= 4 e_cpu + 1e-6 with e_cpu the fp32 CPU oracle's own error, bf16x3 e_split <= 2 e_f32 + 1e-6;
  * a launch may answer DH_EUNSUPPORTED only where convview.refusal says so, and then it has written nothing.

tests/test_conv_views_host.py proves (without a GPU) that each case reaches the family and the code path it is there for.
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
import slabview as SV                              # noqa: E402
from oracle import ops as O                        # noqa: E402

pytestmark = pytest.mark.gpu

NAN = np.nan


def _rand(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _resampled(x, mode):
    """The tensor a stand-alone up-sampling / pooling launch writes from x (dh_conv_args.x_resample), in fp32."""
    if mode == 0:
        return x
    if mode == 1:
        return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    n, h, w, c = x.shape
    win = x.reshape(n, h // 2, 2, w // 2, 2, c)
    return win.max(axis=(2, 4)) if mode == 2 else (win.max(axis=(2, 4)) + win.min(axis=(2, 4))).astype(np.float32)


def _pool2(y):
    n, h, w, c = y.shape
    return y.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


@functools.lru_cache(maxsize=None)
def _data(name):
    """Seeded operands of a case (shared by every launch of it, never modified)."""
    case = CV.CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    d = {}
    if case.x_u8:
        from deephar_amd.engine.executor import normalization_lut
        d['x_u8'] = rng.integers(0, 256, case.shape_of('x'), dtype=np.uint8)
        d['lut'] = normalization_lut(3, 1)
        d['x'] = d['lut'][np.arange(3)[None, None, None, :], d['x_u8']].astype(np.float32)     # the loader's float32 values
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


def _statement(case, d, dtype):
    """The layer in plain oracle ops at `dtype` (fp64: the truth; fp32: the CPU oracle whose error sets the bar)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    x = t(_resampled(d['x'], case.x_resample))
    if case.pre_bn:
        x = x * t(d['pre_scale']) + t(d['pre_shift'])
    if case.pre_relu:
        x = O.relu(x)
    y = O.conv2d(x, t(d['w']), (case.stride, case.stride), 'same')
    if case.bn:
        y = y * t(d['post_scale']) + t(d['post_shift'])
    if case.res1:
        y = y + t(d['res1'])
    if case.up2:
        y = O.upsample2d(y)
    if case.res2:
        y = y + (O.upsample2d(t(d['res2'])) if case.res2 == 'down' else t(d['res2']))
    return (O.relu(y) if case.relu else y).double().numpy()


@functools.lru_cache(maxsize=None)
def _truth(name):
    """(fp64 statement, max error of the fp32 CPU oracle against it) -- computed once per layer."""
    case, d = CV.CASES[name], _data(name)
    ref = _statement(case, d, torch.float64)
    return ref, float(np.abs(_statement(case, d, torch.float32) - ref).max())


def _same(a, b, what):
    assert SV.same_bits(a, b), '%s: differs in bits (max |d| = %.3e)' % (what, float(np.nanmax(np.abs(a - b))))


# ------------------------------------------------------------------------------------------------------------------------
# dh_conv2d_f32: (a) .. (k), refusals (m)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CV.CASES))
def test_conv2d_on_views(name, hip_lib, cuda):
    case, d = CV.CASES[name], _data(name)
    w = CV.pack(case, d['w'])
    sets = CV.layout_sets(case)
    eligible = True
    if case.family == 'split':                     # a shape the split modes refuse, they refuse on every layout and tiling
        eligible = bool(hip_lib.dh_conv2d_split_eligible(C.byref(CV.fake_args(case, sets['dense'][0], False))))
        assert eligible == ('13x11' not in name)
    # ---- dense: every tiling named must run, all tilings give the same bits
    dense = {}
    for cfg in case.cfgs:
        rc, out = CV.launch(hip_lib, case, d, sets['dense'][0], w, cfg, what='%s dense cfg %d' % (name, cfg))
        if case.family == 'split':                 # tilings a mode does not have (the wide ones below three parts)
            assert rc == (0 if eligible and not (cfg in (14, 15) and case.w_split != 1) else CV.DH_EUNSUPPORTED), (name, cfg, rc)
        else:
            assert rc == 0, '%s dense tile_cfg %d: rc = %d' % (name, cfg, rc)
        dense[cfg] = (rc, out)
    ran = [c for c in case.cfgs if dense[c][0] == 0]
    for cfg in ran[1:]:
        _same(dense[cfg][1]['y'], dense[ran[0]][1]['y'], '%s: tile_cfg %d against tile_cfg %d' % (name, cfg, ran[0]))
    # ---- dense against the fp64 statement, by the family's existing bar
    if ran:
        ref, e_cpu = _truth(name)
        e_hip = float(np.abs(dense[ran[0]][1]['y'].astype(np.float64) - ref).max())
        if case.w_split in (0, 2):
            print('%s: |hip - fp64| = %.3e   |fp32 cpu - fp64| = %.3e' % (name, e_hip, e_cpu))
            assert e_hip <= 4 * e_cpu + 1e-6, (name, e_hip, e_cpu)
        else:
            twin = CV.Case(name + '_f32', (case.N, case.H, case.W, case.Cin), case.Cout, k=case.k, stride=case.stride, pre=case.pre,
                           bn=case.bn, relu=case.relu, res1=case.res1)
            rc, f32 = CV.launch(hip_lib, twin, d, sets['dense'][0], CV.pack(twin, d['w']), -1, what=name + ' fp32 twin')
            assert rc == 0
            e_f32 = float(np.abs(f32['y'].astype(np.float64) - ref).max())
            print('%s: |split - fp64| = %.3e   |fp32 mfma - fp64| = %.3e   |fp32 cpu - fp64| = %.3e' % (name, e_hip, e_f32, e_cpu))
            if case.w_split == 1:
                assert e_hip <= 2 * e_f32 + 1e-6, (name, e_hip, e_f32)
    # ---- every other layout set: the bits of dense on the same tiling, or a listed refusal that wrote nothing
    for sname, (lay, tabs) in sets.items():
        if sname == 'dense':
            continue
        for cfg in case.cfgs:
            what = '%s %s cfg %d' % (name, sname, cfg)
            why = CV.refusal(case, lay, tabs, cfg)
            rc, out = CV.launch(hip_lib, case, d, lay, w, cfg, tables_unaligned=tabs, what=what)
            if why is not None:
                assert rc == CV.DH_EUNSUPPORTED, '%s: rc = %d, expected a refusal (%s)' % (what, rc, why)
                continue
            assert rc == dense[cfg][0], '%s: rc = %d, dense answered %d' % (what, rc, dense[cfg][0])
            if rc == 0:
                _same(out['y'], dense[cfg][1]['y'], what)
                if case.pool:
                    _same(out['y_pool'], dense[cfg][1]['y_pool'], what + ' (pooled)')
    # ---- the pooled second output is MaxPooling2D((2, 2)) of the y that was read back
    if case.pool:
        for cfg in ran:
            assert np.array_equal(dense[cfg][1]['y_pool'], _pool2(dense[cfg][1]['y'])), '%s cfg %d: y_pool' % (name, cfg)
    # ---- first layer: dense frames from a base 4 bytes past a 16-byte boundary, uint8 frames = the float frames
    if case.family == 'stem':
        rc, out = CV.launch(hip_lib, case, d, sets['aligned'][0], w, -1, x_lead=4 if case.x_u8 else 1, what=name + ' shifted base')
        assert rc == 0
        _same(out['y'], dense[-1][1]['y'], name + ' shifted base')
        if case.x_u8:                              # the float kernel on the loader's float32 values of the same bytes
            rc, yf = CV.launch(hip_lib, CV.CASES['k_stem'], d, sets['dense'][0], w, -1, what='k_stem on the same frames')
            assert rc == 0
            _same(yf['y'], dense[-1][1]['y'], 'uint8 frames against their float32 values')


def test_an_odd_x_sends_the_library_pick_to_the_general_kernel(hip_lib, cuda):
    """tile_cfg = -1 on a DMA-eligible fp32 layer whose x is not 16-byte aligned: the register-gather kernel, with the bits
    of general-kernel tile_cfg = 3 on the dense tensor."""
    for name in ('b_dma', 'b_dma_ktail', 'b_dma_bn_prologue'):
        case, d = CV.CASES[name], _data(name)
        w = CV.pack(case, d['w'])
        sets = CV.layout_sets(case)
        rc, want = CV.launch(hip_lib, case, d, sets['dense'][0], w, 3)
        assert rc == 0
        for sname in ('odd', 'odd_x'):
            rc, got = CV.launch(hip_lib, case, d, sets[sname][0], w, -1, what='%s %s' % (name, sname))
            assert rc == 0
            _same(got['y'], want['y'], '%s %s tile_cfg -1 against dense tile_cfg 3' % (name, sname))


# ------------------------------------------------------------------------------------------------------------------------
# (j) dh_conv2d_seg_f32, dh_conv2d_pair_f32
# ------------------------------------------------------------------------------------------------------------------------
def _skinny_struct(case, ptr, ld, wt, tab):
    return CV.fill_args(case, ptr, ld, wt.data_ptr(), tab)


def _tables(case, d, unaligned=False):
    keep, tab = [], {}
    for n in (['pre_scale', 'pre_shift'] if case.pre_bn else []) + (['post_scale', 'post_shift'] if case.bn else []):
        t, tab[n] = CV.table(d[n], unaligned)
        keep.append(t)
    return keep, tab


def _pool_same(x, sh):
    """MaxPooling2D((2, 2), strides=(sh, 2), padding='same') of x [N, H, 2 W, C] (sh = 1: windows of two rows starting at every
    row, the last one a single row)."""
    n, h, w2, c = x.shape
    cols = x.reshape(n, h, w2 // 2, 2, c).max(axis=3)
    if sh == 2:
        return cols.reshape(n, h // 2, 2, w2 // 2, c).max(axis=2)
    nxt = np.concatenate([cols[:, 1:], cols[:, -1:]], axis=1)
    return np.maximum(cols, nxt)


@pytest.mark.parametrize('sh,cs', [(1, 64), (2, 64), (1, 66), (2, 66)])
def test_segmented_skinny_conv_on_views(sh, cs, hip_lib, cuda):
    """dh_conv2d_seg_f32 with x (ldx > c_split) and x2 on different views, c_split % 4 != 0 in two of the sets: bit for bit
    dh_conv2d_f32 on the tensor a pooling launch plus the concatenation would have written."""
    cd = 30 if cs % 4 else 32
    case = CV.Case('seg_%d_%d' % (sh, cs), (2, 8, 8, cs + cd), 48, k=3, pre='bnrelu', bn=True, res1=True, family='skinny')
    rng = np.random.default_rng(100 * sh + cs)
    x, x2 = _rand(rng, (2, 8 * sh, 16, cs)), _rand(rng, (2, 8, 8, cd))
    d = dict(x=np.concatenate([_pool_same(x, sh), x2], axis=-1), w=_rand(rng, (3, 3, cs + cd, 48), np.sqrt(1.0 / case.K)),
             pre_scale=rng.uniform(0.5, 1.5, cs + cd).astype(np.float32), pre_shift=_rand(rng, (cs + cd,), 0.3),
             post_scale=rng.uniform(0.5, 1.5, 48).astype(np.float32), post_shift=_rand(rng, (48,), 0.3),
             res1=_rand(rng, (2, 8, 8, 48)))
    w = CV.pack(case, d['w'])
    rc, want = CV.launch(hip_lib, case, d, CV.layout_sets(case)['dense'][0], w)
    assert rc == 0
    assert hip_lib.dh_conv2d_uses_split_k(C.byref(CV.fake_args(case, CV.layout_sets(case)['dense'][0], False))) == 1
    from deephar_amd import _lib
    names = {'x': 0, 'y': 1, 'res1': 2, 'x2': 3}
    runs = {'dense': {}, 'aligned': {}, 'odd': {}}
    for o in names:
        for s in ('dense', 'aligned', 'odd'):
            runs[s][o] = s
        runs['odd_' + o] = dict({p: 'aligned' for p in names}, **{o: 'odd'})
    for sname, lay in runs.items():
        ch = {'x': cs, 'y': 48, 'res1': 48, 'x2': cd}
        L = {o: SV.layout(ch[o], lay[o], names[o]) for o in names}
        if sname == 'dense':
            L['x'] = (cs + 4, 0)                                     # ldx > c_split on every set
        tx, px = SV.slab(x, L['x'][0], L['x'][1], NAN)
        t2, p2 = SV.slab(x2, L['x2'][0], L['x2'][1], NAN)
        tr, pr = SV.slab(d['res1'], L['res1'][0], L['res1'][1], NAN)
        ty, py = SV.out_slab((2, 8, 8, 48), L['y'][0], L['y'][1])
        keep, tab = _tables(case, d, unaligned=sname == 'odd')
        a = _skinny_struct(case, dict(x=px, y=py, res1=pr), dict(x=L['x'][0], y=L['y'][0], res1=L['res1'][0]), w[0], tab)
        seg = _lib.ConvSeg()
        seg.x2, seg.ldx2, seg.c_split, seg.pool_sh = p2, L['x2'][0], cs, sh
        assert a.ldx > cs
        rc = hip_lib.dh_conv2d_seg_f32(C.byref(a), C.byref(seg), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (sname, rc)
        SV.assert_untouched(ty, L['y'][1], 48, what='seg %s' % sname)
        _same(SV.view(ty, L['y'][1], 48), want['y'], 'seg pool_sh %d c_split %d %s' % (sh, cs, sname))


@pytest.mark.parametrize('lname', ['dense', 'aligned', 'odd'])
def test_pair_launch_writes_neighbouring_slabs_of_one_buffer(lname, hip_lib, cuda):
    """dh_conv2d_pair_f32 with the two outputs in neighbouring slabs of ONE buffer, as the planner lays out the concatenation
    behind them: each slab equals its own single launch, the canary between and around the slabs is intact."""
    ca = CV.Case('pair_a', (2, 8, 8, 64), 24, k=3, pre='relu', bn=True, res1=True, family='skinny')
    cb = CV.Case('pair_b', (2, 8, 8, 70), 40, pre='bnrelu', bn=True, family='skinny')
    rng = np.random.default_rng(77)
    data, want, packed = {}, {}, {}
    for c in (ca, cb):
        dd = dict(x=_rand(rng, c.shape_of('x')), w=_rand(rng, (c.k, c.k, c.Cin, c.Cout), np.sqrt(1.0 / c.K)),
                  post_scale=rng.uniform(0.5, 1.5, c.Cout).astype(np.float32), post_shift=_rand(rng, (c.Cout,), 0.3))
        if c.pre_bn:
            dd['pre_scale'], dd['pre_shift'] = rng.uniform(0.5, 1.5, c.Cin).astype(np.float32), _rand(rng, (c.Cin,), 0.3)
        if c.res1:
            dd['res1'] = _rand(rng, c.shape_of('res1'))
        data[c.name], packed[c.name] = dd, CV.pack(c, dd['w'])
        rc, out = CV.launch(hip_lib, c, dd, CV.layout_sets(c)['dense'][0], packed[c.name])
        assert rc == 0
        want[c.name] = out['y']
    gap = {'dense': 0, 'aligned': 0, 'odd': 1}[lname]              # the odd set leaves one canary channel between the slabs
    span = 24 + gap + 40
    ld, off = {'dense': (span, 0), 'aligned': (span + 8, 4), 'odd': (span + 4, 1)}[lname]
    ty, py = SV.out_slab((2, 8, 8, span), ld, off)
    keep, structs = [], []
    for i, (c, yoff) in enumerate(((ca, 0), (cb, 24 + gap))):
        dd = data[c.name]
        lx = SV.layout(c.Cin, lname, 2 * i)
        tx, px = SV.slab(dd['x'], lx[0], lx[1], NAN)
        ptr, lds = dict(x=px, y=py + 4 * yoff), dict(x=lx[0], y=ld)
        if c.res1:
            lr = SV.layout(c.Cout, lname, 2 * i + 1)
            tr, ptr['res1'] = SV.slab(dd['res1'], lr[0], lr[1], NAN)
            lds['res1'] = lr[0]
            keep.append(tr)
        k2, tab = _tables(c, dd, unaligned=lname == 'odd')
        keep += [tx] + k2
        structs.append(_skinny_struct(c, ptr, lds, packed[c.name][0], tab))
    for first, second in ((0, 1), (1, 0)):
        ty.fill_(SV.CANARY)
        rc = hip_lib.dh_conv2d_pair_f32(C.byref(structs[first]), C.byref(structs[second]), _stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        SV.assert_untouched(ty, off, span, what='pair %s' % lname)
        got = SV.view(ty, off, span)
        _same(got[..., :24], want['pair_a'], 'pair %s: first slab' % lname)
        _same(got[..., 24 + gap:], want['pair_b'], 'pair %s: second slab' % lname)
        if gap:
            assert np.all(got[..., 24:24 + gap] == SV.CANARY), 'pair %s: wrote between the slabs' % lname


# ------------------------------------------------------------------------------------------------------------------------
# (l) dh_conv2d_dw_group_f32, dh_dwconv2d_f32 with up_in, the transposed convolutions
# ------------------------------------------------------------------------------------------------------------------------
def _dw_struct(px, ldx, pw, py, ldy, n, h, w, c, k, tab, up_in=0):
    from deephar_amd import _lib
    g = _lib.DwArgs()
    g.x, g.w, g.y, g.pre_scale, g.pre_shift = px, pw, py, tab.get('pre_scale'), tab.get('pre_shift')
    g.N, g.H, g.W, g.C, g.ldx, g.ldy = n, h, w, c, ldx, ldy
    g.KH = g.KW = k
    g.PT, g.PL, g.pre_relu, g.up_in = CV.same_pad(h, k, 1)[0], CV.same_pad(w, k, 1)[0], int(bool(tab)), up_in
    return g


@pytest.mark.parametrize('cout', [48, 264])
def test_grouped_conv_dw_launch_on_views(cout, hip_lib, cuda):
    """dh_conv2d_dw_group_f32: the 1x1 convolution (2, 16, 16, 96 -> cout) beside a 5x5 depthwise convolution on the same 96
    channels, both behind BN + ReLU, x shared, the two outputs and res1 on aligned views: bit-equal to dh_conv2d_f32 +
    dh_dwconv2d_f32 on the same views.  96 -> 48 on a 16 x 16 map is a skinny layer by the shape rule (256 positions, K = 96):
    the group refuses it (-2, nothing written); 96 -> 264 is the pair that runs.  With one operand odd: a misaligned conv
    output or residual runs (scalar epilogue, same bits), a misaligned x or depthwise output is refused."""
    case = CV.Case('group_%d' % cout, (2, 16, 16, 96), cout, pre='bnrelu', bn=True, res1=True)
    rng = np.random.default_rng(cout)
    d = dict(x=_rand(rng, (2, 16, 16, 96)), w=_rand(rng, (1, 1, 96, cout), np.sqrt(1.0 / 96)),
             pre_scale=rng.uniform(0.5, 1.5, 96).astype(np.float32), pre_shift=_rand(rng, (96,), 0.3),
             post_scale=rng.uniform(0.5, 1.5, cout).astype(np.float32), post_shift=_rand(rng, (cout,), 0.3),
             res1=_rand(rng, (2, 16, 16, cout)))
    dwk = _rand(rng, (25, 96), 0.2)
    wt, kp, np_ = CV.pack(case, d['w'])
    dwt = torch.from_numpy(dwk).cuda()
    skinny = bool(hip_lib.dh_conv2d_uses_split_k(C.byref(CV.fake_args(case, CV.layout_sets(case)['aligned'][0], False))))
    assert skinny == (cout == 48)
    for odd in (None, 'x', 'y', 'res1', 'yd'):
        lay = {o: ('odd' if o == odd else 'aligned') for o in ('x', 'y', 'res1', 'yd')}
        L = dict(x=SV.layout(96, lay['x'], 0), y=SV.layout(cout, lay['y'], 1), res1=SV.layout(cout, lay['res1'], 2),
                 yd=SV.layout(96, lay['yd'], 3))
        tx, px = SV.slab(d['x'], L['x'][0], L['x'][1], NAN)
        tr, pr = SV.slab(d['res1'], L['res1'][0], L['res1'][1], NAN)
        keep, tab = _tables(case, d)
        outs = {}
        for which in ('group', 'single'):
            ty, py = SV.out_slab((2, 16, 16, cout), *L['y'])
            td, pd = SV.out_slab((2, 16, 16, 96), *L['yd'])
            a = CV.fill_args(case, dict(x=px, y=py, res1=pr), dict(x=L['x'][0], y=L['y'][0], res1=L['res1'][0]), wt.data_ptr(), tab)
            g = _dw_struct(px, L['x'][0], dwt.data_ptr(), pd, L['yd'][0], 2, 16, 16, 96, 5, tab)
            if which == 'group':
                rc = hip_lib.dh_conv2d_dw_group_f32(C.byref(a), C.byref(g), _stream())
                torch.cuda.synchronize()
                want_rc = CV.DH_EUNSUPPORTED if skinny or odd in ('x', 'yd') else 0
                assert rc == want_rc, ('group', cout, odd, rc)
                if rc != 0:
                    SV.assert_untouched(ty, 0, 0, what='refused group: conv output')
                    SV.assert_untouched(td, 0, 0, what='refused group: depthwise output')
                    break
            else:
                assert hip_lib.dh_conv2d_f32(C.byref(a), -1, _stream()) == 0
                assert hip_lib.dh_dwconv2d_f32(C.byref(g), _stream()) == 0
                torch.cuda.synchronize()
            SV.assert_untouched(ty, L['y'][1], cout, what='%s conv output, odd %s' % (which, odd))
            SV.assert_untouched(td, L['yd'][1], 96, what='%s depthwise output, odd %s' % (which, odd))
            outs[which] = (SV.view(ty, L['y'][1], cout), SV.view(td, L['yd'][1], 96))
        if outs:
            _same(outs['group'][0], outs['single'][0], 'group %d odd %s: conv half' % (cout, odd))
            _same(outs['group'][1], outs['single'][1], 'group %d odd %s: depthwise half' % (cout, odd))


@pytest.mark.parametrize('shape,k', [((2, 8, 8, 32), 5), ((1, 3, 5, 20), 3)])
def test_dwconv_reads_an_upsampled_view(shape, k, hip_lib, cuda):
    """dh_dwconv2d_f32 with up_in = 1 on dense, aligned and odd views (x at half resolution): the bits of the convolution of
    the explicitly up-sampled tensor on the same views, every layout the same bits (one summation order in all stride-1
    kernels), and test_dwconv's bar (atol 1e-5, rtol 2e-5) against the fp64 statement."""
    n, h, w, c = shape
    rng = np.random.default_rng(sum(shape) + k)
    x, dwk = _rand(rng, shape), _rand(rng, (k, k, c, 1), 1.0 / k)
    ps, pb = rng.uniform(0.5, 1.5, c).astype(np.float32), _rand(rng, (c,), 0.3)
    up = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    t = lambda a_: torch.from_numpy(a_).double()
    ref = O.depthwise_conv2d(O.relu(t(up) * t(ps) + t(pb)), t(dwk)).numpy()
    dwt = torch.from_numpy(np.ascontiguousarray(dwk.reshape(k * k, c))).cuda()
    got = {}
    for lname in SV.LAYOUTS:
        for src, up_in in ((x, 1), (up, 0)):
            lx, ly = SV.layout(c, lname, 0), SV.layout(c, lname, 1)
            tx, px = SV.slab(src, lx[0], lx[1], NAN)
            ty, py = SV.out_slab((n, 2 * h, 2 * w, c), ly[0], ly[1])
            keep = [CV.table(ps, lname == 'odd'), CV.table(pb, lname == 'odd')]
            g = _dw_struct(px, lx[0], dwt.data_ptr(), py, ly[0], n, 2 * h, 2 * w, c, k,
                           dict(pre_scale=keep[0][1], pre_shift=keep[1][1]), up_in)
            rc = hip_lib.dh_dwconv2d_f32(C.byref(g), _stream())
            torch.cuda.synchronize()
            assert rc == 0, (lname, up_in, rc)
            SV.assert_untouched(ty, ly[1], c, what='dw up_in=%d %s' % (up_in, lname))
            got[(lname, up_in)] = SV.view(ty, ly[1], c)
        _same(got[(lname, 1)], got[(lname, 0)], 'dw %s: up_in against the up-sampled tensor' % lname)
        err = np.abs(got[(lname, 1)] - ref)
        print('dw up_in %s %s: max err %.3e' % (shape, lname, err.max()))
        assert np.all(err <= 1e-5 + 2e-5 * np.abs(ref)), (lname, err.max())
    for lname in ('aligned', 'odd'):
        _same(got[(lname, 1)], got[('dense', 1)], 'dw up_in %s against dense' % lname)


@pytest.mark.parametrize('cout', CV.CONVT_COUTS)
@pytest.mark.parametrize('parts', [0, 3])
def test_transposed_conv_on_views(cout, parts, hip_lib, cuda):
    """dh_conv2d_transpose2x2_f32 (parts = 0) and dh_conv2d_transpose2x2_split_f32(parts = 3) at (2, 6, 5, 24 -> cout): x on an
    aligned view with a non-zero offset, y and res in three layouts and one at a time odd; cb = 18 is the scalar
    depth-to-space store.  LOUD around x (K = 24 is padded to 32 from the neighbouring channels); an odd x is refused."""
    from deephar_amd import _lib, functional as F
    import resample_ref as R
    n, h, w, cin = CV.CONVT_SHAPE
    rng = np.random.default_rng(cout + parts)
    x, k = _rand(rng, (n, h, w, cin)), _rand(rng, (2, 2, cout, cin), np.sqrt(1.0 / cin))
    ps, pb = rng.uniform(0.5, 1.5, cin).astype(np.float32), _rand(rng, (cin,), 0.3)
    res = _rand(rng, (n, 2 * h, 2 * w, cout))
    wt, kp, np_ = F.pack_convt_weight(k, 'cuda', parts=parts or None)
    t = lambda a_, dt: torch.from_numpy(a_).to(dt)
    st = lambda dt: R.conv_transpose2x2(t(x, dt), t(k, dt), t(ps, dt), t(pb, dt), True, t(res, dt), True).double().numpy()
    ref = st(torch.float64)
    e_cpu = float(np.abs(st(torch.float32) - ref).max())

    def run(lx, ly, lr, split, tabs=False, weight=None):
        weight = wt if weight is None else weight
        Lx, Ly, Lr = SV.layout(cin, lx, 0), SV.layout(cout, ly, 1), SV.layout(cout, lr, 2)
        tx, px = SV.slab(x, Lx[0], Lx[1], CV.LOUD)
        tr, pr = SV.slab(res, Lr[0], Lr[1], NAN)
        ty, py = SV.out_slab((n, 2 * h, 2 * w, cout), Ly[0], Ly[1])
        keep = [CV.table(ps, tabs), CV.table(pb, tabs)]
        a = _lib.ConvtArgs()
        a.x, a.w, a.y, a.pre_scale, a.pre_shift, a.res = px, weight.data_ptr(), py, keep[0][1], keep[1][1], pr
        a.N, a.H, a.W, a.Cin, a.ldx, a.Cout, a.ldy, a.ldr = n, h, w, cin, Lx[0], cout, Ly[0], Lr[0]
        a.Kp, a.Np, a.pre_relu, a.post_relu = kp, np_, 1, 1
        if split:
            assert hip_lib.dh_conv2d_transpose2x2_split_eligible(C.byref(a)) == int(lx != 'odd')
            rc = hip_lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), parts, -1, _stream())
        else:
            rc = hip_lib.dh_conv2d_transpose2x2_f32(C.byref(a), -1, _stream())
        torch.cuda.synchronize()
        if rc != 0:
            SV.assert_untouched(ty, 0, 0, what='refused convT')
            return rc, None
        SV.assert_untouched(ty, Ly[1], cout, what='convT x %s y %s res %s' % (lx, ly, lr))
        return rc, SV.view(ty, Ly[1], cout)

    rc, dense = run('aligned', 'dense', 'dense', bool(parts))
    assert rc == 0
    e_hip = float(np.abs(dense - ref).max())
    if parts:
        rc, f32 = run('aligned', 'dense', 'dense', False, weight=F.pack_convt_weight(k, 'cuda')[0])
        e_f32 = float(np.abs(f32 - ref).max())
        print('convT -> %d bf16x3: |split - fp64| = %.3e   |fp32 mfma - fp64| = %.3e' % (cout, e_hip, e_f32))
        assert rc == 0 and e_hip <= 2 * e_f32 + 1e-6, (e_hip, e_f32)
    else:
        print('convT -> %d fp32: |hip - fp64| = %.3e   |fp32 cpu - fp64| = %.3e' % (cout, e_hip, e_cpu))
        assert e_hip <= 4 * e_cpu + 1e-6, (e_hip, e_cpu)
    for ly, lr, tabs in (('aligned', 'aligned', False), ('odd', 'odd', False), ('odd', 'aligned', False), ('aligned', 'odd', False),
                         ('aligned', 'aligned', True)):
        rc, got = run('aligned', ly, lr, bool(parts), tabs)
        assert rc == 0, (ly, lr, tabs, rc)
        _same(got, dense, 'convT -> %d parts %d: y %s res %s tables %s' % (cout, parts, ly, lr, tabs))
    rc, _ = run('odd', 'aligned', 'aligned', bool(parts))
    assert rc == CV.DH_EUNSUPPORTED, rc
