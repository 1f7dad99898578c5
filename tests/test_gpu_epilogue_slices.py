"""The fp32 LDS-DMA GEMM finishes the direct tiles of its one-row-block tilings (TM == 1, tile_cfg 11..17) column tile by column
tile under the MFMAs of a peeled last K-step (csrc/gemm1x1_body.h, EpiDirect in csrc/conv_common.h).  The peeled step must
give the bits of every path that cannot take it.  Every case here launches dh_conv2d_f32 with each TM == 1 tiling and asserts
bitwise equality with

  * tile_cfg 9, the <2, 2, 2, 3> tiling (TM = 2: whole K loop, LDS-staged epilogue), on the same operands, and
  * the SAME tiling on a sub-problem whose tiles are ragged and therefore staged: the first frames of the batch where that
    leaves a partial last row block, else the first Cout - 4 (or - 8) output channels -- rows and columns of a convolution
    do not depend on their neighbours, so the sub-problem's values are the full launch's.

Shapes are the smallest that can still go wrong: nk = 1 (the peeled step is the only step), 2, a K tail inside a padded
K-step, nk = 18; one and two row tiles, a direct and a staged tile in one launch; all column tiles interior / an edge tile;
every epilogue flag on its own and together; the BN-prologue and ReLU-on-load forms; K x K with and without a stride; views
with canaries; the grouped launch.  A layer of at most 256 positions with K >= 64 and Cout <= 256 belongs to the skinny
kernel whatever tiling is asked for, so such cases carry 288 output channels or K < 64; `_check_route` asserts that every
launch is the LDS-DMA GEMM and that the full launch has direct tiles where the case is there for them.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convview as CV                              # noqa: E402
import slabview as SV                              # noqa: E402

pytestmark = pytest.mark.gpu

REF_CFG = 9                                        # <2, 2, 2, 3> on the LDS-DMA GEMM: TM = 2 never takes the peeled step
SLICED = (11, 12, 13, 14, 15, 16, 17)              # <4,1,1,3> <4,1,1,2> <4,1,1,1> <2,1,1,3> <2,1,1,2> <2,1,1,1> <1,1,1,1>
CONV_DMA = 2                                       # dh_conv_route.kernel


def _case(name, shape, cout, **kw):
    return CV.Case(name, shape, cout, cfgs=(REF_CFG,) + SLICED, **kw)


EPILOGUES = {
    'plain': {},
    'bn': dict(bn=True),
    'bn_res1': dict(bn=True, res1=True),
    'res1': dict(res1=True),
    'bn_res1_down_relu': dict(bn=True, res1=True, res2='down', relu=True),
    'down': dict(res2='down'),
}

CASES = [
    # K: nk = 1, 2, a K tail inside the second K-step, 18
    _case('k32', (4, 8, 8, 32), 288, bn=True, res1=True),
    _case('k64', (4, 8, 8, 64), 288, bn=True, res1=True),
    _case('k40', (4, 8, 8, 40), 288, bn=True, res1=True),
    _case('k576', (4, 8, 8, 576), 288, bn=True, res1=True, relu=True),
    # M: one row tile of WM = 4 (k64 above has two), then a direct and a staged one in the same launch
    _case('m128', (2, 8, 8, 64), 288, bn=True, res1=True),
    _case('m192', (3, 8, 8, 64), 288, bn=True, res1=True),
    # Cout: every column tile interior (288: k32), an edge tile
    _case('cout96', (4, 8, 8, 32), 96, bn=True, res1=True),
    _case('cout192', (4, 8, 8, 32), 192, bn=True, res1=True),
    _case('cout100', (4, 8, 8, 32), 100, bn=True, res1=True),
] + [
    # every epilogue on the two smallest maps the direct half-resolution residual exists on
    _case('epi_%s_%s' % (e, m), shape, 96, **kw)
    for e, kw in EPILOGUES.items() for m, shape in (('8x8', (2, 8, 8, 32)), ('16x16', (1, 16, 16, 32)))
] + [
    # BN prologue / ReLU on load (mixed signs in x: the ReLU is not the identity)
    _case('pre_relu', (4, 8, 8, 64), 288, pre='relu', bn=True, res1=True, relu=True),
    _case('pre_bn', (4, 8, 8, 64), 288, pre='bn', bn=True, res1=True),
    _case('pre_bnrelu', (4, 8, 8, 64), 288, pre='bnrelu', bn=True, res1=True, relu=True),
    _case('pre_bnrelu_k32', (4, 8, 8, 32), 96, pre='bnrelu', res1=True, res2='down'),
    # K x K
    _case('kxk_3x3', (2, 8, 8, 32), 288, k=3, bn=True, res1=True, relu=True),
    _case('kxk_3x3_relu_load', (2, 8, 8, 32), 288, k=3, pre='relu', res1=True),
    _case('kxk_3x3_s2', (2, 16, 16, 32), 288, k=3, stride=2, bn=True, res1=True),
]


def _data(case):
    rng = np.random.default_rng(sum(map(ord, case.name)))
    r = lambda shape, s=1.0: (rng.standard_normal(shape) * s).astype(np.float32)
    d = dict(x=r(case.shape_of('x')), w=r((case.k, case.k, case.Cin, case.Cout), np.sqrt(1.0 / case.K)))
    if case.pre_bn:
        d['pre_scale'], d['pre_shift'] = rng.uniform(0.5, 1.5, case.Cin).astype(np.float32), r((case.Cin,), 0.3)
    if case.bn:
        d['post_scale'], d['post_shift'] = rng.uniform(0.5, 1.5, case.Cout).astype(np.float32), r((case.Cout,), 0.3)
    for o in ('res1', 'res2'):
        if o in case.operands():
            d[o] = r(case.shape_of(o))
    return d


def _sub(case, d, frames=None, cout=None):
    """The first `frames` frames / the first `cout` output channels of a case, as a case of its own."""
    n = case.N if frames is None else frames
    co = case.Cout if cout is None else cout
    sub = CV.Case('%s_sub_%d_%d' % (case.name, n, co), (n, case.H, case.W, case.Cin), co, k=case.k, stride=case.stride, pre=case.pre,
                  bn=case.bn, relu=case.relu, res1=case.res1, res2=case.res2, cfgs=case.cfgs)
    d2 = {k: v for k, v in d.items()}
    d2['x'] = d['x'][:n]
    d2['w'] = np.ascontiguousarray(d['w'][..., :co])
    for k in ('post_scale', 'post_shift'):
        if k in d:
            d2[k] = d[k][:co]
    for k in ('res1', 'res2'):
        if k in d:
            d2[k] = np.ascontiguousarray(d[k][:n, ..., :co])
    return sub, d2


def _staged_twin(hip_lib, case, d, cfg, lay):
    """A sub-problem of `case` on which tiling `cfg` has no direct tile left over the rows / columns it keeps ragged."""
    r = CV.route(hip_lib, CV.fake_args(case, lay, False), cfg)
    hw = case.OH * case.OW
    for n in range(case.N - 1, 0, -1):
        if (n * hw) % r.bm != 0 and n * hw < r.bm:                 # one ragged row block: nothing direct
            return _sub(case, d, frames=n)
    co = case.Cout - 4 if (case.Cout - 4) % r.bn != 0 else case.Cout - 8
    return _sub(case, d, cout=co)


def _check_route(hip_lib, case, lay, cfg, want=None):
    a = CV.fake_args(case, lay, False)
    r = CV.route(hip_lib, a, cfg)
    assert r.rc == 0 and r.kernel == CONV_DMA and r.tile_cfg == cfg - CV.NUM_GENERAL, (case, cfg, r.rc, r.kernel, r.tile_cfg)
    p = CV.paths(hip_lib, case, a, cfg)
    if want is not None:
        assert want in p, (case, cfg, want, p)
    return p


def _same(a, b, what):
    assert SV.same_bits(a, b), '%s: differs in bits (max |d| = %.3e)' % (what, float(np.nanmax(np.abs(a - b))))


def _run(hip_lib, case, d, lay, cfg, what):
    rc, out = CV.launch(hip_lib, case, d, lay, CV.pack(case, d['w']), cfg, what=what)
    assert rc == 0, (what, rc)
    return out['y']


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_peeled_step_gives_the_bits_of_the_staged_paths(case, hip_lib, cuda):
    d = _data(case)
    lay = CV.layout_sets(case)['dense'][0]
    if case.relu or case.pre_relu:
        assert (d['x'] < 0).any() and (d['x'] > 0).any()
    assert 'direct' not in _check_route(hip_lib, case, lay, REF_CFG)
    ref = _run(hip_lib, case, d, lay, REF_CFG, '%s reference' % case.name)
    if case.relu:
        assert (ref == 0).any() and (ref > 0).any(), case
    ndirect = 0
    for cfg in SLICED:
        what = '%s tile_cfg %d' % (case.name, cfg)
        ndirect += 'direct' in _check_route(hip_lib, case, lay, cfg)
        _same(_run(hip_lib, case, d, lay, cfg, what), ref, what + ' against tile_cfg %d' % REF_CFG)
        sub, d2 = _staged_twin(hip_lib, case, d, cfg, lay)
        p = _check_route(hip_lib, sub, lay, cfg, want='staged_vec')
        assert 'direct' not in p or sub.Cout != case.Cout, (sub, cfg, p)     # (a column twin keeps its interior column tiles)
        got = _run(hip_lib, sub, d2, lay, cfg, what + ' staged twin')
        _same(got, ref[:sub.N, ..., :sub.Cout], what + ' staged twin %s' % sub.name)
    assert ndirect == len(SLICED), (case, ndirect)         # every tiling had direct tiles to finish


def test_a_direct_and_a_staged_tile_in_one_launch(hip_lib, cuda):
    """M = 192 with 128-row tiles: the first tile is direct, the second staged; Cout = 100 with 32-column tiles: three
    interior column tiles and an edge one."""
    by_name = {c.name: c for c in CASES}
    lay = CV.layout_sets(by_name['m192'])['dense'][0]
    for case, cfg in ((by_name['m192'], 11), (by_name['m192'], 13), (by_name['cout100'], 13), (by_name['cout100'], 16)):
        p = _check_route(hip_lib, case, lay, cfg)
        assert {'direct', 'staged_vec'} <= p, (case, cfg, p)


@pytest.mark.parametrize('name', ['bn_res1_down_relu', 'res1'])
def test_peeled_step_on_channel_slab_views(name, hip_lib, cuda):
    """Output and residuals with ld > Cout at a non-zero channel offset (CV.launch checks the canaries in the neighbouring
    channels after every launch): the bits of the dense launch."""
    case = _case('view_' + name, (2, 8, 8, 32), 96, **EPILOGUES[name])
    d = _data(case)
    sets = CV.layout_sets(case)
    ref = _run(hip_lib, case, d, sets['dense'][0], REF_CFG, case.name + ' reference')
    for cfg in (11, 13, 15, 17):
        assert 'direct' in _check_route(hip_lib, case, sets['aligned'][0], cfg)
        what = '%s aligned views tile_cfg %d' % (case.name, cfg)
        _same(_run(hip_lib, case, d, sets['aligned'][0], cfg, what), ref, what)


def test_grouped_launch_shares_the_body(hip_lib, cuda):
    """dh_conv2d_dw_group_f32 (the GEMM body beside a depthwise convolution in one launch) against its two stand-alone
    launches: 2 x 16 x 16 x 96 -> 288 behind BN + ReLU, BN + res1 epilogue."""
    from deephar_amd import _lib
    cout = 288
    case = CV.Case('group', (2, 16, 16, 96), cout, pre='bnrelu', bn=True, res1=True)
    d = _data(case)
    dwk = (np.random.default_rng(7).standard_normal((25, 96)) * 0.2).astype(np.float32)
    wt, kp, np_ = CV.pack(case, d['w'])
    dwt = torch.from_numpy(dwk).cuda()
    tx, px = SV.slab(d['x'], 96, 0, np.nan)
    tr, pr = SV.slab(d['res1'], cout, 0, np.nan)
    keep, tab = [], {}
    for n in ('pre_scale', 'pre_shift', 'post_scale', 'post_shift'):
        t, tab[n] = CV.table(d[n], False)
        keep.append(t)
    stream = torch.cuda.current_stream().cuda_stream
    outs = {}
    for which in ('group', 'single'):
        ty, py = SV.out_slab((2, 16, 16, cout), cout, 0)
        td, pd = SV.out_slab((2, 16, 16, 96), 96, 0)
        a = CV.fill_args(case, dict(x=px, y=py, res1=pr), dict(x=96, y=cout, res1=cout), wt.data_ptr(), tab)
        g = _lib.DwArgs()
        g.x, g.w, g.y, g.pre_scale, g.pre_shift = px, dwt.data_ptr(), pd, tab['pre_scale'], tab['pre_shift']
        g.N, g.H, g.W, g.C, g.ldx, g.ldy = 2, 16, 16, 96, 96, 96
        g.KH = g.KW = 5
        g.PT = g.PL = 2
        g.pre_relu, g.up_in = 1, 0
        if which == 'group':
            assert hip_lib.dh_conv2d_dw_group_f32(C.byref(a), C.byref(g), stream) == 0
        else:
            assert hip_lib.dh_conv2d_f32(C.byref(a), -1, stream) == 0
            assert hip_lib.dh_dwconv2d_f32(C.byref(g), stream) == 0
        torch.cuda.synchronize()
        outs[which] = (SV.view(ty, 0, cout), SV.view(td, 0, 96))
    _same(outs['group'][0], outs['single'][0], 'grouped launch: conv half')
    _same(outs['group'][1], outs['single'][1], 'grouped launch: depthwise half')
    ref = _run(hip_lib, case, d, CV.layout_sets(case)['dense'][0], REF_CFG, 'group reference')
    _same(outs['group'][0], ref, 'grouped launch against tile_cfg %d' % REF_CFG)
