"""Host tests (no GPU) that go with tests/test_gpu_conv_views.py, on fake pointers of the intended alignment and by the library's
own answers (dh_conv2d_route and the exported rules; nothing of the launcher is restated): every case of tests/convview.py
reaches the kernel family it is there for, every launch of the tables is refused exactly where convview.refusal says, and
the case tables reach every form of the A load, the epilogue, the half-resolution residual and the pooled output."""
import ctypes as C
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convview as CV                              # noqa: E402
import slabview as SV                              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launches():
    for case in CV.CASES.values():
        for sname, (lay, tabs) in CV.layout_sets(case).items():
            yield case, sname, lay, tabs, CV.fake_args(case, lay, tabs)


def _dma_shape(hip_lib, case, a):
    """gemm1x1_eligible is not exported; dh_conv2d_split_eligible is that rule plus 'no BN prologue, not skinny'."""
    from deephar_amd import _lib
    b = _lib.ConvArgs.from_buffer_copy(a)
    b.pre_scale = b.pre_shift = None
    return hip_lib.dh_conv2d_split_eligible(C.byref(b))


def test_every_case_reaches_its_family(hip_lib):
    seen, calls = set(), {0: 0, CV.DH_EUNSUPPORTED: 0}
    for case, sname, lay, tabs, a in _launches():
        what = (case.name, sname)
        for cfg in case.cfgs:
            # the refusal table, asked of the library: DH_EUNSUPPORTED for every listed refusal, and a route of the case's family
            # for everything else.  The exceptions are those of test_gpu_conv_views.test_conv2d_on_views: the 13 x 11 split
            # cases (a skinny layer by the shape rule: refused on every layout) and the wide tilings below three parts
            r = CV.route(hip_lib, a, cfg)
            want = CV.DH_EUNSUPPORTED if CV.refused_by_shape(case, cfg) or CV.refusal(case, lay, tabs, cfg) else 0
            assert r.rc == want, (what, cfg, r.rc)
            calls[r.rc] += 1
            if r.rc == 0:
                fam = case.family_of(cfg)
                if fam == 'auto':                            # the library's own pick: the DMA GEMM unless x is misaligned
                    fam = 'general' if lay['x'] == 'odd' else 'dma'
                assert CV.FAMILY_OF_KERNEL[r.kernel] == fam, (what, cfg, r.kernel)
        skinny = hip_lib.dh_conv2d_uses_split_k(C.byref(a))
        stem = hip_lib.dh_conv2d_uses_first_layer_kernel(C.byref(a))
        x_ok = int(lay['x'] != 'odd')
        seen.add(case.family)
        if case.family == 'skinny':                          # a rule on the geometry: every layout, every tile_cfg
            assert skinny == 1 and stem == 0, what
        elif case.family == 'stem':
            assert (skinny, stem) == (0, 1) and a.ldx == 3, what
        elif case.family == 'halo':
            assert (skinny, stem) == (0, 0) and hip_lib.dh_conv2d_halo_eligible(C.byref(a)) == x_ok, what
            assert (CV.refusal(case, lay, tabs, 0) is not None) == (not x_ok), what
        elif case.family == 'split':
            # the 13 x 11 K x K shape is a skinny layer by the shape rule: the split modes refuse it on every layout
            want = 0 if '13x11' in case.name else x_ok
            assert (skinny, stem) == (0, 0) and hip_lib.dh_conv2d_split_eligible(C.byref(a)) == want, what
            assert (CV.refusal(case, lay, tabs, 0) is not None) == (not x_ok), what
        else:
            # (e) and (g) would quietly become skinny layers with K >= 64; (k)'s geometry must not be met by accident
            assert (skinny, stem) == (0, 0), what
            if any(c < 0 or c >= CV.NUM_GENERAL for c in case.cfgs):
                assert _dma_shape(hip_lib, case, a) == x_ok, what
    assert seen == {'fp32', 'halo', 'split', 'skinny', 'stem'}
    assert calls == {0: 1214, CV.DH_EUNSUPPORTED: 672}, calls              # 1886 launches of the tables
    # the shape (c) / (i) name for K x K on the DMA GEMM: 143 positions, K = 576, 72 channels -- a skinny layer
    from deephar_amd.engine.planner import split_k_rule
    assert split_k_rule(13 * 11, 576, 72, 64) and not split_k_rule(35 * 33, 576, 72, 64) and not split_k_rule(18 * 17, 576, 72, 64)


def test_transposed_conv_cases_are_eligible_on_an_aligned_x_only(hip_lib):
    from deephar_amd import _lib
    for cout in CV.CONVT_COUTS:
        n, h, w, cin = CV.CONVT_SHAPE
        for name, want in (('aligned', 1), ('odd', 0)):
            ld, off = SV.layout(cin, name, 0)
            a = _lib.ConvtArgs()
            a.x, a.w, a.y = 0x100000 + 4 * off, 0x200000, 0x300000
            a.N, a.H, a.W, a.Cin, a.ldx, a.Cout, a.ldy = n, h, w, cin, ld, cout, cout
            a.Kp, a.Np = 32, (4 * cout + 31) // 32 * 32
            assert off > 0 and hip_lib.dh_conv2d_transpose2x2_split_eligible(C.byref(a)) == want, (cout, name)


def test_no_source_includes_a_source_and_the_split_tilings_stand_once():
    """The kernel sources share code through headers only, and the split-bf16 tilings -- stated once, in gemm_family.h, for the
    standard and the extended scope -- are the ones the benchmark names its kernels by."""
    csrc = os.path.join(ROOT, 'deephar_amd', 'csrc')
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    for fname, text in texts.items():
        assert not re.search(r'#\s*include\s*["<][^">]*\.hip[">]', text), '%s includes a source' % fname
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    # a row of kGemmTiles: `{wm, wn, tm, tn, ns},  // cfg: ...`; the wide tilings end in `true` and spell their 192 columns as tn = 6
    row = r'\{(\d+), (\d+), (\d+), (\d+), (\d+)(, true)?\},\s*//\s*(\d+):'
    found = re.findall(row, texts['gemm_family.h'])
    tiles = {int(c): (tuple(int(v) for v in t[:4]), int(t[4])) for *t, w, c in found if not w}
    wide = {int(c): int(t[0]) for *t, w, c in found if w}
    assert all(tuple(t[1:]) == ('1', '1', '6', '2') for *t, w, c in found if w)
    assert tiles == bench.SPLIT_TILES and wide == bench.SPLIT_WIDE
    assert sorted(tiles) + sorted(wide) == list(range(16)) and [int(c) for *_, c in found] == list(range(16))
    # nowhere else, and none twice: no other table row, and no tiling spelled out as template arguments of a launch
    rows = [(f, m) for f, text in texts.items() for m in re.findall(row, text)]
    assert len(rows) == 16 and all(f == 'gemm_family.h' for f, _ in rows), rows
    spelled = [(f, m) for f, text in texts.items() for m in re.findall(r'(?:launch_cfg|launch_ext_cfg|Tile)<[\d, ]+>', text)]
    assert not spelled, spelled


def _epi_and_gather(hip_lib, case, a):
    """(16-byte epilogue, float4 A gather) of a struct as the library's routes say: over the case's tilings and, for the fp32
    family, the general kernel's 128 x 64 (the only kernel with a scalar gather).  Each is the one value all accepted routes
    agree on, None where no kernel with that choice accepts the struct."""
    cfgs = set(case.cfgs) | ({3} if case.family == 'fp32' else set())
    routes = [r for r in (CV.route(hip_lib, a, c) for c in sorted(cfgs)) if r.rc == 0]
    es = {r.epi & 1 for r in routes if CV.FAMILY_OF_KERNEL[r.kernel] in ('general', 'dma', 'split', 'halo')}
    vs = {r.vec4 for r in routes if CV.FAMILY_OF_KERNEL[r.kernel] == 'general'}
    assert len(es) <= 1 and len(vs) <= 1, (case.name, es, vs)
    return (es.pop() if es else None), (vs.pop() if vs else None)


def test_case_tables_reach_every_path_of_the_launcher(hip_lib):
    reached, per = set(), {}
    for case, sname, lay, tabs, a in _launches():
        e, v = _epi_and_gather(hip_lib, case, a)
        if case.family == 'fp32' and not case.up2 and not (case.pool and CV.refusal(case, lay, tabs, 3)):
            assert e is not None and v is not None, (case.name, sname)        # (the general kernel takes every layout)
        # a single misaligned operand is enough to send the whole epilogue / the whole gather scalar
        if sname in ('odd_y', 'odd_res1', 'odd_res2') or (sname == 'tables' and case.bn):
            assert e in (0, None), (case.name, sname)
        if sname == 'odd_x' or (sname == 'tables' and case.pre_bn):
            assert v in (0, None), (case.name, sname)
        if sname in ('dense', 'aligned') and case.Cout % 4 == 0:
            assert e in (1, None) and (v in (1, None) or case.Cin % 4 != 0 or case.x_u8), (case.name, sname)
        if sname == 'odd_y_pool':
            assert all(CV.refusal(case, lay, tabs, c) for c in case.cfgs), case.name
        if case.family not in ('fp32', 'halo', 'split'):
            continue
        for cfg in case.cfgs:
            if cfg < 0 or CV.refusal(case, lay, tabs, cfg) or CV.refused_by_shape(case, cfg):
                continue
            p = CV.paths(hip_lib, case, a, cfg)
            per[(case.name, sname, cfg)] = p
            reached |= p
    assert reached >= {'vec4', 'scalar_a', 'staged_vec', 'staged_scalar', 'direct', 'down_direct', 'down_staged_div',
                       'down_scalar', 'pool_pair', 'pool_in_wave'}, reached
    # (a) aligned = VEC4 + the 16-byte staged epilogue, odd = scalar gather + scalar epilogue
    for name in ('a_general_1x1', 'a_general_3x3'):
        for cfg in (3, 8):
            assert per[(name, 'aligned', cfg)] == {'vec4', 'staged_vec'} and per[(name, 'odd', cfg)] == {'scalar_a', 'staged_scalar'}
    # (b) tile_cfg 12: direct on the 6 x 3 interior tiles, staged on the ragged ones; 10 (TM = 2) has no prefetch: staged
    c = CV.CASES['b_dma']
    r = CV.route(hip_lib, CV.fake_args(c, *CV.layout_sets(c)['aligned']), 12)
    assert (r.bm, r.bn, r.tm) == (128, 64, 1) and c.M // 128 == 6 and c.Cout // 64 == 3 and c.M % 128 and c.Cout % 64
    assert per[('b_dma', 'aligned', 12)] == {'direct', 'staged_vec'} and per[('b_dma', 'aligned', 10)] == {'staged_vec'}
    assert per[('b_dma', 'odd_res1', 12)] == {'staged_scalar'} and per[('b_dma', 'tables', 12)] == {'staged_scalar'}
    # (e) the power-of-two direct form on every tile | the staged form with integer divides
    for cfg in (13, 16):
        assert per[('e_down_pow2', 'aligned', cfg)] == {'direct', 'down_direct'}
        assert per[('e_down_div', 'aligned', cfg)] == {'staged_vec', 'down_staged_div'}
        assert per[('e_down_pow2', 'odd_res2', cfg)] == {'staged_scalar', 'down_scalar'}
    # (f) two full-resolution residuals never store direct; (d) nor does the up-sampling epilogue
    assert 'direct' not in per[('f_two_residuals', 'aligned', 13)] and 'direct' not in per[('d_up2', 'aligned', 11)]
    # (g) wave pair at OW = 32, in-wave below
    assert 'pool_pair' in per[('g_pool_32', 'aligned', 12)] and 'pool_pair' in per[('g_pool_32', 'aligned', 3)]
    assert 'pool_in_wave' in per[('g_pool_16', 'aligned', 12)] and 'pool_in_wave' in per[('g_pool_8', 'aligned', 17)]
    # (h) the halo kernel: direct on every tile of the 32-column tiling that lies inside Cout, scalar at Cout = 70
    assert per[('h_halo_72', 'aligned', 0)] == {'direct', 'staged_vec'} and per[('h_halo_72', 'aligned', 2)] == {'staged_vec'}
    assert per[('h_halo_70', 'aligned', 0)] == {'staged_scalar'}


def test_operand_layouts_of_a_launch_are_pairwise_distinct():
    for case in CV.CASES.values():
        for name in ('aligned', 'odd'):
            ls = [CV.layout_of(case, o, name) for o in case.operands()]
            assert len(set(ls)) == len(ls), (case.name, name, ls)
            assert len({l[0] for l in ls}) == len(ls) and len({l[1] for l in ls}) == len(ls), (case.name, name, ls)
        for o in case.operands():
            ch = case.shape_of(o)[-1]
            assert CV.layout_of(case, o, 'dense') == (ch, 0)
            ld, off = CV.layout_of(case, o, 'aligned')
            assert ld % 4 == 0 and off % 4 == 0 and off > 0 and off + ch <= ld
            ld, off = CV.layout_of(case, o, 'odd')
            assert ld % 2 == 1 and off % 2 == 1 and off + ch <= ld
        for sname, (lay, tabs) in CV.layout_sets(case).items():
            if sname.startswith('odd_'):
                assert [o for o in lay if lay[o] == 'odd'] == [sname[4:]] and not tabs, (case.name, sname)
            if sname == 'tables':
                a = CV.fake_args(case, lay, tabs)
                assert all((getattr(a, n) or 4) % 16 == 4 for n in ('pre_scale', 'pre_shift', 'post_scale', 'post_shift'))
    assert CV.LOUD == float(2 ** 100) and CV.CASES['b_dma_ktail'].fill == CV.LOUD and CV.CASES['i_split1_pw_ktail'].fill == CV.LOUD
    import numpy as np
    assert all(np.isnan(c.fill) for c in CV.CASES.values() if c.Cin % 32 == 0 or c.family in ('halo', 'skinny', 'stem'))


def test_every_listed_refusal_occurs():
    """(m): the case tables contain each refusal of the list at least once (the launches themselves, with the exact return
    code and the untouched output slabs, are part of test_gpu_conv_views.test_conv2d_on_views; an odd x of a
    transposed convolution is refused in test_transposed_conv_on_views)."""
    seen = set()
    for case in CV.CASES.values():
        for sname, (lay, tabs) in CV.layout_sets(case).items():
            for cfg in case.cfgs:
                why = CV.refusal(case, lay, tabs, cfg)
                if why:
                    seen.add((why, sname if case.pool else ''))
    reasons = {w for w, _ in seen}
    assert len(reasons) == 5, reasons
    assert {s for w, s in seen if 'pooled' in w} >= {'odd', 'odd_y', 'odd_y_pool', 'odd_res1', 'tables'}
