"""Host tests (no GPU) of the geometry sweep, tests/convsweep.py: what tests/test_gpu_conv_sweep.py launches is deterministic,
reaches every kernel family and every cell the hand-picked tables lack (asked of dh_conv2d_route on fake pointers), is refused
only for listed reasons -- and the bar it holds the kernels to is one the CPU reference itself meets and a geometry mix-up does
not."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convsweep as S                               # noqa: E402
import convview as CV                               # noqa: E402

# cases that run, at least, per family (a split case counts where its bf16x3 launch runs)
MINIMA = {'general': 40, 'dma': 40, 'skinny': 40, 'halo': 12, 'split': 20, 'ext_a': 6, 'ext_b': 6}
MIN_CELL = 5
W_SPLIT_OF = {'halo': 2, 'split': 1, 'ext_a': 5, 'ext_b': 5}
KERNEL_OF = {'general': 'general', 'dma': 'dma', 'skinny': 'skinny', 'halo': 'halo', 'split': 'split', 'ext_a': 'split', 'ext_b': 'split'}


@pytest.fixture(scope='module')
def table(hip_lib):
    return S.cases(hip_lib)


def test_the_table_is_deterministic(hip_lib, table):
    again = S.generate(hip_lib)
    assert [c.key() for c in again] == [c.key() for c in table.values()]
    assert len({c.name for c in again}) == len(again) == sum(n for _, n in S.STRATA)
    for c in again:                                 # the operands too
        d0, d1 = S.data(table[c.name]), S._data.__wrapped__(c.key())
        assert sorted(d0) == sorted(d1) and all(np.array_equal(d0[k], d1[k]) for k in d0), c
        break
    for gen in (S.pool_cases, S.dw_cases, S.dws_cases):
        assert [sorted(g.__dict__.items()) for g in gen()] == [sorted(g.__dict__.items()) for g in gen()]


def test_every_case_is_a_keras_geometry(table):
    """0 <= pad < kernel extent on all four sides, extents that follow from the padding, every window starting inside the padded
    frame with at least one pixel of the frame in it; sizes at the small end of what the family runs."""
    for c in table.values():
        for size, k, s, front, behind, out in ((c.H, c.KH, c.SH, c.PT, c.PB, c.OH), (c.W, c.KW, c.SW, c.PL, c.PR, c.OW)):
            assert 0 <= front < k and 0 <= behind < k and out == (size + front + behind - k) // s + 1, c.key()
            assert (out - 1) * s - front < size and (out - 1) * s - front + k > 0 and out >= 1, c.key()
        if c.res2 == 'down':
            assert c.OH % 2 == 0 and c.OW % 2 == 0
        if c.stratum == 'skinny':
            assert c.OH <= 16 and c.OW <= 16 and c.H <= 16 and c.W <= 16
        elif c.stratum == 'halo':
            assert (c.OH, c.OW) in ((32, 32), (16, 64)) and c.Cin in (32, 48, 64)
        else:
            assert 200 <= c.M <= 2200
    for gen in (S.pool_cases, S.dws_cases):
        for g in gen():
            assert (g.OH - 1) * g.SH - g.PT < g.H and (g.OW - 1) * g.SW - g.PL < g.W and 0 <= g.PT < g.KH and 0 <= g.PL < g.KW, g
    widths = collections.Counter((g.KH, g.W) for g in S.dw_cases())
    assert set(widths) == {(k, w) for k in (1, 3, 5) for w in S.DW_WIDTHS}
    for g in S.dw_cases():
        assert 0 <= g.PT < g.KH and 0 <= g.PL < g.KW and (not g.up_in or (g.H % 2 == 0 and g.W % 2 == 0)), g
    assert [S.dw_rows(w) for w in S.DW_WIDTHS] == [8, 16, 10, 8, 8, 8]


def test_coverage_and_cells(hip_lib, table):
    ran, cells, paths, launches = collections.Counter(), collections.defaultdict(collections.Counter), set(), collections.Counter()
    for c in table.values():
        ws = W_SPLIT_OF.get(c.stratum, 0)
        rc, fam = S.family(hip_lib, c, ws)
        assert (rc == 0 and fam == KERNEL_OF[c.stratum]) or (ws == 0 and S.refusal(hip_lib, c)), (c.key(), rc, fam)
        if rc != 0:
            continue
        ran[c.stratum] += 1
        for cell, hit in c.cells().items():
            cells[c.stratum][cell] += bool(hit)
        if c.stratum == 'dma':                      # the forced tiling with TM == 1 runs, through the direct and the staged epilogue
            r = CV.route(hip_lib, S.fake_args(c), c.dcfg)
            assert r.rc == 0 and r.tm == 1 and CV.FAMILY_OF_KERNEL[r.kernel] == 'dma', (c.key(), r.rc)
            paths |= CV.paths(hip_lib, c, S.fake_args(c), c.dcfg)
        if c.stratum == 'split':                    # codes 5 / 6 / 7 run the standard kernels on a layer of the standard scope
            assert all(S.family(hip_lib, c, w) == (0, 'split') for w in (1, 3, 4, 5, 6, 7)), c.key()
            assert S.ext_class(hip_lib, c) == 0
        if c.stratum in ('ext_a', 'ext_b'):         # the standard codes refuse the layer
            assert all(S.family(hip_lib, c, w)[0] == CV.DH_EUNSUPPORTED for w in (1, 3, 4)), c.key()
            assert all(S.family(hip_lib, c, w) == (0, 'split') for w in (5, 6, 7)), c.key()
        for w, cfg in c.launches():
            launches[(c.stratum, w, S.family(hip_lib, c, w, cfg)[0])] += 1
    print()
    print('%-8s %5s  %s' % ('family', 'run', '  '.join('%s' % cell for cell in S.CELLS)))
    for s, n in S.STRATA:
        print('%-8s %2d/%2d  %s' % (s, ran[s], n, '  '.join(('%*d' % (len(cell), cells[s][cell])) if cell in S.ADMITS[s] else
                                                           ('%*s' % (len(cell), '-')) for cell in S.CELLS)))
    print('launches (family, w_split, rc): %s' % dict(sorted(launches.items())))
    for s, least in MINIMA.items():
        assert ran[s] >= least, (s, ran[s])
        for cell in S.ADMITS[s]:
            assert cells[s][cell] >= MIN_CELL, (s, cell, cells[s][cell])
    assert paths >= {'direct', 'staged_vec'}, paths
    # cells the issue names for the skinny kernel: none of them existed before
    sk = [c for c in table.values() if c.stratum == 'skinny']
    assert sum(c.KH != c.KW for c in sk) >= 20 and sum(c.SH != c.SW for c in sk) >= 15 and sum(c.nonsame for c in sk) >= 15


def test_default_launches_are_refused_for_listed_reasons_only(hip_lib, table):
    refused = collections.Counter()
    for c in table.values():
        rc, fam = S.family(hip_lib, c)
        why = S.refusal(hip_lib, c)
        assert (rc != 0) == (why is not None), (c.key(), rc, why)
        if rc != 0:
            assert rc == CV.DH_EUNSUPPORTED and why in S.DEFAULT_REFUSALS, (c.key(), rc, why)
            refused[why] += 1
    print('refused default launches: %s of %d' % (dict(refused), len(table)))
    assert 0 < sum(refused.values()) <= 0.05 * len(table)
    # a launch the library refuses is never a matter of the tiling asked for on a skinny layer, and every other refusal of the
    # sweep's launches is DH_EUNSUPPORTED as well (never DH_EINVAL: the sweep is for results, not for argument checking)
    for c in table.values():
        for ws, cfg in c.launches():
            assert S.family(hip_lib, c, ws, cfg)[0] in (0, CV.DH_EUNSUPPORTED), (c.key(), ws, cfg)


def test_the_reference_itself_meets_the_bar(table):
    """The fp32 CPU statement stays inside (K + 8) 2^-24 B on every case, the fp64 emulation E_P of each split mode inside its
    own bar on every case of a split stratum; where a ReLU is on, both signs occur."""
    worst = {}
    for c in table.values():
        d = S.data(c)
        ref, B, cpu = S.truth(c)
        S.assert_signs(c, d, ref)
        assert ref.shape == (c.N, c.OH, c.OW, c.Cout) and np.isfinite(ref).all() and (B >= np.abs(ref) * (1 - 1e-12)).all()
        r, at = S.worst(np.abs(cpu - ref), S.bound(c, B))
        worst['fp32'] = max(worst.get('fp32', (0, None)), (r, c.name))
        assert r <= 1.0, (c.key(), r, at)
        if c.stratum in ('split', 'ext_a', 'ext_b'):
            for parts in (3, 2, 1):
                ep = S.statement(c, d, torch.float64, parts=parts)
                # E_P alone against its term (the fp32 rounding of the prologue is the one thing besides: one of the + 8)
                r, at = S.worst(np.abs(ep - ref), (S.SPLIT_TERM[parts] + S.U24) * B)
                worst[parts] = max(worst.get(parts, (0, None)), (r, c.name))
                assert r <= 1.0, (c.key(), parts, r, at)
    print('worst err / bound of the references: %s' % worst)
    assert worst[1][0] > worst[2][0] * 10 or worst[1][0] > 0.05       # (the modes are not all exact: the emulation does split)


def test_geometry_mixups_leave_the_bar(table):
    """The statement with KH <-> KW, SH <-> SW, PT <-> PL, pb taken equal to pt, and zero padding applied before the BN prologue:
    each is outside the bar on every case where it is not the identity."""
    hit = collections.Counter()
    for c in table.values():
        d = S.data(c)
        ref, B, _ = S.truth(c)
        lim = S.bound(c, B, 3)                      # (the widest bar an fp32-grade launch is held to)
        for swap in S.SWAPS:
            y = S.statement(c, d, torch.float64, swap=swap)
            if y is None:
                continue
            r, at = S.worst(np.abs(y - ref), lim)
            assert r > 1.0, '%s: %s stays inside the bar (worst err / bound %.3g)' % (c.key(), swap, r)
            hit[swap] += 1
    print('mix-ups told apart: %s' % dict(hit))
    assert all(hit[s] >= 20 for s in S.SWAPS), hit


def test_depthwise_cases_reach_the_three_kernels(hip_lib):
    """Every depthwise geometry runs on the LDS-tiled kernel (k > 1: its first C - 4 channels, a multiple of 32) and on the two
    kernels beside it; the heights lie around the band of each width."""
    lds = collections.Counter()
    for g in S.dw_cases():
        assert (g.C - 4) % 32 == 0 and g.C % 4 == 0
        for kernel, less, layname in S.DW_VARIANTS:
            uses = hip_lib.dh_dwconv2d_uses_lds_kernel(C.byref(S.dw_fake_args(g, g.C - less, layname)))
            assert uses == int(kernel == 'lds' and g.KH > 1), (g, kernel, uses)
            lds[(g.KH, g.W)] += uses
    assert all(lds[(k, w)] == 5 for k in (3, 5) for w in S.DW_WIDTHS), lds
    for w in S.DW_WIDTHS:
        hs = sorted(g.H for g in S.dw_cases() if (g.KH, g.W) == (5, w))
        r = S.dw_rows(w)
        assert hs == [1, r - 1, r, r + 1, 2 * r + 3]
    ups = [g for g in S.dw_cases() if g.up_in]
    assert len(ups) >= 8 and {g.KH for g in ups} == {1, 3, 5}


def test_pool_and_depthwise_statements(table):
    """The window statements of the pooling and depthwise sweeps against brute-force loops on one case each."""
    g = S.pool_cases()[0]
    x = np.random.default_rng(0).standard_normal((g.N, g.H, g.W, 3)).astype(np.float32)
    ref = S.pool_ref(x, g)
    for oh in range(g.OH):
        for ow in range(g.OW):
            px = [x[:, r, q] for r in range(oh * g.SH - g.PT, oh * g.SH - g.PT + g.KH) for q in range(ow * g.SW - g.PL, ow * g.SW - g.PL + g.KW)
                  if 0 <= r < g.H and 0 <= q < g.W]
            want = np.max(px, axis=0) + np.min(px, axis=0) if g.mode else np.max(px, axis=0)
            assert np.array_equal(ref[:, oh, ow], want)
    g = [w for w in S.dws_cases() if w.pre == 'none'][0]
    d = S.dw_data(g)
    ref = S.dw_statement(g, d, torch.float64)
    x, w = d['x'].astype(np.float64), d['w'].astype(np.float64)
    for oh in (0, g.OH - 1):
        for ow in (0, g.OW // 2, g.OW - 1):
            acc = np.zeros((g.N, g.C))
            for kh in range(g.KH):
                for kw in range(g.KW):
                    r, q = oh * g.SH - g.PT + kh, ow * g.SW - g.PL + kw
                    if 0 <= r < g.H and 0 <= q < g.W:
                        acc += x[:, r, q] * w[kh, kw]
            assert np.allclose(ref[:, oh, ow], acc, rtol=1e-12, atol=1e-300)


def test_the_depthwise_reference_meets_its_bar():
    """(k k + 4) 2^-24 B holds for the fp32 CPU statement of every depthwise case (with the kernels' fused prologue)."""
    worst = (0.0, None)
    for g in S.dw_cases() + S.dws_cases():
        d = S.dw_data(g)
        ref, B = S.dw_statement(g, d, torch.float64), S.dw_statement(g, d, torch.float64, mag=True)
        assert ref.shape == (g.N, g.OH, g.OW, g.C)
        r, at = S.worst(np.abs(S.dw_statement(g, d, torch.float32) - ref), S.dw_bound(g, B))
        worst = max(worst, (r, g.name))
        assert r <= 1.0, (g, r, at)
    print('worst err / bound of the fp32 depthwise reference: %.3f (%s)' % worst)
