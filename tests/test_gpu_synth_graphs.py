"""Fused plans of synthetic graphs (tests/synthgraphs.py: one graph per planner guard with its near-miss twin, and seeded random
DAGs) against the fp64 graph interpreter of tests/graphref.py: under the default rules, with every switch off and with one
switch off; with the arena poisoned; across engine settings and through the C-level plan executor.

This is the fp32 leg (gemm_precision='f32').  tests/test_gpu_synth_graphs_split.py is the split-bf16 leg: the same graphs bound
under 'bf16x3' / 'bf16x2' / 'bf16' and both scopes, held to the interpreter with the mode inside (graphref.evaluate(split=...))."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphref as GR                              # noqa: E402
import paritylog                                   # noqa: E402
import synthgraphs as S                            # noqa: E402

pytestmark = pytest.mark.gpu

# one switch off must give the bits of the default plan: the rule text in engine/planner.py (R12, R4b, R10, R10b, R10c, R13, R14)
# or the rule's own test promises it; the other switches re-order fp32 sums or pick another kernel (printed, not asserted)
BIT_IDENTICAL = ('resample_on_load', 'concat_shared', 'merge_heads', 'merge_kxk', 'merge_siblings', 'merge_pools', 'pool_segments')

CASES = [(fn.__name__, fn, None, H, W, C) for fn, H, W, C in S.graphs()] + \
    [('random%d' % seed, None, seed, H, W, C) for seed in S.SEEDS for (H, W, C) in S.RANDOM_SHAPES]


def _variant(m, **opts):
    """the same graph (and weights) as a fresh Model under other engine options"""
    from deephar_amd import Model
    from deephar_amd.engine.rules import RuleSet
    v = Model(list(m.inputs), list(m.outputs), name=m.name)
    v.rules = RuleSet()
    for k, val in opts.items():
        setattr(v, k, val)
    v.executor.autotune = False                    # (every tiling gives the same bits; keeps a case to a second or two)
    return v


def _predict(m, x, n):
    outs = m.predict(x if len(x) > 1 else x[0], batch_size=n)
    return outs if isinstance(outs, list) else [outs]


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('name,fn,seed,H,W,C', CASES, ids=['%s-%dx%dx%d' % (c[0], c[3], c[4], c[5]) for c in CASES])
def test_synthetic_graph(name, fn, seed, H, W, C, hip_lib, cuda, tmp_path):
    """Measured on an MI355X (1060 comparisons): the largest |hip - o64| / bar is 0.023 (epi_chain 32 x 32 x 48)."""
    m0 = S.build(fn, H, W, C, seed=seed)
    n = 3 if H * W <= 256 else 2
    x = S.frames(m0, n)
    t64 = {}
    o64 = GR.evaluate(m0.inputs, m0.outputs, x, torch.float64, taps=t64)
    o32 = GR.evaluate(m0.inputs, m0.outputs, x, torch.float32)
    L = GR.layers_on_longest_path(m0.outputs)
    tag = '%s-%dx%dx%d' % (name, H, W, C)

    def hold(what, got, **extra):
        assert len(got) == len(o64)
        for k, t in enumerate(m0.outputs):
            label = '%s[%s].%d' % (tag, what, k)
            if GR.is_decoder_output(t):
                assert np.all(np.isfinite(got[k]))
                GR.compare_decoder(label, t, got[k], o32[k], o64[k], t64)
            else:
                GR.compare(label, got[k], o32[k], o64[k], t64, L, graph=name, rules=what, **extra)

    # 1. default rules and every switch off
    m = _variant(m0)
    base = _predict(m, x, n)
    hold('default', base)
    hold('all_off', _predict(_variant(m0, rules=S.all_off()), x, n))

    # 2. one switch off, wherever it changes this graph's step list (the executor's switches: wherever their pattern occurs)
    for k in S.switches_that_change(m0) + S.executor_switches(m.plan):
        got = _predict(_variant(m0, rules=S.one_off(k)), x, n)
        same = _same_bits(got, base)
        print('%s: %s off -> bits %s' % (tag, k, 'identical' if same else 'DIFFER'))
        hold(k + '_off', got, bits_match=same)
        if k in BIT_IDENTICAL:
            assert same, '%s off changes the bits of %s' % (k, tag)

    # 3. arena poisoning: two different finite fills, eagerly and through the captured graph
    ex = m.executor
    bp = ex.bind(n)
    for use_graph in (False, True):
        ex.use_graph = use_graph
        for fill in (2.0 ** 100, 1.0):
            bp.arena.fill_(fill)
            torch.cuda.synchronize()
            got = _predict(m, x, n)
            assert all(np.all(np.isfinite(g)) for g in got)
            assert _same_bits(got, base), '%s: arena filled with %g, %s: other bits' % (tag, fill, 'graph' if use_graph else 'eager')
    assert ex.bind(n) is bp

    # 4. engine settings: two streams, one frame alone, the C-level executor
    assert _same_bits(_predict(_variant(m0, num_streams=2, stream_policy='list'), x, n), base)
    assert _same_bits(_predict(m, [a[:1] for a in x], 1), [b[:1] for b in base])
    path = str(tmp_path / 'synth.dhplan')
    m.export_plan(path, n)
    blob = open(path, 'rb').read()
    plan = ctypes.c_void_p()
    assert hip_lib.dh_plan_create(blob, len(blob), ctypes.byref(plan)) == 0
    try:
        xd = [torch.from_numpy(a).to(cuda) for a in x]
        outs = [torch.full(r.shape, float('nan'), device=cuda) for r in base]
        ins_p = (ctypes.c_void_p * len(xd))(*[a.data_ptr() for a in xd])
        outs_p = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        assert hip_lib.dh_forward(plan, ins_p, n, outs_p, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert _same_bits([o.cpu().numpy() for o in outs], base)
    finally:
        assert hip_lib.dh_plan_destroy(plan) == 0
