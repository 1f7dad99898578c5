"""Everything about the synthetic-graph tests that can be proven without a GPU: the fp64 graph interpreter of tests/graphref.py
equals the hand-written oracles; every graph of tests/synthgraphs.py triggers the planner rule it exists for and its near-miss
twin does not; the bar of graphref.compare fails when any shape-preserving node of any zoo graph is skipped; the generator's
graphs are plannable."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphref as GR                              # noqa: E402
import resample_ref as R                           # noqa: E402
import synthgraphs as S                            # noqa: E402

from deephar_amd import graph, weights             # noqa: E402
from deephar_amd.engine.planner import build_plan  # noqa: E402
from deephar_amd.engine.rules import RuleSet       # noqa: E402

PLANNER_RULES, switches_that_change = S.PLANNER_RULES, S.switches_that_change


# ---- 1. the interpreter against the hand-written oracles ---------------------------------------------------------------
def _reception(dim):
    from deephar_amd.models import reception
    from oracle import reception as oref
    graph.reset_naming()
    kw = dict(num_blocks=2, ksize=(5, 5), concat_pose_confidence=True)
    kw.update(dict(num_context_per_joint=2) if dim == 2 else dict(depth_maps=16))
    m = reception.build((256, 256, 3), 16, dim=dim, **kw)
    weights.init_synthetic(m, seed=0)
    x = np.random.default_rng(0).uniform(-1, 1, (1, 256, 256, 3)).astype(np.float32)
    return m, x, oref.forward(weights.as_dict(m), x, 16, dim, dtype=torch.float64, **kw)


def _mini():
    m, wd = R.build_mini_pyramid()
    x = np.random.default_rng(21).standard_normal((2, 16, 16, 96)).astype(np.float32)
    return m, x, [R.mini_pyramid(wd, x, dtype=torch.float64)]


def _spnet():
    from deephar_amd import utils
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import spnet
    from oracle import spnet as osp
    graph.reset_naming()
    m = spnet.build(ModelConfig((128, 128, 3), utils.pa16j2d, num_actions=[], num_pyramids=2, action_pyramids=[]))
    weights.init_synthetic(m, seed=0)
    ocfg = dict(num_joints=16, dim=2, num_actions=[], num_pyramids=2, action_pyramids=[], num_levels=4, kernel_size=(5, 5),
                growth=96, image_div=8, num_pose_features=0, num_visual_features=0, sam_alpha=1)
    x = np.random.default_rng(3).uniform(-1, 1, (1, 128, 128, 3)).astype(np.float32)
    return m, x, osp.forward(weights.as_dict(m), x, ocfg, dtype=torch.float64)


@pytest.mark.parametrize('which', ['reception_2d_context', 'reception_3d_16_depth_maps', 'mini_pyramid', 'spnet_128_pose_only'])
def test_interpreter_equals_the_hand_written_oracle(which):
    """evaluate(..., float64) walks the graph node by node; the oracle is the model's forward written out by hand.  Both use
    the statements of oracle/ops.py in the same order, so they agree to rounding of nothing at all: <= 1e-12."""
    m, x, ref = {'reception_2d_context': lambda: _reception(2), 'reception_3d_16_depth_maps': lambda: _reception(3),
                 'mini_pyramid': _mini, 'spnet_128_pose_only': _spnet}[which]()
    got = GR.evaluate(m.inputs, m.outputs, [x], torch.float64)
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        d = float(np.abs(g - r.reshape(g.shape)).max())
        print('%s output %d: max |interpreter - oracle| = %.1e' % (which, k, d))
        assert d <= 1e-12


def test_layers_on_longest_path():
    m, _, _ = _mini()
    assert GR.layers_on_longest_path(m.outputs) == R.MINI_LAYERS == 9
    m = S.build(S.add4, 16, 16, 48)
    assert GR.layers_on_longest_path(m.outputs) == 2          # the separable convolution; the other operands cross one layer


# ---- 2. rule coverage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.ZOO, ids=lambda c: '%s-%s' % (c.name, c.feature))
def test_rule_coverage(case):
    """the default plan of every zoo graph shows the feature the graph exists for, at every shape where the guard holds, and
    does not show it in the near-miss twin (or at the shapes where the guard fails)"""
    for (H, W, C) in case.shapes:
        m = S.build(case.fn, H, W, C)
        plan = build_plan(m.inputs, m.outputs, rules=RuleSet())
        got, want = bool(S.FEATURES[case.feature](plan)), bool(case.expected(H, W, C))
        print('%-26s %-12s %-24s %s' % (case.name, (H, W, C), case.feature, 'yes' if got else 'no'))
        assert got == want, '%s at %s: %s is %s, expected %s\n%s' % (case.name, (H, W, C), case.feature, got, want,
                                                                     '\n'.join(S.describe(plan)))


def test_every_planner_switch_changes_some_zoo_plan():
    """(the three executor switches -- halo_conv, group_launches, pair_convs -- act when a plan is bound, on the GPU: the step list
    cannot show them; tests/test_gpu_synth_graphs.py runs them wherever synthgraphs.executor_switches finds their pattern)"""
    hit = {k: [] for k in PLANNER_RULES}
    for fn, H, W, C in S.graphs():
        m = S.build(fn, H, W, C)
        for k in switches_that_change(m):
            hit[k].append('%s%s' % (fn.__name__, (H, W, C)))
        assert S.describe(build_plan(m.inputs, m.outputs, rules=S.all_off()))      # plannable with every switch off
    for k, where in hit.items():
        print('%-18s %d graphs, e.g. %s' % (k, len(where), where[:2]))
    assert not [k for k, where in hit.items() if not where]


# ---- 3. the bar has teeth --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fn', sorted({c.fn for c in S.ZOO}, key=lambda f: f.__name__), ids=lambda f: f.__name__)
def test_skipping_any_node_breaks_the_bar(fn):
    """fp32 interpreter with one BatchNormalization / ReLU / scale / sigmoid / add turned into the identity, held to the fp64
    interpreter of the intact graph through graphref.compare: it must fail on some feature-map output, for every such node."""
    for (f, H, W, C) in S.graphs():
        if f is not fn:
            continue
        m = S.build(fn, H, W, C)
        x = S.frames(m, 2)
        t64 = {}
        o64 = GR.evaluate(m.inputs, m.outputs, x, torch.float64, taps=t64)
        o32 = GR.evaluate(m.inputs, m.outputs, x, torch.float32)
        L = GR.layers_on_longest_path(m.outputs)
        fmaps = [k for k, t in enumerate(m.outputs) if not GR.is_decoder_output(t)]
        for k in fmaps:                                   # the intact fp32 evaluation passes
            GR.compare('intact', o32[k], o32[k], o64[k], t64, L, log=False)
        nodes = [n for n in m._nodes if n.op in GR.SKIPPABLE]       # (a few graphs -- bare convolutions -- have none)
        for node in nodes:
            bad = GR.evaluate(m.inputs, m.outputs, x, torch.float32, skip=node)
            caught = 0
            for k in fmaps:
                try:
                    GR.compare('skip', bad[k], o32[k], o64[k], t64, L, log=False)
                except AssertionError:
                    caught += 1
            assert caught, '%s%s: skipping %r (%s) goes unnoticed' % (fn.__name__, (H, W, C), node, node.name)


# ---- 4. the generator ------------------------------------------------------------------------------------------------------
def test_generator_graphs_are_plannable():
    assert len(S.SEEDS) == len(set(S.SEEDS)) == 12
    differ = 0
    for seed in S.SEEDS:
        for (H, W, C) in S.RANDOM_SHAPES:
            m = S.build(None, H, W, C, seed=seed)
            ops_ = [n.op for n in m._nodes]
            assert 8 <= len(ops_) <= 14 and 1 <= len(m.outputs) <= 3
            a = S.describe(build_plan(m.inputs, m.outputs, rules=RuleSet()))
            b = S.describe(build_plan(m.inputs, m.outputs, rules=S.all_off()))
            differ += a != b
            print('seed %3d %s: %s%s' % (seed, (H, W, C), ' '.join(ops_), '   [plans differ]' if a != b else ''))
            again = S.build(None, H, W, C, seed=seed)
            assert [n.op for n in again._nodes] == ops_                # a seed is a graph
    assert 2 * differ >= 2 * len(S.SEEDS)


# ---- 5. guards the synthetic graphs found wrong, pinned ---------------------------------------------------------------------
def _kinds(m, rules=None):
    return [(s.kind, s.name) for s in build_plan(m.inputs, m.outputs, rules=rules or RuleSet()).steps]


def test_up2_epilogue_needs_an_aligned_input():
    """R3's fallback -- the low-resolution convolution writes at 2x resolution (dh_conv_args.up2) -- asked the MFMA kernels for
    an input of 34 channels; they load 16 bytes at a time (up_res at 16 x 16 x 34, and at 32 x 32 x 34 with res2_down off:
    'configuration not supported').  Such a convolution is followed by a stand-alone upsample_add now."""
    for shape, rules in (((16, 16, 34), RuleSet()), ((32, 32, 34), S.one_off('res2_down'))):
        m = S.build(S.up_res, *shape)
        plan = build_plan(m.inputs, m.outputs, rules=rules)
        assert [(s.kind, s.name) for s in plan.steps] == [('conv', 'a_conv'), ('pool', 'pool'), ('conv', 'lo'),
                                                           ('upsample_add', 'upsample_add')]
        assert not any(s.attrs.get('up2') for s in plan.steps) and set(plan.steps[-1].ins) == {'a', 'b'}
    m = S.build(S.up_res, 16, 16, 48)                  # aligned: the epilogue form, as before
    assert _kinds(m) == [('conv', 'a_conv'), ('pool', 'pool'), ('conv', 'lo')]


def test_kxk_siblings_do_not_merge_on_the_skinny_kernel():
    """R10b promises the bits of the separate convolutions.  On the skinny-conv kernel every wave sums a contiguous run of K
    and the runs follow from K: inside the 3x5 window the 3x1 part's products fall into other runs (kxk_siblings at
    4 x 16 x 40, K = 120 | 360 | 600: merge_heads off changed the bits).  The rule stays on the general kernel."""
    m = S.build(S.kxk_siblings, 4, 16, 40)
    assert _kinds(m) == [('conv', 'k31'), ('conv', 'k33'), ('conv', 'k35')]
    m = S.build(S.kxk_siblings, 32, 32, 40)            # 1024 pixels: the general kernel
    plan = build_plan(m.inputs, m.outputs, rules=RuleSet())
    assert [(s.kind, s.name, s.attrs['kh'], s.attrs['kw'], s.attrs['Cout']) for s in plan.steps] == \
        [('conv', 'k31+k33+k35', 3, 5, 49)]


def test_kxk_siblings_merge_only_where_the_taps_keep_their_places():
    """The general kernel walks every eight k of a K-step as 0, 4, 1, 5, 2, 6, 3, 7 (conv_igemm.hip): with Cin = 4 a 3x1 kernel's
    taps fall on other places of that chain inside a 3x5 window than in its own launch, and merge_heads off moved the bits of
    kxk_siblings at 4 x 16 x 4; with Cin = 40 (a multiple of eight) every tap keeps its place."""
    from deephar_amd.engine.planner import kxk_window_keeps_k_order as keeps
    assert not keeps(3, 1, 3, 5, 4) and not keeps(3, 3, 3, 5, 4)
    assert keeps(3, 1, 3, 5, 40) and keeps(3, 3, 3, 5, 40) and keeps(3, 5, 3, 5, 4)
    assert not keeps(3, 1, 3, 5, 34) and not keeps(3, 3, 3, 5, 34)
    for shape in ((4, 16, 4), (32, 32, 34)):
        assert _kinds(S.build(S.kxk_siblings, *shape)) == [('conv', 'k31'), ('conv', 'k33'), ('conv', 'k35')]
    # the action heads' masked pose (Cin = 2, 3) merges as tests/test_gpu_models.py measures it: bit-identical
    plan = build_plan(*(lambda m: (m.inputs, m.outputs))(S.build(S.kxk_siblings, 8, 16, 3)), rules=RuleSet())
    assert [s.name for s in plan.steps] == ['k31+k33+k35']


def test_conv2dtranspose_of_unaligned_channels_fails_at_plan_time():
    """the transposed-convolution kernel takes multiples of four input channels: a plan-time error, not one at the first predict"""
    from deephar_amd import Model, layers as L
    graph.reset_naming()
    x = L.Input((8, 8, 50))
    m = Model(x, L.conv2dtranspose(x, 34, (2, 2), strides=(2, 2)))
    with pytest.raises(NotImplementedError, match='multiples of four'):
        build_plan(m.inputs, m.outputs, rules=RuleSet())
