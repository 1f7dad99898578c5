"""The split-bf16 ladder on the synthetic graphs of tests/synthgraphs.py, as far as it can be proven without a GPU.

1. Classification.  For every graph of the split leg the default plan's conv / convtranspose steps are put to the LIBRARY's
   rules (dh_conv2d_split_eligible, dh_conv2d_split_wide_eligible, dh_conv2d_transpose2x2_split_eligible) with the launch
   struct the engine's own binder fills (engine/binding.py) on its fake arena (`classify`).  tests/test_gpu_synth_graphs_split.py imports the
   table and holds the bound plan to it step by step.
2. Coverage.  `COVERAGE` lists the (layer class, plan feature) pairs the split leg must meet on at least one (graph, shape).
3. The twin.  The slice readers of slice_reader_odd are refused under every mode and scope, its sibling's are taken.
4. The clauses of the GPU test (`hold_mode`) hold for the reference alone -- evaluate(float32, split=...) as a stand-in for
   the engine -- and bite: the stand-in of the next rung down fails the upper rung's clauses, a skipped epilogue node fails
   the loosest one.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphref as GR                              # noqa: E402
import synthgraphs as S                            # noqa: E402

from deephar_amd.engine import binding            # noqa: E402
from deephar_amd.engine.packing import LAYOUT_CODES as CODES, MODE_PARTS as PARTS    # noqa: E402
from deephar_amd.engine.planner import build_plan  # noqa: E402
from deephar_amd.engine.rules import RuleSet       # noqa: E402

MODES = ('bf16x3', 'bf16x2', 'bf16')
CONVT_CODES = CODES['standard']                    # (a transposed convolution has one rule and one set of codes)
STD_PW, STD_KXK, EXT_KXK, EXT_BNPW, CONVT = 'standard pointwise', 'standard KxK', 'extended KxK', 'extended BN-pointwise', 'transposed'
ADDED = (EXT_KXK, EXT_BNPW)                        # the classes only gemm_scope='extended' reaches


def batch(H, W):
    """the batch size of a case, as tests/test_gpu_synth_graphs.py picks it"""
    return 3 if H * W <= 256 else 2


# ---- 1. classification -----------------------------------------------------------------------------------------------------
def features(s):
    """what a split layer meets in its fused step (the names of COVERAGE)"""
    a, x, y = s.attrs, s.ins['x'], s.outs['y']
    f = set()
    r1, r2 = s.ins.get('res1') is not None, s.ins.get('res2') is not None
    if s.kind == 'convtranspose':
        if 'pre_bn' in s.params and r1:
            f.add('pre_bn+residual')
        return f
    post_bn = 'post_bn' in s.params or 'post_affine' in s.params
    if post_bn:
        f.add('post_bn')
    if a.get('post_relu'):
        f.add('post_relu')
    if post_bn and a.get('post_relu'):
        f.add('post_bn+post_relu')
    if a.get('pre_relu'):
        f.add('pre_relu')
    if a.get('res2_down'):
        f.add('res2_down')
    elif r1 and r2:
        f.add('res1+res2')
    elif r1:
        f.add('res1')
    if a.get('up2'):
        f.add('up2')
    if s.outs.get('ypool') is not None:
        f.add('ypool')
    if y.coff != 0 or y.ld != y.C:
        f.add('y_view')
    if x.coff != 0 or x.ld != x.C:
        f.add('x_view')
    if hasattr(s.params['w'], 'parts'):
        f.add('merged')
    return f


def classify(lib, plan, n):
    """One row per step of `plan` bound for n frames: None for a step that is no convolution, else a dict with the library's
    answers (`std`, `wide`), the layer class (`cls`: None where the layer stays fp32 under both scopes) and its features."""
    rows, env = [], binding.FakeEnv(n)
    for s in plan.steps:
        if s.kind == 'conv':
            args = binding.bind(s, n, env)[1][0]
            std, wide = lib.dh_conv2d_split_eligible(C.byref(args)), lib.dh_conv2d_split_wide_eligible(C.byref(args))
            assert wide >= std
            pw = s.attrs['kh'] == 1 and s.attrs['kw'] == 1
            cls = (STD_PW if pw else STD_KXK) if std else ((EXT_BNPW if 'pre_bn' in s.params else EXT_KXK) if wide else None)
            assert cls != EXT_BNPW or pw
        elif s.kind == 'convtranspose':
            std = wide = lib.dh_conv2d_transpose2x2_split_eligible(C.byref(binding.bind(s, n, env)[1][0]))
            cls = CONVT if std else None
        else:
            rows.append(None)
            continue
        rows.append(dict(step=s, kind=s.kind, name=s.name, std=int(std), wide=int(wide), cls=cls, features=features(s)))
    return rows


def expected_code(row, mode, scope):
    """the w_split a row's step must be bound with under (mode, scope); None: an fp32 packing (0, or 2 for the halo kernel)"""
    if row['kind'] == 'convtranspose':
        return CONVT_CODES[mode] if row['std'] else None
    return CODES[scope][mode] if row['wide' if scope == 'extended' else 'std'] else None


def table_param_ids(rows, scope, only=None):
    """the ids of the weight Params the table says run split under `scope` (graphref.split_param_ids for a bound plan);
    only=<class>: of the layers of that class alone"""
    ids = set()
    for r in rows:
        if r is not None and r['wide' if scope == 'extended' else 'std'] and only in (None, r['cls']):
            w = r['step'].params['w']
            ids.update(id(p) for p in getattr(w, 'parts', [w]))
    return ids


def classes(rows, scope='extended'):
    return {r['cls'] for r in rows if r is not None and r['cls'] and (scope == 'extended' or r['cls'] not in ADDED)}


def cases():
    """(name, fn, seed, H, W, C) of the split leg: the zoo at SPLIT_SHAPES, the random seeds at SPLIT_RANDOM_SHAPES"""
    return [(fn.__name__, fn, None, H, W, C) for fn, H, W, C in S.split_graphs()] + \
        [('random%d' % seed, None, seed, H, W, C) for seed in S.SEEDS for (H, W, C) in S.SPLIT_RANDOM_SHAPES]


def unaligned_cases():
    return [(fn.__name__, fn, None, H, W, C) for fn, H, W, C in S.split_graphs((S.UNALIGNED_SHAPE,))]


def default_table(lib, m, H, W, rules=None):
    return classify(lib, build_plan(m.inputs, m.outputs, rules=rules or RuleSet()), batch(H, W))


# (32, 32, 34): the graphs in which the library takes a layer all the same -- the 1x1 convolution behind a concatenation of
# 17 + 34 + 17 channels, the BN-prologue pointwise layers of 68 and 48 channels (under gemm_scope='extended' only), and the
# transposed convolution of (34 + 16) // 4 * 4 = 48 channels.  Everywhere else at this shape a split mode is the fp32 plan.
UNALIGNED = {'cat_nested': {STD_PW}, 'cat_twice': {STD_PW}, 'siblings': {EXT_BNPW}, 'siblings_output': {EXT_BNPW},
             'learned_resample': {CONVT}, 'learned_resample_bn_twice': {CONVT, EXT_BNPW}}

COVERAGE = (
    (STD_PW, 'post_bn'), (STD_PW, 'res1'), (STD_PW, 'res1+res2'), (STD_PW, 'res2_down'), (STD_PW, 'up2'), (STD_PW, 'ypool'),
    (STD_PW, 'y_view'), (STD_PW, 'x_view'),
    (STD_KXK, 'post_bn+post_relu'), (STD_KXK, 'res1'), (STD_KXK, 'res1+res2'), (STD_KXK, 'res2_down'), (STD_KXK, 'ypool'),
    (STD_KXK, 'y_view'), (STD_KXK, 'x_view'),
    (EXT_KXK, 'post_bn'), (EXT_KXK, 'res1'), (EXT_KXK, 'res1+res2'), (EXT_KXK, 'res2_down'), (EXT_KXK, 'y_view'),
    (EXT_BNPW, 'pre_relu'), (EXT_BNPW, 'post_bn'), (EXT_BNPW, 'post_relu'), (EXT_BNPW, 'merged'), (EXT_BNPW, 'y_view'),
    (CONVT, 'pre_bn+residual'),
)


@pytest.fixture(scope='module')
def tables(hip_lib):
    """{(name, H, W, C): rows} of every case of the split leg, the unaligned shape included"""
    out = {}
    for name, fn, seed, H, W, C in cases() + unaligned_cases():
        out[(name, H, W, C)] = default_table(hip_lib, S.build(fn, H, W, C, seed=seed), H, W)
    return out


def test_classification_and_coverage(tables):
    """every (class, feature) pair of COVERAGE is met by a split layer of some (graph, shape) of the split leg"""
    met = {}
    for (name, H, W, C), rows in tables.items():
        if (H, W, C) == S.UNALIGNED_SHAPE:
            continue
        for r in rows:
            if r is not None and r['cls']:
                for f in r['features']:
                    met.setdefault((r['cls'], f), []).append('%s%s' % (name, (H, W, C)))
    for pair in sorted(met):
        print('%-22s %-18s %3d  e.g. %s' % (pair + (len(met[pair]), met[pair][0])))
    assert not [p for p in COVERAGE if p not in met]


def test_what_the_shapes_are_for(tables):
    """16 x 16 x 48 keeps pointwise layers (K = 48 < 64) off the skinny kernel and splits no 3 x 3 layer (the one layer of a
    K x K class there is the strided 1x1 shortcut of learned_resample*: 8 x 8 output pixels, K = 48); 32 x 32 x 48 has K x K
    layers of the extended class, 32 x 32 x 64 of the standard class.  At 32 x 32 x 34 the library takes what reads a whole,
    aligned buffer whose channel count is a multiple of four, and nothing else: UNALIGNED."""
    by_shape = {}
    for (name, H, W, C), rows in tables.items():
        by_shape.setdefault((H, W, C), {})[name] = rows
    union = lambda shape: set().union(*[classes(rows) for rows in by_shape[shape].values()])
    small = [r for rows in by_shape[(16, 16, 48)].values() for r in rows if r is not None and r['cls'] in (STD_KXK, EXT_KXK)]
    assert small and all((r['name'], r['step'].attrs['kh'], r['step'].attrs['sh']) == ('sc', 1, 2) for r in small)
    assert {STD_PW, EXT_BNPW, CONVT} <= union((16, 16, 48))
    assert {STD_PW, EXT_KXK, EXT_BNPW, CONVT} <= union((32, 32, 48))
    assert {STD_PW, STD_KXK, EXT_BNPW, CONVT} <= union((32, 32, 64))
    got = {name: classes(rows) for name, rows in by_shape[S.UNALIGNED_SHAPE].items() if classes(rows)}
    assert got == UNALIGNED, got


# ---- 3. the twin -------------------------------------------------------------------------------------------------------------
def test_the_misaligned_twin_is_refused(tables, hip_lib):
    """slice_reader: the slice readers `p` (1x1) and `k` (3x3) read 16-byte aligned views (x.coff % 4 == 0, x.ld > Cin) and are
    split wherever their class is; slice_reader_odd: the same layers from channel 2 / 6 on are refused by both rules, hence
    fp32 under every mode and scope -- and by the alignment clause alone: the struct with its view moved by two channels is taken."""
    for shape in S.SPLIT_SHAPES:
        good = {r['name']: r for r in tables[('slice_reader',) + shape] if r is not None}
        odd = {r['name']: r for r in tables[('slice_reader_odd',) + shape] if r is not None}
        for name in ('p', 'k'):
            g, o = good[name], odd[name]
            assert 'x_view' in g['features'] and 'x_view' in o['features']
            assert g['step'].ins['x'].coff % 4 == 0 and o['step'].ins['x'].coff % 4 == 2
            assert g['step'].ins['x'].ld > g['step'].ins['x'].C and g['step'].ins['x'].ld % 4 == 0
            assert (o['std'], o['wide'], o['cls']) == (0, 0, None), (shape, name)
            for mode in MODES:
                for scope in ('standard', 'extended'):
                    assert expected_code(o, mode, scope) is None
            a = binding.bind(o['step'], batch(*shape[:2]), binding.FakeEnv(batch(*shape[:2])))[1][0]
            a.x += 8                                   # the twin's view, two channels on: nothing else changes
            assert hip_lib.dh_conv2d_split_eligible(C.byref(a)) == g['std']
            assert hip_lib.dh_conv2d_split_wide_eligible(C.byref(a)) == g['wide']
        assert good['wide']['std'] == odd['wide']['std'] == 1                    # the producer is the same layer in both
    assert good_classes(tables) == {(32, 32, 48): (STD_PW, EXT_KXK), (32, 32, 64): (STD_PW, STD_KXK), (16, 16, 48): (STD_PW, None)}


def good_classes(tables):
    out = {}
    for shape in S.SPLIT_SHAPES:
        rows = {r['name']: r for r in tables[('slice_reader',) + shape] if r is not None}
        out[shape] = (rows['p']['cls'], rows['k']['cls'])
    return out


# ---- 4. the clauses ------------------------------------------------------------------------------------------------------------
def rms(d):
    return float(np.sqrt(np.mean(np.square(np.asarray(d, np.float64)))))


class Ratios(dict):
    """the largest |got - ref| / limit per clause"""

    def note(self, clause, value):
        self[clause] = max(self.get(clause, 0.0), float(value))


def hold_mode(mode, outputs, got, base32, o32, o64, t64, e64, te64, L, any_split, label, ratios=None, log=False, extra=None):
    """The clauses a run `got` of a plan bound under `mode` is held to (tests/test_gpu_synth_graphs_split.py; here a CPU
    stand-in takes the engine's place).  o64 / o32 / t64: the plain fp64 / fp32 evaluations and the fp64 taps; e64 / te64: the
    fp64 evaluation OF THE MODE (evaluate(float64, split=(P, ids of the plan))) and its taps; base32: the run of the fp32 plan.

      'bf16x3'  graphref.compare against o64, both clauses (the mode is of the fp32 class); decoder outputs through
                graphref.compare_decoder.
      'bf16x2'  |got - e64| <= graphref.bar(e64, te64, L) element-wise.
      'bf16'    max|got - o64| <= max(max graphref.bar(o64, t64, L), 2 max|e64 - o64|) per output.
      engaged   ('bf16x2', 'bf16', any_split): some output differs from base32, and each that does is closer (RMS) to e64
                than to o64.
    Raises AssertionError; `ratios` (a Ratios) collects |got - ref| / limit per clause; log / extra: graphref.compare's
    printing and recording, with `extra` as further fields of the record."""
    ratios = Ratios() if ratios is None else ratios
    assert len(got) == len(o64) == len(outputs)
    differ = []
    for k, t in enumerate(outputs):
        g = np.asarray(got[k], np.float64)
        name = '%s.%d' % (label, k)
        assert g.shape == o64[k].shape and np.all(np.isfinite(g)), '%s: shape / non-finite values' % name
        A = GR.amplitude(t64)
        if mode == 'bf16x3':
            if GR.is_decoder_output(t):
                GR.compare_decoder(name, t, got[k], o32[k], o64[k], t64)
            else:
                e_hip, e_cpu = float(np.abs(g - o64[k]).max()), float(np.abs(o32[k].astype(np.float64) - o64[k]).max())
                ratios.note('bf16x3: 4 |o32 - o64| + 1e-6 A', e_hip / (4 * e_cpu + 1e-6 * A))
                ratios.note('bf16x3: bar', float((np.abs(g - o64[k]) / GR.bar(o64[k], t64, L)).max()))
                GR.compare(name, got[k], o32[k], o64[k], t64, L, log=log, **(extra or {}))
        elif mode == 'bf16x2':
            r = float((np.abs(g - e64[k]) / GR.bar(e64[k], te64, L)).max())
            ratios.note('bf16x2: bar(e64)', r)
            assert r <= 1.0, '%s: %.3f of the bar away from the emulated mode' % (name, r)
        else:
            e = float(np.abs(g - o64[k]).max())
            limit = max(float(GR.bar(o64[k], t64, L).max()), 2 * float(np.abs(e64[k] - o64[k]).max()))
            ratios.note('bf16: max(bar, 2 |e64 - o64|)', e / limit)
            assert e <= limit, '%s: %.3e from fp64, limit %.3e' % (name, e, limit)
        if mode != 'bf16x3' and not np.array_equal(got[k], base32[k]):
            differ.append(k)
            a, b = rms(g - e64[k]), rms(g - o64[k])
            ratios.note('%s engaged: rms(got - e64) / rms(got - o64)' % mode, a / b if b else np.inf)
            assert a < b, '%s: rms %.3e from the emulated mode, %.3e from fp64: the mode is not engaged' % (name, a, b)
    if mode != 'bf16x3' and any_split:
        assert differ, '%s: a layer is split, yet every output has the bits of the fp32 plan' % label
    return ratios


class Reference:
    """the evaluations of one case that do not depend on the mode, and the emulated ones by (P, ids)"""

    def __init__(self, m, x):
        self.m, self.x, self.t64, self._e = m, x, {}, {}
        self.o64 = GR.evaluate(m.inputs, m.outputs, x, torch.float64, taps=self.t64)
        self.o32 = GR.evaluate(m.inputs, m.outputs, x, torch.float32)
        self.L = GR.layers_on_longest_path(m.outputs)

    def emulated(self, parts, ids):
        key = (parts, frozenset(ids))
        if key not in self._e:
            te = {}
            self._e[key] = (GR.evaluate(self.m.inputs, self.m.outputs, self.x, torch.float64, taps=te,
                                        split=(parts, ids)), te)
        return self._e[key]

    def stand_in(self, parts, ids, skip=None):
        """the mode in fp32 arithmetic, another summation order than the engine's: what a correct engine may look like"""
        return GR.evaluate(self.m.inputs, self.m.outputs, self.x, torch.float32, split=(parts, ids), skip=skip)

    def hold(self, mode, got, base32, ids, label, ratios=None, log=False, extra=None):
        e64, te = self.emulated(PARTS[mode], ids)
        return hold_mode(mode, self.m.outputs, got, base32, self.o32, self.o64, self.t64, e64, te, self.L, bool(ids), label,
                         ratios=ratios, log=log, extra=extra)


def modes_at(H, W):
    """the modes a case of SPLIT_SHAPES runs: all three on the 32 x 32 maps; 16 x 16 x 48 leaves 'bf16x3' out (its split layers
    are the pointwise class of 32 x 32 x 48 over again, and the GPU file's wall time is the suite's)"""
    return MODES if H * W > 256 else MODES[1:]


def scopes_and_modes(rows, H, W):
    """[(scope, mode)] the GPU test runs numerically for a case of SPLIT_SHAPES: its modes under 'standard'; and under
    'extended' where the table has a layer of an added class (elsewhere 'extended' must give the bits of 'standard')"""
    out = [('standard', m) for m in modes_at(H, W)]
    if classes(rows) & set(ADDED):
        out += [('extended', m) for m in modes_at(H, W)]
    return out


ALL_CASES = cases()


@pytest.mark.parametrize('name,fn,seed,H,W,C', ALL_CASES, ids=['%s-%dx%dx%d' % (c[0], c[3], c[4], c[5]) for c in ALL_CASES])
def test_the_clauses_hold_for_the_reference_alone(name, fn, seed, H, W, C, hip_lib, record_property):
    """evaluate(float32, split=(P, ids)) -- the mode itself, fp32 arithmetic, another summation order -- passes every clause of
    hold_mode, for every case, scope and mode the GPU test runs.  Largest ratios to the limits over all cases (torch-CPU):
      bf16x3: bar 0.034, 4 |o32 - o64| + 1e-6 A 0.21;  bf16x2: bar(e64) 0.094;  bf16: max(bar, 2 |e64 - o64|) 0.53;
      engaged, rms(got - e64) / rms(got - o64): bf16x2 0.46, bf16 0.17."""
    m = S.build(fn, H, W, C, seed=seed)
    rows = default_table(hip_lib, m, H, W)
    ref = Reference(m, S.frames(m, batch(H, W)))
    ratios = Ratios()
    for scope, mode in scopes_and_modes(rows, H, W):
        ids = table_param_ids(rows, scope)
        ref.hold(mode, ref.stand_in(PARTS[mode], ids), ref.o32, ids, '%s[%s %s]' % (name, mode, scope), ratios)
    for k, v in sorted(ratios.items()):
        print('%-52s %.4f' % (k, v))
        record_property(k, v)


# one graph per class; the layers of THAT class alone are emulated, so that what fails is the class's own doing
BITE = (
    (STD_PW, S.conv_pool, (32, 32, 48), 'standard'),
    (STD_KXK, S.epi_chain, (32, 32, 64), 'standard'),
    (EXT_KXK, S.epi_chain, (32, 32, 48), 'extended'),
    (EXT_BNPW, S.siblings, (32, 32, 48), 'extended'),
    (CONVT, S.learned_resample, (32, 32, 48), 'standard'),
)


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('cls,fn,shape,scope', BITE, ids=[b[0].replace(' ', '_') for b in BITE])
def test_the_clauses_bite(cls, fn, shape, scope, hip_lib):
    """The stand-in of the next rung down fails the upper rung's clauses: P = 2 under 'bf16x3''s, P = 1 under 'bf16x2''s -- on
    conv_pool (standard pointwise), epi_chain at C = 64 (standard K x K) and at C = 48 (extended K x K), siblings (extended
    BN-pointwise) and learned_resample (transposed), with the layers of that class alone emulated.  And with any one
    BatchNormalization or add behind such a layer skipped, the stand-in of 'bf16' fails that mode's loose clause."""
    m = S.build(fn, *shape)
    rows = default_table(hip_lib, m, *shape[:2])
    assert cls in classes(rows, scope)
    ids = table_param_ids(rows, scope, only=cls)
    ref = Reference(m, S.frames(m, batch(*shape[:2])))
    for mode in MODES:                                   # intact: every rung passes its own clauses
        ref.hold(mode, ref.stand_in(PARTS[mode], ids), ref.o32, ids, mode)
    assert _fails(ref.hold, 'bf16x3', ref.stand_in(2, ids), ref.o32, ids, 'P = 2 as bf16x3')
    assert _fails(ref.hold, 'bf16x2', ref.stand_in(1, ids), ref.o32, ids, 'P = 1 as bf16x2')
    # the epilogue nodes behind a split layer: every bn / add that reads what such a layer writes
    split_nodes = [n for n in m._nodes if n.op in GR.LAYER_COST and
                   any(id(p) in ids for layer in n.layers.values() for p in layer.params)]
    behind = [n for n in m._nodes if n.op in ('bn', 'add') and any(t.node in split_nodes for t in n.inputs)]
    assert behind, 'no bn / add behind a split layer in %s' % fn.__name__
    for node in behind:
        assert _fails(ref.hold, 'bf16', ref.stand_in(1, ids, skip=node), ref.o32, ids, 'skip %s' % node.name), node.name


def test_hook_is_inert_without_ids_and_exact_for_three_parts():
    """split=(P, empty set) gives the bits of the plain evaluation; E_3 of a layer is the fp32 product up to terms of 2^-24
    relative size (bf16_modes_ref), so the fp64 evaluations with and without it agree to ~1e-6 -- and E_1 does not."""
    m = S.build(S.slice_reader, 32, 32, 48)
    x = S.frames(m, 2)
    plain = GR.evaluate(m.inputs, m.outputs, x, torch.float64)
    for parts in (1, 2, 3):
        assert all(np.array_equal(a, b) for a, b in zip(plain, GR.evaluate(m.inputs, m.outputs, x, torch.float64, split=(parts, set()))))
    ids = {id(p) for p in m.params if p.role == 'conv'}
    d = {parts: max(float(np.abs(a - b).max()) for a, b in zip(plain, GR.evaluate(m.inputs, m.outputs, x, torch.float64,
                                                                                   split=(parts, ids)))) for parts in (1, 2, 3)}
    print(d)
    assert d[3] < 2e-6 < 2e-4 < d[1] and d[3] < d[2] < d[1]
