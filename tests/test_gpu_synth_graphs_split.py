"""The split-bf16 leg of tests/test_gpu_synth_graphs.py: fused plans of the synthetic graphs (tests/synthgraphs.py) bound under
gemm_precision = 'bf16x3' / 'bf16x2' / 'bf16' and gemm_scope = 'standard' / 'extended', held to a reference OF THE MODE -- the
fp64 graph interpreter with the bound plan's split layers evaluated as E_P (tests/graphref.py: evaluate(split=...)).

Per (graph, shape): the bound w_split codes equal the library's own classification (tests/test_synth_split_host.py:
classify) step by step; the outputs pass the mode's clauses (test_synth_split_host.hold_mode, proven on a CPU stand-in there);
where nothing is eligible a mode gives the bits of the fp32 plan; a layer of the standard class keeps its bits under
gemm_scope='extended'; and per mode the run is bit-identical with the arena poisoned, on two streams, for one frame alone,
repeated, through the C-level plan executor -- with every rule switched off it is held to the same clauses."""
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
import test_synth_split_host as H                  # noqa: E402
from test_gpu_synth_graphs import _predict, _same_bits, _variant      # noqa: E402

from deephar_amd import graph as G                 # noqa: E402

pytestmark = pytest.mark.gpu

CASES = H.cases() + H.unaligned_cases()


def _bound_codes(m, rows, mode, scope, n, tag):
    """The layers that matter are split: the bound w_split of every conv / convtranspose step is the mode's code where the
    host table says eligible and an fp32 packing (0, or 2: the halo kernel) elsewhere, and no grouped or paired launch has
    taken a split step in.  Returns the number of split steps."""
    steps = m.plan.steps
    assert len(steps) == len(rows), '%s: %d steps, the table has %d' % (tag, len(steps), len(rows))
    nsplit = 0
    for s, r in zip(steps, rows):
        if r is None:
            assert s.kind not in ('conv', 'convtranspose')
            continue
        assert (s.kind, s.name) == (r['kind'], r['name'])
        want, code = H.expected_code(r, mode, scope), s.attrs['w_split']
        if want is None:
            assert code in (0, 2), '%s: %s is bound with w_split %d, the library refuses the layer' % (tag, s.name, code)
        else:
            assert code == want, '%s: %s is bound with w_split %d, expected %d' % (tag, s.name, code, want)
            nsplit += 1
    bp = m.executor.bind(n)
    for i, sk in bp.absorbed.items():
        for s in (bp.calls[i][2], sk):
            assert s.attrs.get('w_split', 0) not in GR.SPLIT_CODES, '%s: %s runs inside a grouped / paired launch' % (tag, s.name)
    assert not [s.name for s in steps if s.attrs.get('grouped') and s.attrs.get('w_split', 0) in GR.SPLIT_CODES]
    return nsplit


def _ancestor_params(t):
    """id()s of the Params of every layer an output depends on"""
    return {id(p) for node in G.topo_nodes([t]) for layer in node.layers.values() for p in layer.params}


@pytest.mark.parametrize('name,fn,seed,H_,W,C', CASES, ids=['%s-%dx%dx%d' % (c[0], c[3], c[4], c[5]) for c in CASES])
def test_synthetic_graph_split(name, fn, seed, H_, W, C, hip_lib, cuda, tmp_path):
    """Measured on an MI355X (1536 recorded comparisons of 192 cases), the largest |got - ref| / limit per clause:
      'bf16x3'  0.029 of the bar, 0.26 of 4 |o32 - o64| + 1e-6 A (siblings, siblings_output at 32 x 32 x 64); its bits differed from the fp32
                plan's in every one of the 240 runs with a split layer;
      'bf16x2'  0.093 of bar(e64);  engaged: rms(hip - e64) / rms(hip - o64) at most 0.53;
      'bf16'    0.50 of max(bar, 2 |e64 - o64|) -- the engine sits on the emulated mode, the limit is twice the mode's own
                distance from fp64;  engaged: rms(hip - e64) / rms(hip - o64) at most 0.17.
    The CPU stand-in of tests/test_synth_split_host.py measures 0.034 / 0.21, 0.094 / 0.46 and 0.53 / 0.17 for the same clauses.
    Wall time 27.8 s (192 cases) beside 8.8 s for the 193 cases of tests/test_gpu_synth_graphs.py on the same machine, with
    'bf16x3' already left out at 16 x 16 x 48 (test_synth_split_host.modes_at); no case takes more than 0.5 s."""
    m0 = S.build(fn, H_, W, C, seed=seed)
    n = H.batch(H_, W)
    x = S.frames(m0, n)
    ref = H.Reference(m0, x)
    rows = H.default_table(hip_lib, m0, H_, W)
    rows_off = H.default_table(hip_lib, m0, H_, W, rules=S.all_off())
    tag = '%s-%dx%dx%d' % (name, H_, W, C)
    case = os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]
    ratios = H.Ratios()
    base32 = _predict(_variant(m0), x, n)
    base32_off = []                                    # the fp32 plan with every rule off: what ITS split forms depart from

    def bound(mode, scope, table=rows, **opts):
        """a variant bound under (mode, scope), its outputs, the ids of its split layers"""
        m = _variant(m0, gemm_precision=mode, gemm_scope=scope, **opts)
        got = _predict(m, x, n)
        what = '%s[%s %s%s]' % (tag, mode, scope, ' all_off' if 'rules' in opts else '')
        nsplit = _bound_codes(m, table, mode, scope, n, what)
        ids = GR.split_param_ids(m)
        assert ids == H.table_param_ids(table, scope) and bool(ids) == bool(nsplit)
        return m, got, ids, nsplit, what

    def numerics(mode, scope, got, ids, nsplit, what, base32=base32):
        if not ids:                                   # nothing eligible means the fp32 plan
            assert _same_bits(got, base32), '%s: no layer is split, yet other bits than the fp32 plan' % what
            return
        ref.hold(mode, got, base32, ids, what, ratios=ratios, log=True,
                 extra=dict(graph=name, mode=mode, scope=scope, split_layers=nsplit))
        e64, _ = ref.emulated(H.PARTS[mode], ids)
        for k in range(len(got)):
            if mode != 'bf16x3':
                paritylog.record('%s.%d' % (what, k), got[k], ref.o32[k], ref.o64[k], case, px=False, graphref=True, graph=name,
                                 mode=mode, scope=scope, split_layers=nsplit,
                                 hip_vs_e64=float(np.abs(got[k].astype(np.float64) - e64[k]).max()),
                                 e64_vs_o64=float(np.abs(e64[k] - ref.o64[k]).max()))
        if mode == 'bf16x3':
            print('%s: bits %s the fp32 plan\'s' % (what, 'equal' if _same_bits(got, base32) else 'differ from'))

    def invariants(m, mode, scope, got, what):
        """bit for bit against the mode's own default run"""
        ex = m.executor
        bp = ex.bind(n)
        for use_graph in (False, True):               # arena poisoning: two finite fills, eagerly and through the captured graph
            ex.use_graph = use_graph
            for fill in (2.0 ** 100, 1.0):
                bp.arena.fill_(fill)
                torch.cuda.synchronize()
                again = _predict(m, x, n)
                assert all(np.all(np.isfinite(g)) for g in again)
                assert _same_bits(again, got), '%s: arena filled with %g, %s: other bits' % (what, fill, 'graph' if use_graph else 'eager')
        assert ex.bind(n) is bp
        assert _same_bits(_predict(m, x, n), got), '%s: a second predict gives other bits' % what
        two = _variant(m0, gemm_precision=mode, gemm_scope=scope, num_streams=2, stream_policy='list')
        assert _same_bits(_predict(two, x, n), got), '%s: two streams give other bits' % what
        assert _same_bits(_predict(m, [a[:1] for a in x], 1), [b[:1] for b in got]), '%s: one frame alone' % what
        path = str(tmp_path / 'synth.dhplan')
        m.export_plan(path, n)
        blob = open(path, 'rb').read()
        plan = ctypes.c_void_p()
        assert hip_lib.dh_plan_create(blob, len(blob), ctypes.byref(plan)) == 0
        try:
            xd = [torch.from_numpy(a).to(cuda) for a in x]
            outs = [torch.full(r.shape, float('nan'), device=cuda) for r in got]
            ins_p = (ctypes.c_void_p * len(xd))(*[a.data_ptr() for a in xd])
            outs_p = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            assert hip_lib.dh_forward(plan, ins_p, n, outs_p, torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            assert _same_bits([o.cpu().numpy() for o in outs], got), '%s: the exported plan gives other bits' % what
        finally:
            assert hip_lib.dh_plan_destroy(plan) == 0

    def leg(mode, scope):
        m, got, ids, nsplit, what = bound(mode, scope)
        numerics(mode, scope, got, ids, nsplit, what)
        if ids:
            invariants(m, mode, scope, got, what)
            # every rule off: the same clauses, with the reference of ITS bound plan
            _, goff, ioff, noff, woff = bound(mode, scope, table=rows_off, rules=S.all_off())
            if not base32_off:
                base32_off.extend(_predict(_variant(m0, rules=S.all_off()), x, n))
            numerics(mode, scope, goff, ioff, noff, woff, base32=base32_off)
        return got

    if (H_, W, C) == S.UNALIGNED_SHAPE:
        # 'bf16' only; next to nothing is eligible here (test_synth_split_host.UNALIGNED): the bits of the fp32 plan
        for scope in ('standard', 'extended'):
            leg('bf16', scope)
    else:
        modes = H.modes_at(H_, W)
        std = {mode: leg(mode, 'standard') for mode in modes}
        added = H.table_param_ids(rows, 'extended') - H.table_param_ids(rows, 'standard')
        if added:
            assert H.classes(rows) & set(H.ADDED)
            for mode in modes:
                got = leg(mode, 'extended')
                for k, t in enumerate(m0.outputs):     # behind layers of the standard class only: the bits of 'standard'
                    if not _ancestor_params(t) & added:
                        assert np.array_equal(got[k], std[mode][k]), '%s output %d: other bits under gemm_scope=extended' % (tag, k)
        else:                                          # no layer of an added class: the scope changes nothing
            _, got, ids, _, what = bound('bf16x2', 'extended')
            assert _same_bits(got, std['bf16x2']), '%s: other bits than under gemm_scope=standard' % what
    for k, v in sorted(ratios.items()):
        print('RATIO %-52s %.4f' % (k, v))
