"""The host binder against what the engine launches: a plan is bound on the device (executor.BoundPlan), then bound again
with a binding.FakeEnv at the device arena's address; every argument struct and every scalar must agree byte for byte once
arena pointers are offsets and weight / table pointers are "null or not" (tests/test_binding_host.py: canonical), with the
weight layout of the fake struct taken from the host classification (binding.weight_layout on the FAKE struct)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synthgraphs as S                            # noqa: E402
import test_binding_host as B                      # noqa: E402
from test_gpu_synth_graphs import _variant         # noqa: E402

from deephar_amd.engine import binding, executor, packing      # noqa: E402

pytestmark = pytest.mark.gpu


class _DeviceEnv:
    """what canonical_ptr needs of the bound plan: its arena; every other non-null address is a weight or a table"""
    tables = None

    def __init__(self, bp):
        self.base = bp.base


def _models():
    from test_gpu_models import _build
    graph = lambda **kw: _variant(S.build(S.learned_resample, *B.smallest(S.learned_resample)), **kw)
    return [('reception2d', lambda: _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)[0], 2),
            ('learned_resample', graph, 2),
            ('learned_resample-bf16x3-extended', lambda: graph(gemm_precision='bf16x3', gemm_scope='extended'), 2)]


@pytest.mark.parametrize('name,make,n', _models(), ids=[m[0] for m in _models()])
def test_device_binding_is_the_host_binding(name, make, n, hip_lib, cuda):
    m = make()
    ex = m.executor
    ex.autotune = False
    plan = m.plan
    with torch.cuda.device(ex.device), torch.cuda.stream(ex.stream):
        bp = executor.BoundPlan(plan, n, ex.store, ex.device)
    ex.stream.synchronize()
    assert bp.npre == 0 and len(bp.calls) == len(plan.steps)
    dev, items = _DeviceEnv(bp), bp.arena.numel()
    bound_codes = {id(s): s.attrs.get('w_split') for s in plan.steps}
    host, env = B.launches(plan, n, base=bp.base)
    kinds = set()
    for (fn, args, step), (s, fname, structs, scalars) in zip(bp.calls, host):
        assert step is s
        if s.kind in ('conv', 'convtranspose'):
            fake = structs[0]
            if s.kind == 'conv':
                code = fake.w_split = binding.weight_layout(hip_lib, plan, fake)
            else:
                code = binding.convt_weight_layout(hip_lib, plan, fake)
                if code:
                    fname, scalars = 'dh_conv2d_transpose2x2_split_f32', [packing.SPLIT_PARTS[code]] + scalars
            assert code == bound_codes[id(s)], (s.name, code, bound_codes[id(s)])
            fake.w = 1 << 20                                          # (the engine must have bound SOME weight)
            env.tables['w'] = 1 << 20
        nst = len(structs)
        assert fn is getattr(hip_lib, fname), (s.kind, s.name, fname)
        got = B.canonical(fname, [a._obj for a in args[:nst]], list(args[nst:]), dev, items)
        want = B.canonical(fname, structs, scalars, env, items)
        assert got == want, (s.kind, s.name)
        kinds.add((s.kind, bound_codes[id(s)]))
    print(sorted(kinds, key=str))
    if name.startswith('learned_resample'):
        assert any(k == 'convtranspose' for k, _ in kinds) and any(k == 'dwconv' for k, _ in kinds)
    if 'bf16x3' in name:
        assert any(k == 'convtranspose' and c == 1 for k, c in kinds)
