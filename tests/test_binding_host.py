"""engine/binding.py without a device: every step of the default plans of the synthetic zoo (tests/synthgraphs.py, each graph at
its smallest shape) and of the two small models of tests/test_gpu_plan_api.py binds under binding.FakeEnv; every pointer it
writes is null, inside the fake arena, or one of the fake tables; and between batch 1 and batch 3 the batch count of a struct
(N / F / npix) triples while every pitch and every other field stays.  `launches` / `canonical` are shared with
tests/test_gpu_binding.py, which holds the same structs against what the engine binds on the device."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synthgraphs as S                            # noqa: E402

from deephar_amd import _lib                       # noqa: E402
from deephar_amd.engine import binding             # noqa: E402

BATCH_FIELDS = ('N', 'F', 'npix')                  # the one field of an argument struct that counts frames
BASE = 1 << 40                                     # the fake arena's address: above every fake table (k << 20)
ARENA, TABLE = 1 << 60, (1 << 64) - 1              # canonical pointers: ARENA | byte offset, TABLE for anything else non-null


def smallest(fn):
    return min((s for c in S.ZOO if c.fn is fn for s in c.shapes), key=lambda s: s[0] * s[1] * s[2])


def models():
    """(name, builder of a model) of every case"""
    from test_gpu_models import _build
    fns = list(dict.fromkeys(c.fn for c in S.ZOO))
    return [(fn.__name__, lambda fn=fn: S.build(fn, *smallest(fn))) for fn in fns] + \
        [('reception2d', lambda: _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)[0]),
         ('reception3d', lambda: _build(3, 2, 17, depth_maps=16)[0])]


def canonical_ptr(p, env, items):
    """null -> 0; an address inside env's arena of `items` floats -> ARENA | offset; one of env's tables, or (env.tables is None:
    a device environment) any other address -> TABLE; anything else is an error"""
    p = int(p or 0)
    if p == 0:
        return 0
    if env.base <= p < env.base + 4 * items:
        assert (p - env.base) % 4 == 0
        return ARENA | (p - env.base)
    assert env.tables is None or p in env.tables.values(), 'pointer 0x%x is neither in the arena nor a table' % p
    return TABLE


def canonical(name, structs, scalars, env, items):
    """(entry point, struct bytes with canonical pointers..., scalars with canonical pointers)"""
    out = [name]
    for st in structs:
        raw = bytearray(bytes(st))
        for f, t in st._fields_:
            if t is C.c_void_p:
                off = getattr(type(st), f).offset
                raw[off:off + 8] = canonical_ptr(getattr(st, f), env, items).to_bytes(8, 'little')
        out.append(bytes(raw))
    sig = _lib.SIGNATURES[name][1][len(structs):-1]          # (without the structs in front and the stream behind)
    assert len(sig) == len(scalars), (name, len(sig), len(scalars))
    out.append(tuple(canonical_ptr(v, env, items) if t is C.c_void_p else v for t, v in zip(sig, scalars)))
    return out


def launches(plan, n, base=BASE):
    """[(step, name, structs, scalars)] of every step of `plan` under a FakeEnv, and the env"""
    env = binding.FakeEnv(n, base=base)
    return [(s,) + tuple(binding.bind(s, n, env)) for s in plan.steps], env


@pytest.mark.parametrize('name,make', models(), ids=[m[0] for m in models()])
def test_every_step_binds_and_scales_with_the_batch(name, make, hip_lib):
    plan = make().plan
    (one, env1), (three, env3) = launches(plan, 1), launches(plan, 3)
    assert len(one) == len(three) == len(plan.steps) > 0
    for (s, name1, st1, sc1), (_, name3, st3, sc3) in zip(one, three):
        assert name1 == name3 and hasattr(hip_lib, name1), (s.kind, s.name)
        c1 = canonical(name1, st1, sc1, env1, plan.arena_items * 1)      # (raises on a pointer that is out of range)
        c3 = canonical(name3, st3, sc3, env3, plan.arena_items * 3)
        assert [len(b) for b in c1[1:-1]] == [C.sizeof(st) for st in st1]
        for a, b in zip(st1, st3):
            assert type(a) is type(b)
            for f, t in a._fields_:
                va, vb = getattr(a, f), getattr(b, f)
                if t is C.c_void_p:
                    assert (va is None) == (vb is None), (s.name, f)
                elif f in BATCH_FIELDS:
                    assert va > 0 and vb == 3 * va, (s.name, f, va, vb)
                else:
                    assert va == vb, (s.name, f, va, vb)               # ldx, ldy, every pitch and extent: per frame
            assert sum(1 for f, _ in a._fields_ if f in BATCH_FIELDS) == (0 if isinstance(a, _lib.ConvSeg) else 1)
            if hasattr(a, 'ldx'):
                assert a.ldx == s.ins['x'].ld and a.ldy == s.outs['y'].ld
        counts = 0
        for t, va, vb in zip(_lib.SIGNATURES[name1][1][len(st1):-1], c1[-1], c3[-1]):
            if t is C.c_void_p:
                assert (va == 0) == (vb == 0), (s.name, va, vb)
            elif va > 0 and vb == 3 * va:
                counts += 1
            else:
                assert va == vb, (s.name, va, vb)
        assert counts == (0 if st1 else 1), s.name                        # a launch of scalars alone: ONE of them counts frames
