"""Multi-stream plans for the C executor, without a device: the schedule section of a version-5 blob (engine/serialize.py)
run through the GPU-free schedule module (csrc/plan_sched.h behind dh_sched_build_ops) and the resulting enqueue program
checked against the plan's happens-before relation; the tables the module must refuse; dh_pack_outputs_host against NumPy
slicing; and the export keyword leaving every single-stream blob as it was.  Nothing is computed on: every comparison is
exact.  tools/sched_sweep.cpp runs random tables through the same two headers as a stand-alone program for a sanitizer build."""
import ctypes as C
import functools
import hashlib
import inspect
import struct
import types

import numpy as np
import pytest

from deephar_amd import _lib
from deephar_amd.engine import schedule, serialize

EINVAL = -1
LAUNCH, RECORD, WAIT = _lib.SCHED_LAUNCH, _lib.SCHED_RECORD, _lib.SCHED_WAIT


# ---- plans (built without a device) ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def spnet_plan(streams, policy):
    """the small SPNet of test_host_logic.test_tail_stream_policy_is_one_directional_and_sound"""
    from deephar_amd import graph, utils
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import spnet
    graph.reset_naming()
    cfg = ModelConfig((8, 128, 128, 3), utils.pa16j2d, num_actions=[15], num_pyramids=2, action_pyramids=[1, 2],
                      num_levels=4, pose_replica=True, num_pose_features=160, num_visual_features=160)
    m = spnet.build(cfg)
    m.num_streams, m.stream_policy = streams, policy
    return m.plan


@functools.lru_cache(maxsize=None)
def reception_plan(streams, policy):
    """the 2-block ReceptionNet of test_gpu_models._build(2, 2, 16, num_context_per_joint=2)"""
    from deephar_amd import graph
    from deephar_amd.models import reception
    graph.reset_naming()
    m = reception.build((256, 256, 3), 16, dim=2, num_blocks=2, ksize=(5, 5), num_context_per_joint=2)
    m.num_streams, m.stream_policy = streams, policy
    return m.plan


PLANS = [('spnet', 2, 'tail'), ('spnet', 3, 'tail'), ('spnet', 2, 'list'), ('reception', 2, 'list'), ('reception', 3, 'list')]


def get_plan(kind, streams, policy):
    return (spnet_plan if kind == 'spnet' else reception_plan)(streams, policy)


# ---- the schedule module -----------------------------------------------------------------------------------------------------

def build_ops(lib, entries, nstreams, npre, nsteps=None, wait_off=None, nwaits=None):
    """entries [(step or None, stream, records, [waits])] -> (rc, [(kind, stream, arg, entry)], nevents) of dh_sched_build_ops"""
    n = len(entries)
    arr = lambda vals: (C.c_int32 * max(len(vals), 1))(*vals)
    waits = [w for e in entries for w in e[3]]
    if wait_off is None:
        wait_off = [0]
        for e in entries:
            wait_off.append(wait_off[-1] + len(e[3]))
    if nsteps is None:
        nsteps = sum(1 for e in entries if e[0] is not None)
    step = arr([-1 if e[0] is None else e[0] for e in entries])
    stream, record = arr([e[1] for e in entries]), arr([1 if e[2] else 0 for e in entries])
    nops, nev = C.c_int(-1), C.c_int(-1)
    args = (n, step, stream, record, arr(wait_off), arr(waits), len(waits) if nwaits is None else nwaits, nstreams, npre, nsteps)
    rc = lib.dh_sched_build_ops(*args, None, 0, C.byref(nops), C.byref(nev))
    if rc != 0:
        return rc, None, None
    ops = (_lib.SchedOp * nops.value)()
    assert lib.dh_sched_build_ops(*args, ops, nops.value, C.byref(nops), C.byref(nev)) == 0 and nops.value == len(ops)
    return 0, [(o.kind, o.stream, o.arg, o.entry) for o in ops], nev.value


def unpack_section(section):
    """the schedule section's bytes -> (nstreams, npre, entries): what the library reads"""
    ns, npre, nent, nwaits = struct.unpack_from('<IIII', section)
    rows = [struct.unpack_from('<IIII', section, 16 + 16 * i) for i in range(nent)]
    waits = list(struct.unpack_from('<%dI' % nwaits, section, 16 + 16 * nent))
    assert len(section) == 16 + 16 * nent + 4 * nwaits and sum(r[3] for r in rows) == nwaits
    entries, at = [], 0
    for step, stream, flags, nw in rows:
        entries.append((None if step == serialize.NO_LAUNCH else step, stream, bool(flags & 1), waits[at:at + nw]))
        at += nw
    return ns, npre, entries


def check_program(ops, nevents, entries, nstreams, npre):
    """(a), (c), (d), (e) of the enqueue program; -> (launch_pos {entry: op index}, after [op index -> bitmask of the entries
    whose LAUNCH is ordered behind that op by stream order + record -> wait edges], number of relays)"""
    recorded, on_stream = {}, {}                                   # event -> (op index, stream) of its newest RECORD
    launch_pos, edges, last = {}, [[] for _ in ops], {}
    relays = 0
    nrec = sum(1 for e in entries if e[2])
    for k, (kind, stream, arg, entry) in enumerate(ops):
        assert 0 <= stream < nstreams and kind in (LAUNCH, RECORD, WAIT)
        if stream in last:
            edges[last[stream]].append(k)
        last[stream] = k
        if kind == LAUNCH:
            assert entries[entry][0] == arg and entries[entry][1] == stream and entry not in launch_pos
            launch_pos[entry] = k
        elif kind == RECORD:
            assert 0 <= arg < nevents
            recorded[arg] = (k, stream)
            relays += arg >= nstreams + nrec
        else:
            assert arg in recorded, ('(a) WAIT %d names an event nobody has recorded yet' % k, arg)
            src_op, src_stream = recorded[arg]
            assert src_stream != stream
            # (c) a side stream never waits directly on a higher-numbered side stream
            assert not (stream != 0 and src_stream > stream), ('(c)', k, stream, src_stream)
            edges[src_op].append(k)
    assert sorted(launch_pos) == [i for i, e in enumerate(entries) if e[0] is not None]
    # (d) the staging entries, then the fork
    assert [o[0] for o in ops[:npre]] == [LAUNCH] * npre and all(o[1] == 0 for o in ops[:npre])
    assert [o[3] for o in ops[:npre]] == list(range(npre))
    if nstreams > 1:
        assert ops[npre] == (RECORD, 0, 0, -1)
        assert ops[npre + 1:npre + nstreams] == [(WAIT, k, 0, -1) for k in range(1, nstreams)]
        # (e) every side stream is joined exactly once, and the joins come last
        tail = ops[len(ops) - 2 * (nstreams - 1):]
        assert tail == [o for k in range(1, nstreams) for o in ((RECORD, k, k, -1), (WAIT, 0, k, -1))]
        body = ops[npre + nstreams:len(ops) - 2 * (nstreams - 1)]
        assert all(o[3] >= npre for o in body) and not any(o[0] != LAUNCH and o[2] < nstreams for o in body)
    after = [0] * len(ops)
    for k in range(len(ops) - 1, -1, -1):
        mask = 0
        for j in edges[k]:
            assert j > k
            mask |= after[j]
            if ops[j][0] == LAUNCH:
                mask |= 1 << ops[j][3]
        after[k] = mask
    return launch_pos, after, relays


@pytest.mark.parametrize('kind,streams,policy', PLANS)
def test_enqueue_program_keeps_the_plans_happens_before(kind, streams, policy, hip_lib):
    plan = get_plan(kind, streams, policy)
    assert plan.nstreams == streams
    section = serialize.schedule_section(plan.steps, plan.nstreams, multi_stream=True)
    ns, npre, entries = unpack_section(section)
    assert (ns, npre, len(entries)) == (plan.nstreams, 0, len(plan.steps))
    assert entries == schedule.schedule_entries(plan.steps)
    for j, (e, s) in enumerate(zip(entries, plan.steps)):
        assert e == (j, s.stream, bool(s.record), list(s.wait))
    rc, ops, nev = build_ops(hip_lib, entries, ns, npre)
    assert rc == 0
    launch_pos, after, relays = check_program(ops, nev, entries, ns, npre)
    # (b) what the arena layout relies on: every pair the plan orders is ordered by the program
    n = len(plan.steps)
    reach = schedule.happens_before(n, schedule.compute_deps(plan), [s.stream for s in plan.steps])
    for i in range(n):
        missing = reach[i] & ~after[launch_pos[i]]
        assert missing == 0, ('(b) step %d is not ordered before steps' % i, [j for j in range(n) if missing >> j & 1][:8])
    nwait = sum(len(e[3]) for e in entries)
    assert sum(1 for o in ops if o[0] == WAIT) == nwait + relays + 2 * (ns - 1)
    print('%s %d %s: %d entries, %d waits, %d relays, %d ops' % (kind, streams, policy, n, nwait, relays, len(ops)))


# a 3-stream table by hand: entry 3 (stream 1) waits for entry 2 (stream 2) -> a relay through stream 0; entry 6 (stream 2)
# waits for entry 3 (stream 1) directly; entry 0 stages the input
HAND = [(0, 0, False, []), (1, 0, True, []), (2, 2, True, [1]), (3, 1, True, [2]), (4, 1, True, []), (5, 0, False, [4]),
        (6, 2, False, [3])]


def test_hand_made_table_needs_a_relay(hip_lib):
    rc, ops, nev = build_ops(hip_lib, HAND, 3, 1)
    assert rc == 0
    launch_pos, after, relays = check_program(ops, nev, HAND, 3, 1)
    assert relays == 1 and nev == 3 + 4 + 1
    k = launch_pos[3]
    assert ops[k - 3:k] == [(WAIT, 0, 3 + 1, 3), (RECORD, 0, 7, 3), (WAIT, 1, 7, 3)]      # stream 0 waits and re-records
    assert ops[launch_pos[6] - 1] == (WAIT, 2, 3 + 2, 6)                                    # the upward wait is direct
    for i, j in [(1, 2), (2, 3), (3, 6), (4, 5), (0, 6), (1, 6)]:
        assert after[launch_pos[i]] >> j & 1, (i, j)
    # one stream: the program is the launches in order, no event at all
    rc, ops, nev = build_ops(hip_lib, [(i, 0, False, []) for i in range(4)], 1, 1)
    assert rc == 0 and ops == [(LAUNCH, 0, i, i) for i in range(4)] and nev == 1


ABSORBED = [(0, 0, False, []), (1, 0, True, []), (2, 2, True, [1]), (3, 1, True, [2]), (None, 1, True, []), (4, 0, False, [4]),
            (5, 2, False, [3])]
# ... and with entries that have no op at all (absorbed, no record, no wait): in the middle (2) and behind everything (8)
OPLESS = [(0, 0, False, []), (1, 0, True, []), (None, 0, False, []), (2, 2, True, [1]), (3, 1, True, [3]), (None, 1, True, []),
          (4, 0, False, [5]), (5, 2, False, [4]), (None, 2, False, [])]


def test_absorbed_entry_still_records_at_its_place(hip_lib):
    """(f) entry 4 (records, no waits) absorbed into an earlier launch of its stream: no LAUNCH, its RECORD stays behind the
    absorbing launch on the same stream, and the waiter is still ordered behind that launch."""
    table = ABSORBED
    rc, ops, nev = build_ops(hip_lib, table, 3, 1)
    assert rc == 0
    launch_pos, after, relays = check_program(ops, nev, table, 3, 1)
    assert 4 not in launch_pos and relays == 1
    rec = [k for k, o in enumerate(ops) if o[0] == RECORD and o[3] == 4]
    assert len(rec) == 1 and ops[rec[0]][1] == 1 and rec[0] > launch_pos[3]
    assert not any(o[0] == LAUNCH and o[1] == 1 for o in ops[launch_pos[3] + 1:rec[0]])
    assert after[launch_pos[3]] >> 5 & 1                           # entry 5 waits for the event: ordered behind the absorbing launch


# ---- what Python enqueues: the walker, and BoundPlan.launch_all over it ----------------------------------------------------------

def walk(ops, nentries):
    """schedule.run_program over `ops` with recording callbacks -> the log: ops as the walker handed them out, ('before', i)"""
    log = []
    schedule.run_program(ops, lambda e, s: log.append((LAUNCH, s, e)), lambda ev, s: log.append((RECORD, s, ev)),
                         lambda ev, s: log.append((WAIT, s, ev)), lambda i: log.append(('before', i)), nentries)
    return log


@pytest.mark.parametrize('case', PLANS + ['hand', 'absorbed', 'opless', 'one stream'], ids=str)
def test_walker_hands_out_the_program_one_for_one(case, hip_lib):
    if isinstance(case, tuple):
        plan = get_plan(*case)
        entries, ns, npre = schedule.schedule_entries(plan.steps), plan.nstreams, 0
    else:
        entries, ns, npre = {'hand': (HAND, 3, 1), 'absorbed': (ABSORBED, 3, 1), 'opless': (OPLESS, 3, 1),
                             'one stream': ([(0, 0, False, []), (None, 0, False, []), (1, 0, False, []), (None, 0, False, [])], 1, 1)}[case]
    ops, nev = _lib.sched_program(hip_lib, entries, ns, npre)
    assert (0, ops, nev) == build_ops(hip_lib, entries, ns, npre)
    log = walk(ops, len(entries))
    # same kind, stream, event id / entry, in order (a LAUNCH is handed out by entry: the step is the caller's to look up)
    assert [o for o in log if o[0] != 'before'] == [(k, s, e if k == LAUNCH else a) for k, s, a, e in ops]
    # `before`: once per entry, in increasing order, no later than the entry's first LAUNCH / RECORD -- and in front of the join
    assert [o[1] for o in log if o[0] == 'before'] == list(range(len(entries)))
    seen, at = set(), 0
    for o in log:
        if o[0] == 'before':
            seen.add(o[1])
            continue
        kind, stream, arg, entry = ops[at]
        at += 1
        assert entry < 0 or kind == WAIT or entry in seen, ('op of an entry in front of its hook', at - 1, entry)
        if at > len(ops) - 2 * (ns - 1):
            assert len(seen) == len(entries), 'a hook behind the join'
    opless = [i for i, e in enumerate(entries) if e[0] is None and not e[2] and not e[3]]
    assert not any(o[3] in opless for o in ops) and (case not in ('opless', 'one stream') or len(opless) == 2)
    # without the hook nothing else changes
    plain = []
    schedule.run_program(ops, lambda e, s: plain.append((LAUNCH, s, e)), lambda ev, s: plain.append((RECORD, s, ev)),
                         lambda ev, s: plain.append((WAIT, s, ev)))
    assert plain == [o for o in log if o[0] != 'before']


def test_more_than_four_streams_are_refused_by_name(hip_lib):
    table = [(0, 0, True, [])] + [(k, k, False, [0]) for k in range(1, 5)]
    assert len(_lib.sched_program(hip_lib, table[:4], 4, 0)[0]) == 4 + 4 + 3 + 1 + 6
    with pytest.raises(_lib.DeepharHipError, match='at most 4 streams'):
        _lib.sched_program(hip_lib, table, 5, 0)


MAIN_STREAM, ROLE_STREAMS = 0x1000, {'head': 0x2000, 'comm': 0x3000, 'copy': 0x4000}


class RecordingLib:
    """stand-in for BoundPlan.lib without a device: stream and event calls are written down, the scheduler is the library's"""

    def __init__(self, lib):
        self.lib, self.trace, self.handles = lib, [], 0

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def _create(self, ref):
        self.handles += 1
        ref._obj.value = 0x10000 + 16 * self.handles
        return 0

    dh_event_create_sync = dh_stream_create = _create

    def dh_event_record(self, ev, stream):
        self.trace.append((RECORD, getattr(stream, 'value', stream), ev.value))
        return 0

    def dh_stream_wait_event(self, stream, ev):
        self.trace.append((WAIT, getattr(stream, 'value', stream), ev.value))
        return 0


def enqueue_trace(executor, lib, plan, npre=0, absorbed=()):
    """What `executor`.BoundPlan.launch_all enqueues for `plan` behind `npre` staging calls, the calls in `absorbed` being no-ops,
    as [(kind, stream index, entry | event)] with events numbered by their first RECORD.  No device: the BoundPlan is made
    without __init__, its library is a RecordingLib and the role streams are numbers."""
    rec = RecordingLib(lib)
    bp = executor.BoundPlan.__new__(executor.BoundPlan)
    steps = [executor._InputStep(None) for _ in range(npre)] + list(plan.steps)
    bp.lib, bp.plan, bp.npre, bp.device, bp.perturb, bp.graph, bp.noop_calls = rec, plan, npre, None, None, None, set(absorbed)
    bp.calls = [(executor._noop_launch, (), st) if i in bp.noop_calls else
                ((lambda stream, i=i: rec.trace.append((LAUNCH, getattr(stream, 'value', stream), i)) or 0), (), st)
                for i, st in enumerate(steps)]
    shared, executor.shared_stream = executor.shared_stream, lambda device, role: types.SimpleNamespace(cuda_stream=ROLE_STREAMS[role])
    try:
        bp.launch_all(MAIN_STREAM)
    finally:
        executor.shared_stream = shared
    streams = [MAIN_STREAM] + [st.value for st in getattr(bp, '_streams', None) or []]
    assert streams[1:] == list(ROLE_STREAMS.values())[:plan.nstreams - 1]      # the role streams first, in their order
    return canonical(rec.trace, streams.index)


def canonical(trace, stream_index=int):
    events, out = {}, []
    for kind, stream, arg in trace:
        if kind == RECORD:
            events.setdefault(arg, len(events))
        out.append((kind, stream_index(stream), arg if kind == LAUNCH else events[arg]))
    return out


# sha256 of repr(enqueue_trace(...)) and (ops, waits, relays), recorded from the last commit whose launch_all had loops of its own
# (fork / wait / relay / launch / record / join, and a second loop for one stream) instead of walking the library's program:
# that BoundPlan was driven by enqueue_trace exactly as here, and the order of stream and event calls has not moved since.
# Variant 'bare': the plan's steps; 'staged+absorbed': one staging call in front and call 1 + len(steps) // 2 absorbed.
RECORDED_TRACES = {
    ('spnet', 2, 'tail', 'bare'): ('ccf16f0cfd15caac507d95e86952beb58310429590f9b7131d043718e1d44e24', (173, 8, 0)),
    ('spnet', 2, 'tail', 'staged+absorbed'): ('6caec2e8da00231071019da6b35c083cd836c3655dbfeeaa63319f2e7e8fe6bd', (173, 8, 0)),
    ('spnet', 3, 'tail', 'bare'): ('15987810ff995705635021a564e88c2ffb74e2c578ad861799bb16cd54f1f344', (186, 15, 0)),
    ('spnet', 3, 'tail', 'staged+absorbed'): ('7eecdac31253b8fa102f622fe8e400916abf3145a0f85ec3080c6682c5943edd', (186, 15, 0)),
    ('spnet', 2, 'list', 'bare'): ('4539a13011445f161cbe8cab3903870cc615c7ee2b8c7320da533e57ec86b2b2', (243, 43, 0)),
    ('spnet', 2, 'list', 'staged+absorbed'): ('cd125bba18a81ea8559b8bfadff9f3412a71fee9246f8634e4f95934535923f5', (243, 43, 0)),
    ('reception', 2, 'list', 'bare'): ('902aa73d94456d0a1a1a85b974d7ecddb06d3a29382911de453beec2a42d7bd2', (99, 21, 0)),
    ('reception', 2, 'list', 'staged+absorbed'): ('668bb8c6bc76ff33bca5eb9fb1ed204cdb8257c029f5a2d3cbe1fa9f269896e9', (99, 21, 0)),
    ('reception', 3, 'list', 'bare'): ('d45d20e60166b986eb0137ce0c450e3e30779e44b3e7c22e4d6ce152b7f1a188', (111, 28, 4)),
    ('reception', 3, 'list', 'staged+absorbed'): ('308b6f523991fcb98d2bd237c8e8061792346121ee4d35e3fbdde30c593b69de', (111, 28, 4)),
    ('spnet', 1, 'tail', 'bare'): ('8b40093e16fc5325ea8d5a38939b41e77592042fc6fab1fccc3d16d4a784879c', (157, 0, 0)),
    ('spnet', 1, 'tail', 'staged+absorbed'): ('daa305846a546d5a0c484ffc6fc721ade9f6a832e4e673ad9ab950e0af0a7d2a', (157, 0, 0)),
    ('reception', 1, 'list', 'bare'): ('528dc9914e12bc9d3990e57d1dfd723fa56dd9c02a6584e45b62642a14857684', (57, 0, 0)),
    ('reception', 1, 'list', 'staged+absorbed'): ('8d250f0968a230427c6129eaf4ec051c16d5ba02bbd99f156fde4de115035fec', (57, 0, 0)),
}


def trace_case(kind, streams, policy, variant, hip_lib):
    from deephar_amd.engine import executor
    plan = get_plan(kind, streams, policy)
    assert plan.nstreams == streams
    npre, absorbed = (0, ()) if variant == 'bare' else (1, (1 + len(plan.steps) // 2,))
    trace = enqueue_trace(executor, hip_lib, plan, npre, absorbed)
    # what was enqueued is the library's program, one for one
    entries = schedule.schedule_entries([executor._InputStep(None)] * npre + list(plan.steps), npre, absorbed)
    ops, nev = _lib.sched_program(hip_lib, entries, streams, npre)
    assert trace == canonical([(k, s, e if k == LAUNCH else a) for k, s, a, e in ops])
    nrec = sum(1 for e in entries if e[2])
    nevents = len({o[2] for o in trace if o[0] == RECORD})          # fork + joins + recording entries + relays
    counts = (len(trace), sum(1 for o in trace if o[0] == WAIT), nevents - nrec - (streams if streams > 1 else 0))
    return hashlib.sha256(repr(trace).encode()).hexdigest(), counts


@pytest.mark.parametrize('variant', ['bare', 'staged+absorbed'])
@pytest.mark.parametrize('kind,streams,policy', PLANS)
def test_launch_all_enqueues_the_recorded_order_multi_stream(kind, streams, policy, variant, hip_lib):
    assert trace_case(kind, streams, policy, variant, hip_lib) == RECORDED_TRACES[kind, streams, policy, variant]


@pytest.mark.parametrize('variant', ['bare', 'staged+absorbed'])
@pytest.mark.parametrize('kind,streams,policy', [('spnet', 1, 'tail'), ('reception', 1, 'list')])
def test_launch_all_enqueues_the_recorded_order_one_stream(kind, streams, policy, variant, hip_lib):
    digest, counts = trace_case(kind, streams, policy, variant, hip_lib)
    assert (digest, counts) == RECORDED_TRACES[kind, streams, policy, variant]
    assert counts == (len(get_plan(kind, streams, policy).steps), 0, 0)          # the launches (one staged, one absorbed), no event


def test_malformed_tables_are_refused(hip_lib):
    ok = lambda: [list(e[:3]) + [list(e[3])] for e in HAND]
    assert build_ops(hip_lib, HAND, 3, 1)[0] == 0
    assert build_ops(hip_lib, [(i, 0, False, []) for i in range(3)], 0, 0)[0] == EINVAL            # nstreams 0
    assert build_ops(hip_lib, HAND, 5, 1)[0] == EINVAL                                               # nstreams 5
    assert build_ops(hip_lib, HAND, 4, 1)[0] == 0
    assert build_ops(hip_lib, HAND, 2, 1)[0] == EINVAL                                               # stream 2 of 2
    for mutate in [lambda t: t[2].__setitem__(1, 3),                  # a stream index out of range
                   lambda t: t[2].__setitem__(1, -1),
                   lambda t: t[2].__setitem__(3, [3]),                # a wait on a later entry
                   lambda t: t[2].__setitem__(3, [2]),                # ... on itself
                   lambda t: t[1].__setitem__(2, False),              # a wait on an entry without the record flag
                   lambda t: t[5].__setitem__(3, [1]),                # a wait on the same stream
                   lambda t: t[0].__setitem__(3, [0]),
                   lambda t: t[2].__setitem__(3, [-1]),
                   lambda t: t[3].__setitem__(0, 5)]:                 # steps out of order
        t = ok()
        mutate(t)
        assert build_ops(hip_lib, [tuple(e) for e in t], 3, 1)[0] == EINVAL, t
    # a staging entry with a wait / on a side stream
    small = [(0, 0, False, []), (1, 1, True, []), (2, 0, False, [1])]
    assert build_ops(hip_lib, small, 2, 3)[0] == EINVAL
    assert build_ops(hip_lib, small, 2, 2)[0] == EINVAL
    assert build_ops(hip_lib, small, 2, 1)[0] == 0
    assert build_ops(hip_lib, [(0, 0, True, [])] + small[1:], 2, 1)[0] == EINVAL                    # ... that records an event
    # inconsistent table sizes
    assert build_ops(hip_lib, HAND, 3, 1, nwaits=5)[0] == EINVAL
    assert build_ops(hip_lib, HAND, 3, 1, nwaits=3)[0] == EINVAL
    assert build_ops(hip_lib, HAND, 3, 1, wait_off=[0, 0, 0, 1, 2, 2, 4, 3])[0] == EINVAL
    assert build_ops(hip_lib, HAND, 3, 1, wait_off=[1, 1, 1, 1, 2, 2, 3, 4])[0] == EINVAL
    assert build_ops(hip_lib, HAND, 3, 8)[0] == EINVAL                                               # more staging entries than entries
    assert build_ops(hip_lib, HAND, 3, 1, nsteps=8)[0] == EINVAL
    assert build_ops(hip_lib, HAND, 3, 1, nsteps=6)[0] == EINVAL


# ---- the pack launch's host form --------------------------------------------------------------------------------------------

# (pixels per item, C, ld, channel offset into a NaN-filled slab, floats by which dst is moved off its 16-byte boundary)
PACK_SEGMENTS = [(16, 2, 2, 0, 0), (16, 1, 1, 0, 0), (16, 3, 4, 0, 0), (1, 15, 15, 0, 0), (1024, 16, 48, 0, 0), (1024, 16, 48, 16, 0),
                 (64, 4, 4, 0, 1), (64, 4, 6, 0, 0)]
GUARD_FLOATS = 8


def aligned(nfloats, fill):
    """float32 array of nfloats whose first element sits on a 64-byte boundary"""
    raw = np.empty(nfloats + 16, np.float32)
    a = raw[(-raw.ctypes.data // 4) % 16:][:nfloats]
    assert a.ctypes.data % 64 == 0
    a[:] = fill
    return a


def pack_case(segments, m, seed):
    """-> per segment (slab [npix, ld] NaN outside the view, channel offset, expected dense [npix, C], dst shift)"""
    rng = np.random.default_rng(seed)
    case = []
    for ppi, c, ld, coff, shift in segments:
        npix = ppi * m
        slab = aligned(npix * ld, np.nan).reshape(npix, ld)
        slab[:, coff:coff + c] = rng.standard_normal((npix, c)).astype(np.float32)
        case.append((slab, coff, np.ascontiguousarray(slab[:, coff:coff + c]), shift))
    return case


def out_table(case, src_ptrs, dst_ptrs):
    tab = (_lib.OutSeg * len(case))()
    for k, ((slab, coff, want, _), s, d) in enumerate(zip(case, src_ptrs, dst_ptrs)):
        tab[k].src, tab[k].dst, tab[k].npix, tab[k].C, tab[k].ld = s + 4 * coff, d, want.shape[0], want.shape[1], slab.shape[1]
    return tab


def check_packed(case, dsts, null=()):
    """every dst: guards before and behind untouched, payload == the view; a NULL segment's buffer untouched altogether"""
    for k, ((slab, coff, want, shift), d) in enumerate(zip(case, dsts)):
        lo = GUARD_FLOATS + shift
        if k in null:
            assert np.all(np.isnan(d)), ('unwanted segment written', k)
            continue
        assert np.array_equal(d[lo:lo + want.size].reshape(want.shape), want), k
        assert np.all(np.isnan(d[:lo])) and np.all(np.isnan(d[lo + want.size:])), ('guard floats', k)
        rest = np.ones(slab.shape[1], bool)
        rest[coff:coff + want.shape[1]] = False
        assert np.all(np.isnan(slab[:, rest])) and np.array_equal(slab[:, ~rest], want), ('the slab', k)


@pytest.mark.parametrize('m', [1, 3])
def test_pack_outputs_host_equals_numpy(m, hip_lib):
    case = pack_case(PACK_SEGMENTS, m, 40 + m)
    dsts = [aligned(want.size + 2 * GUARD_FLOATS + 4, np.nan) for _, _, want, _ in case]
    null = (3,)                                                     # one NULL dst in the middle
    ptrs = [None if k in null else d.ctypes.data + 4 * (GUARD_FLOATS + c[3]) for k, (c, d) in enumerate(zip(case, dsts))]
    tab = out_table(case, [c[0].ctypes.data for c in case], ptrs)
    assert hip_lib.dh_pack_outputs_host(tab, len(case)) == 0
    check_packed(case, dsts, null)
    # 70 one-channel segments of 4 pixels
    many = pack_case([(4, 1, 1 + k % 3, 0, 0) for k in range(70)], m, 50 + m)
    dsts = [aligned(want.size + 2 * GUARD_FLOATS + 4, np.nan) for _, _, want, _ in many]
    tab = out_table(many, [c[0].ctypes.data for c in many], [d.ctypes.data + 4 * GUARD_FLOATS for d in dsts])
    assert hip_lib.dh_pack_outputs_host(tab, len(many)) == 0
    check_packed(many, dsts)


def test_pack_outputs_refuses_bad_segments_and_answers_the_path(hip_lib):
    src, dst = aligned(64, 1.0), aligned(64, np.nan)
    for npix, c, ld in [(0, 1, 1), (4, 0, 1), (4, 2, 1), (-1, 1, 1), (1 << 41, 1, 1)]:
        tab = (_lib.OutSeg * 1)()
        tab[0].src, tab[0].dst, tab[0].npix, tab[0].C, tab[0].ld = src.ctypes.data, dst.ctypes.data, npix, c, ld
        assert hip_lib.dh_pack_outputs_host(tab, 1) == EINVAL, (npix, c, ld)
    tab = (_lib.OutSeg * 1)()
    tab[0].src, tab[0].dst, tab[0].npix, tab[0].C, tab[0].ld = None, dst.ctypes.data, 4, 1, 1
    assert hip_lib.dh_pack_outputs_host(tab, 1) == EINVAL and hip_lib.dh_pack_outputs_host(None, 1) == EINVAL
    assert hip_lib.dh_pack_outputs_host(None, 0) == 0 and np.all(np.isnan(dst))
    # 16 bytes per lane exactly when C and ld are multiples of 4 and both addresses are 16-byte aligned
    ok = (16, 48, 0x1000, 0x2000)
    assert hip_lib.dh_pack_outputs_vec4(*ok) == 1 and hip_lib.dh_pack_outputs_vec4(16, 48, 0x1040, 0x2000) == 1
    for k, bad in enumerate((15, 6, 0x1004, 0x2008)):
        args = list(ok)
        args[k] = bad
        assert hip_lib.dh_pack_outputs_vec4(*args) == 0, k


# ---- the exporter's keyword ---------------------------------------------------------------------------------------------------

def test_single_stream_exports_are_unchanged_by_the_keyword():
    """dump_plan's pure halves: without the keyword -- and for a one-stream plan with it -- no schedule section is written and
    the version is what blob_version always gave; with it a several-stream plan is version 5.  (The bytes of whole blobs are
    compared on a device: tests/test_gpu_plan_streams.py.)"""
    from deephar_amd import Model, parallel
    for fn in (serialize.dump_plan, serialize.dump_clip_plan, Model.export_plan, parallel.ShardedClipModel.export_clip_plan):
        assert inspect.signature(fn).parameters['multi_stream'].default is False
    ids = [0, 1, serialize.FUNCTIONS.index('dh_copy_channels_f32')]
    for extra, want in [([], 2), ([serialize.V3_FUNCTIONS], 3), ([len(serialize.FUNCTIONS)], 4)]:
        multi, single = reception_plan(2, 'list'), reception_plan(1, 'list')
        assert multi.nstreams == 2 and single.nstreams == 1
        for plan, flag in [(multi, False), (single, False), (single, True)]:
            section = serialize.schedule_section(plan.steps, plan.nstreams, multi_stream=flag)
            assert section == b'' and serialize.plan_version(ids + extra, section) == serialize.blob_version(ids + extra) == want
        section = serialize.schedule_section(multi.steps, multi.nstreams, multi_stream=True)
        assert section and serialize.plan_version(ids + extra, section) == serialize.SCHEDULE_VERSION == 5
    # entries of a bound plan: staging calls in front shift the waits, an absorbed call keeps its entry without a step
    class S:
        def __init__(self, stream, record, wait):
            self.stream, self.record, self.wait = stream, record, wait
    steps = [S(0, False, ()), S(0, True, []), S(1, False, [0]), S(1, True, []), S(0, False, [2])]
    assert schedule.schedule_entries(steps, npre=1, noop={3}) == \
        [(0, 0, False, []), (1, 0, True, []), (2, 1, False, [1]), (None, 1, True, []), (3, 0, False, [3])]
    assert unpack_section(serialize.pack_schedule(schedule.schedule_entries(steps, 1, {3}), 2, 1))[2] == \
        schedule.schedule_entries(steps, 1, {3})
