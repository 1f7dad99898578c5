"""The C executor in the latency regime: what dh_forward costs per call on the protocol's last model, with one stream and with
the engine's two-stream 'tail' schedule, against the PARENT commit's library -- profiles/c_plan_streams.json, DESIGN 3.5.

  model    exp/pennaction/eval_speed2d.py:31-36's configuration (bench.build_speed2d), Model(full.input, full.outputs[34:36]),
           synthetic weights, 2 clips per call
  exports  one stream (the blob every commit writes) and two streams 'tail' with multi_stream=True (blob version 5)
  timed    dh_forward per call, HIP events around it on the caller's stream, device pointers, after warm-up; the variants
           alternate call by call in ONE process; median of --calls calls each
  parent   the parent commit's executor on the one-stream blob -- TWICE (two plans, timed like two variants): the spread between
           the two is the margin of every comparison below.  Its library is this tree's objects with the parent's plan.hip:
             git show HEAD~1:deephar_amd/csrc/plan.hip > /tmp/plan_parent.hip
             python tools/build_variant.py /tmp/plan_parent.hip /tmp/libdeephar_parent.so
           (--parent-plan-hip does the second line itself; --parent-lib takes the result)
  reported two streams (version 5) against the parent, and one stream through THIS library against the parent: the latter
           isolates what the single pack launch at the end of a forward saves over one copy launch per output; it must not be
           slower than the parent by more than the spread.

The export runs in a child process: the Python engine opens its four role streams (engine/executor.py: shared_stream), and a
process that times a C host must not hold them -- the plan's side stream would share a hardware queue with one of them.  The
timing process opens the caller's stream and what the plans open themselves."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def export(outdir):
    import bench
    from deephar_amd import Model
    from deephar_amd.engine.serialize import dump_plan
    full = bench.build_speed2d()
    one = Model(full.input, full.outputs[34:36])
    two = Model(full.input, full.outputs[34:36])
    two.num_streams, two.stream_policy = 2, 'tail'
    blob1 = dump_plan(one, 2)
    two.executor.tune_table = one.executor.tune_table
    blob2 = dump_plan(two, 2, multi_stream=True)
    assert two.plan.nstreams == 2 and blob2[4] == 5 and blob1[4] < 5
    open(os.path.join(outdir, 'one.dhplan'), 'wb').write(blob1)
    open(os.path.join(outdir, 'two.dhplan'), 'wb').write(blob2)
    json.dump({'launches_one': len(one.executor.bound[2].calls) - len(one.executor.bound[2].noop_calls),
               'launches_two': len(two.executor.bound[2].calls) - len(two.executor.bound[2].noop_calls),
               'waits_two': sum(len(s.wait) for s in two.plan.steps), 'outputs': len(one.outputs)},
              open(os.path.join(outdir, 'info.json'), 'w'))


def plan_api(lib):
    vp = C.c_void_p
    lib.dh_plan_create.argtypes, lib.dh_plan_create.restype = [vp, C.c_size_t, C.POINTER(vp)], C.c_int
    lib.dh_plan_destroy.argtypes, lib.dh_plan_destroy.restype = [vp], C.c_int
    lib.dh_forward.argtypes, lib.dh_forward.restype = [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), vp], C.c_int
    lib.dh_plan_output_items.argtypes, lib.dh_plan_output_items.restype = [vp, C.c_int], C.c_int64
    lib.dh_plan_num_outputs.argtypes, lib.dh_plan_num_outputs.restype = [vp], C.c_int
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--phase', default='time', choices=['time', 'export'])
    ap.add_argument('--dir', default=None, help='where the two blobs are written / read (default: a temporary directory)')
    ap.add_argument('--parent-lib', default=None, help='the parent commit\'s library (tools/build_variant.py)')
    ap.add_argument('--parent-plan-hip', default=None, help='the parent commit\'s csrc/plan.hip: the library is built from it')
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'c_plan_streams.json'))
    a = ap.parse_args()
    if a.phase == 'export':
        return export(a.dir)
    if a.calls < 200:
        ap.error('--calls: the median is taken over at least 200 calls')
    work = a.dir or tempfile.mkdtemp(prefix='c_plan_streams_')
    os.makedirs(work, exist_ok=True)
    if a.parent_lib is None:
        if a.parent_plan_hip is None:
            ap.error('--parent-lib or --parent-plan-hip: the baseline is the parent commit\'s executor')
        a.parent_lib = os.path.join(work, 'libdeephar_parent.so')
        subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'build_variant.py'), a.parent_plan_hip, a.parent_lib], check=True)
    subprocess.run([sys.executable, os.path.abspath(__file__), '--phase', 'export', '--dir', work], check=True)

    import numpy as np
    import torch
    from deephar_amd import _lib
    new = _lib.load()
    parent = plan_api(C.CDLL(os.path.abspath(a.parent_lib)))
    blobs = {k: open(os.path.join(work, k + '.dhplan'), 'rb').read() for k in ('one', 'two')}
    info = json.load(open(os.path.join(work, 'info.json')))
    variants = [('parent_a', parent, 'one'), ('new_one_stream', new, 'one'), ('parent_b', parent, 'one'), ('new_two_streams', new, 'two')]
    plans = {}
    for name, lib, blob in variants:
        h = C.c_void_p()
        assert lib.dh_plan_create(blobs[blob], len(blobs[blob]), C.byref(h)) == 0, name
        plans[name] = h
    assert new.dh_plan_num_streams(plans['new_two_streams']) == 2 and new.dh_plan_num_streams(plans['new_one_stream']) == 1
    dev = torch.device('cuda:0')
    x = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (2, 8, 256, 256, 3)).astype(np.float32)).to(dev)
    nout = new.dh_plan_num_outputs(plans['new_one_stream'])
    outs = {name: [torch.full((2 * new.dh_plan_output_items(plans['new_one_stream'], k),), float('nan'), device=dev)
                   for k in range(nout)] for name, _, _ in variants}
    stream = C.c_void_p()
    _lib.check(new.dh_stream_create(C.byref(stream)))
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(new.dh_event_create(C.byref(e0)))
    _lib.check(new.dh_event_create(C.byref(e1)))
    torch.cuda.synchronize()
    ins = (C.c_void_p * 1)(x.data_ptr())
    outs_p = {name: (C.c_void_p * nout)(*[o.data_ptr() for o in outs[name]]) for name in outs}
    times = {name: [] for name, _, _ in variants}
    ms = C.c_float()
    for it in range(a.warmup + a.calls):
        for name, lib, _ in variants:
            _lib.check(new.dh_event_record(e0, stream))
            rc = lib.dh_forward(plans[name], ins, 2, outs_p[name], stream)
            _lib.check(new.dh_event_record(e1, stream))
            _lib.check(new.dh_event_synchronize(e1))
            assert rc == 0, (name, rc)
            _lib.check(new.dh_event_elapsed_ms(e0, e1, C.byref(ms)))
            if it >= a.warmup:
                times[name].append(ms.value)
    _lib.check(new.dh_stream_synchronize(stream))
    want = [o.cpu().numpy() for o in outs['parent_a']]
    same = {name: all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs[name], want)) for name in outs}
    for name, lib, _ in variants:
        lib.dh_plan_destroy(plans[name])
    new.dh_event_destroy(e0)
    new.dh_event_destroy(e1)
    new.dh_stream_destroy(stream)
    med = {name: statistics.median(t) for name, t in times.items()}
    p10 = {name: sorted(t)[len(t) // 10] for name, t in times.items()}
    parent_ms = 0.5 * (med['parent_a'] + med['parent_b'])
    spread = abs(med['parent_a'] - med['parent_b'])
    res = {
        'what': 'dh_forward per call, HIP events on the caller\'s stream, device pointers; speed2d last model (outputs 34-35), '
                '2 clips per call, synthetic weights; variants alternate call by call in one process',
        'device': torch.cuda.get_device_name(0), 'calls': a.calls, 'warmup': a.warmup,
        'launches_per_forward': {'parent_one_stream': info['launches_one'] + info['outputs'], 'new_one_stream': info['launches_one'] + 1,
                                 'new_two_streams': info['launches_two'] + 1},
        'event_waits_two_streams': info['waits_two'],
        'median_ms': {k: round(v, 4) for k, v in med.items()}, 'p10_ms': {k: round(v, 4) for k, v in p10.items()},
        'parent_ms': round(parent_ms, 4), 'parent_spread_ms': round(spread, 4),
        'new_one_stream_minus_parent_ms': round(med['new_one_stream'] - parent_ms, 4),
        'new_two_streams_minus_parent_ms': round(med['new_two_streams'] - parent_ms, 4),
        'one_stream_not_slower_than_parent_within_spread': bool(med['new_one_stream'] <= max(med['parent_a'], med['parent_b']) + spread),
        'two_streams_beat_one_stream': bool(med['new_two_streams'] < med['new_one_stream']),
        'bit_identical_to_parent': same,
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    assert all(same.values()), same


if __name__ == '__main__':
    main()
