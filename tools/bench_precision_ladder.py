#!/usr/bin/env python
"""The GEMM precision ladder measured in ONE process: Model.gemm_precision = 'f32', 'bf16x3', 'bf16x2', 'bf16' on the same
model, batch, warm-up and timed window as the driver line of bench.py (its builders, its set-up routines and its `timed`),
the four modes ALTERNATING, several rounds -- so that a difference between two rungs is read against the run-to-run spread
of the same process on the same card, not against a number from an older record.

    python tools/bench_precision_ladder.py [--workloads mpii,h36m,ntu_spnet] [--rounds 5] [--out profiles/precision_ladder.json]

mpii is timed like `bench.py --gpus 1 --steps 20 --warmup 3` (batch 64); h36m / ntu_spnet like the compact legs bench.py
appends to its line (10 steps after 3 warm-up steps, one GPU).  Also: the main launch shape (65 536 x 576 x 576, ReLU
prologue, BN + residual epilogue) per mode, best tiling, HIP events.

bench.py's own line labels its `dtype` field for ANY split mode as the three-part split (only its `gemm` field names the
mode that ran): records of the reduced modes come from this tool."""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                    # noqa: E402

MODES = ('f32', 'bf16x3', 'bf16x2', 'bf16')


def setup(workload, mode):
    """One resident, bound and tuned instance of `workload` in `mode` -> (step, streams, pairs, frames per step)."""
    wl = bench.WORKLOADS[workload]
    a = types.SimpleNamespace(no_graph=False, input='f32', force_cfg=None, force_collective=False, no_overlap=False)
    model = wl['build']()
    model.gemm_precision = mode
    if wl['clips']:
        step, pairs, bound, streams, frames, flops, check, par, restage = bench.setup_clips(workload, model, wl['per_gpu'], 1, 0, a)
        scm = bench.LAST_SCM[0]
        plans = [scm.frame_model.plan, scm.head_model.plan]
    else:
        step, bound, streams, frames, flops, check, restage = bench.setup_frame_workload(model, wl['per_gpu'], wl['T'], a, 1, 0)
        pairs = None
        plans = [model.plan]
    nsplit = sum(1 for p in plans for s in p.steps if s.kind == 'conv' and s.attrs.get('w_split') in (1, 3, 4))
    return dict(step=step, streams=streams, pairs=pairs, frames=frames, check=check, split_convs=nsplit, keep=(model, bound))


def ladder(workload, steps, warmup, rounds):
    import torch
    inst = {m: setup(workload, m) for m in MODES}
    fps = {m: [] for m in MODES}
    for r in range(rounds):
        for m in (MODES if r % 2 == 0 else MODES[::-1]):        # alternate, and alternate the order
            i = inst[m]
            dt = bench.timed(i['step'], i['streams'], steps, warmup, 1, i['pairs'])
            fps[m].append(i['frames'] * steps / dt)
    out = {'workload': bench.WORKLOADS[workload]['name'], 'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'frames_per_step': inst['f32']['frames'], 'modes': {}}
    for m in MODES:
        v = fps[m]
        med = statistics.median(v)
        pose = inst[m]['check']()
        out['modes'][m] = {'frames_per_s_median': round(med, 1), 'frames_per_s_rounds': [round(x, 1) for x in v],
                           'spread_fraction': round((max(v) - min(v)) / med, 4), 'split_convs': inst[m]['split_convs'],
                           'outputs_finite': bool(np.all(np.isfinite(pose)))}
    base = out['modes']['bf16x3']['frames_per_s_median']
    for m in MODES:
        out['modes'][m]['vs_bf16x3'] = round(out['modes'][m]['frames_per_s_median'] / base, 4)
    order = ('bf16x3', 'bf16x2', 'bf16')
    out['rungs'] = []
    for above, below in zip(order, order[1:]):
        a, b = out['modes'][above], out['modes'][below]
        gain = b['frames_per_s_median'] / a['frames_per_s_median'] - 1.0
        spread = max(a['spread_fraction'], b['spread_fraction'])
        out['rungs'].append({'rung': below, 'above': above, 'gain_fraction': round(gain, 4), 'spread_fraction': spread,
                             'faster_by_more_than_spread': bool(gain > spread)})
    del inst
    torch.cuda.empty_cache()
    return out


def main_shape(reps=30):
    """65 536 x 576 x 576 (64 frames of 32 x 32, ReLU prologue, BN + residual): per mode the fastest tiling, HIP events."""
    import torch
    from deephar_amd import _lib, functional as F
    from deephar_amd.engine import packing
    lib = _lib.load()
    rng = np.random.default_rng(0)
    dev = torch.device('cuda:0')
    x = torch.from_numpy(rng.uniform(-1, 1, (64, 32, 32, 576)).astype(np.float32)).to(dev)
    r1 = torch.from_numpy(rng.uniform(-1, 1, (64, 32, 32, 576)).astype(np.float32)).to(dev)
    k = (rng.standard_normal((1, 1, 576, 576)) / 24.0).astype(np.float32)
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, 576).astype(np.float32)).to(dev)
    sh = torch.zeros(576, device=dev)
    out = {'shape_mkn': [65536, 576, 576], 'epilogue': 'relu prologue, BN, one residual', 'reps': reps, 'modes': {}}
    for m in MODES:
        if m == 'f32':
            pk, kp, np_ = packing.pack_conv(k)
            ncfg = lib.dh_conv2d_num_tile_cfgs()
        else:
            pk, kp, np_ = packing.pack_conv_split(k, parts={'bf16x3': 3, 'bf16x2': 2, 'bf16': 1}[m])
            ncfg = lib.dh_conv2d_num_split_tile_cfgs()
        packed = (torch.from_numpy(pk).to(dev), kp, np_)
        run = lambda cfg: F.conv2d(x, k, pre_relu=True, post_scale=sc, post_shift=sh, res1=r1, packed=packed, tile_cfg=cfg,
                                   precision=m)
        times = {}
        for cfg in range(ncfg):
            try:
                run(cfg)
            except _lib.DeepharHipError as e:
                if 'rc=-2' not in str(e):
                    raise
                continue
            best = float('inf')
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run(cfg)
                e1.record()
                e1.synchronize()
                best = min(best, 1e3 * e0.elapsed_time(e1) / reps)
            times[cfg] = round(best, 2)
        cfg = min(times, key=times.get)
        out['modes'][m] = {'best_tile_cfg': cfg, 'us_per_launch': times[cfg], 'us_per_tile_cfg': times,
                           'tflops': round(2 * 65536 * 576 * 576 / times[cfg] / 1e6, 1)}
    out['note'] = 'eager launches back to back (host-side argument marshalling included: an upper bound for the short ones)'
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--workloads', default='mpii,h36m,ntu_spnet')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20, help='mpii: timed steps per round (the driver line\'s window)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-main-shape', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'precision_ladder.json'))
    args = ap.parse_args()
    import torch
    res = {'tool': 'tools/bench_precision_ladder.py', 'device': torch.cuda.get_device_name(0),
           'protocol': 'four modes alternating inside one process; median over rounds; spread = (max - min) / median; '
                       'baseline = bf16x3 of the same process', 'workloads': {}}
    for w in [v for v in args.workloads.split(',') if v]:
        compact = w != 'mpii'
        res['workloads'][w] = ladder(w, 10 if compact else args.steps, args.warmup, args.rounds)
        print(json.dumps({w: res['workloads'][w]}), flush=True)
    if not args.no_main_shape:
        res['main_shape'] = main_shape()
        print(json.dumps({'main_shape': res['main_shape']}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
