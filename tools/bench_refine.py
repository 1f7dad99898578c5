"""Measure the box-refinement loop on one GPU; writes profiles/refine_loop.json.

    python tools/bench_refine.py [--out profiles/refine_loop.json] [--samples 512] [--reps 5]

The MPII workload of bench.py (ReceptionNet, 8 blocks, batch 64) under evaltools.refine_pred_frames over 720 x 1280 frames,
three legs alternating in one process, `reps` repetitions each, wall clock per call, at num_iter = 2 and then 3:
    loop='host',  program='host'    every iteration drains, blends the boxes in Python, builds the crop programs on the host
    loop='host',  program='device'  the same loop, the crop programs built on the GPU from staged jobs
    loop='device'                   the boxes stay on the GPU: dh_refine_boxes_f64 behind every forward, no drain between iterations
Reported per leg: frames/s (samples x num_iter per second) of every repetition and their median; per pair of legs the ratio of
the medians and whether the difference of the medians is outside the repetition spread (max - min) of the loop='host' legs.
The weights are synthetic: the poses, and with them the windows, are whatever such a network gives; a run in which a window
dies (empty, or beyond the scale cap) is recorded as refused, for every leg alike.  The device loop's poses are compared with
the host loop's once per num_iter (np.array_equal) and the answer is recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def boxes0(rng, n, H, W):
    cx, cy = rng.uniform(0.2 * W, 0.8 * W, n), rng.uniform(0.2 * H, 0.8 * H, n)
    side = rng.uniform(250.3, 900.7, n)
    return np.stack([cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2], axis=1)


def bench_loop(torch, total, reps, batch=64, blocks=8):
    from bench import build_mpii
    from deephar_amd import frontend
    from deephar_amd.evaltools import mpii_tools
    rng = np.random.default_rng(1)
    model = build_mpii(blocks)
    outidx = max(k for k, v in enumerate(model.outputs) if len(v.shape) == 2 and v.shape[-1] >= 2)
    H, W = 720, 1280
    store = frontend.FrameStore([rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(total)])
    bbox0 = boxes0(rng, total, H, W)
    res = {'samples': total, 'batch': batch, 'blocks': blocks, 'repetitions': reps, 'frames': '720x1280', 'outidx': outidx}
    for num_iter in (2, 3):
        kw = dict(num_iter=num_iter, batch_size=batch)
        legs = {'loop_host_program_host': lambda: mpii_tools.refine_pred_frames(model, store, bbox0, outidx, **kw),
                'loop_host_program_device': lambda: mpii_tools.refine_pred_frames(model, store, bbox0, outidx, program='device', **kw),
                'loop_device': lambda: mpii_tools.refine_pred_frames(model, store, bbox0, outidx, loop='device', **kw)}
        rec = res['num_iter_%d' % num_iter] = {}
        try:                                                                      # bind, autotune, capture, staging; and the bits
            first = {k: fn() for k, fn in legs.items()}
        except (ValueError, ZeroDivisionError) as e:                              # (a window of no width divides by zero on the host)
            rec['refused'] = repr(e)
            continue
        rec['loop_device_equals_loop_host'] = all(np.array_equal(a, b) for a, b in zip(first['loop_device'], first['loop_host_program_host']))
        times = {k: [] for k in legs}
        for _ in range(reps):
            for k, fn in legs.items():                                           # alternating in one process
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        work = total * num_iter
        for k, ts in times.items():
            rec[k] = dict(seconds=ts, frames_per_s=[work / t for t in ts], median_frames_per_s=work / float(np.median(ts)),
                          spread_frames_per_s=work / min(ts) - work / max(ts))
        med = {k: float(np.median(ts)) for k, ts in times.items()}
        host_spread = max(max(times[k]) - min(times[k]) for k in ('loop_host_program_host', 'loop_host_program_device'))
        rec['host_legs_spread_seconds'] = host_spread
        for a, b in [('loop_device', 'loop_host_program_host'), ('loop_device', 'loop_host_program_device'),
                     ('loop_host_program_device', 'loop_host_program_host')]:
            rec['%s_over_%s' % (a, b)] = dict(ratio_frames_per_s=med[b] / med[a], difference_seconds=med[b] - med[a],
                                              difference_us_per_sample_and_iteration=(med[b] - med[a]) / work * 1e6,
                                              outside_the_spread=bool(abs(med[b] - med[a]) > host_spread))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refine_loop.json'))
    ap.add_argument('--samples', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_refine needs a HIP device'
    rec = {'device': torch.cuda.get_device_name(0), 'refine_loop': bench_loop(torch, args.samples, args.reps)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
