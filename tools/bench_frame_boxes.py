"""Measure the per-frame person-box pass on one GPU; writes profiles/frame_boxes.json.

    python tools/bench_frame_boxes.py [--out profiles/frame_boxes.json] [--samples 512] [--reps 5]

The MPII workload of bench.py (ReceptionNet, 8 blocks) over 720 x 1280 frames, three legs alternating in one process, `reps`
repetitions each, wall clock per call:
    reference_shape   the pass of evaltools.bbox.predict_frame_bboxes: one model.predict of ONE pre-cropped frame per sample, the
                      whole pose output to the host, get_bbox_from_poses there (the crops are made beforehand and not timed)
    loop_host         predict_frame_bboxes_frames(loop='host') at batch 64: crops on the GPU, packed outputs to the host, the
                      same Python chain per sample
    loop_device       predict_frame_bboxes_frames(loop='device') at batch 64: dh_pose_boxes_f64 behind every forward, 52 bytes
                      per sample to the host
Reported per leg: frames/s of every repetition, their median and the spread between repetitions; per pair of legs the ratio of
the medians and whether the difference of the medians is outside the repetition spread (max - min, in seconds) of the slower
leg of the pair.  Separately: dh_pose_boxes_f64 alone, 2 000 launches back to back on one stream between two device events.
The weights are synthetic: the poses are whatever such a network gives; a sample whose pose keeps no joint is recorded as
refused, for every leg alike.  The device loop's dictionary is compared with the host loop's once and the answer recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows0(rng, n, H, W):
    cx, cy = rng.uniform(0.2 * W, 0.8 * W, n), rng.uniform(0.2 * H, 0.8 * H, n)
    side = rng.uniform(250.3, 900.7, n)
    return np.stack([cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2], axis=1).astype(np.int64)


def bench_pass(torch, total, reps, batch=64, blocks=8):
    from bench import build_mpii
    from deephar_amd import frontend
    from deephar_amd.evaltools.bbox import get_bbox_from_poses, predict_frame_bboxes_frames
    rng = np.random.default_rng(1)
    model = build_mpii(blocks)
    outidx = max(k for k, v in enumerate(model.outputs) if len(v.shape) == 2 and v.shape[-1] >= 2)
    H, W = 720, 1280
    store = frontend.FrameStore([rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(total)])
    windows = windows0(rng, total, H, W)
    index = np.arange(total)
    keys = ['0.%d' % i for i in range(total)]
    OH, OW = model.inputs[0].shape[0], model.inputs[0].shape[1]
    res = {'samples': total, 'batch': batch, 'blocks': blocks, 'repetitions': reps, 'frames': '720x1280', 'outidx': outidx}
    # the reference shape's inputs: the same crops, made once (cropped on the GPU, copied out), and their affine maps
    from deephar_amd import functional as Fn
    jobs = [(i, tuple(int(v) for v in windows[i]), False) for i in range(total)]
    crops = np.concatenate([Fn.crop_resize(store.tensors, jobs[a:a + batch], (OH, OW)).cpu().numpy() for a in range(0, total, batch)])
    afmat = [frontend.crop_afmat(w, (OW, OH)) for w in windows]

    def reference_shape():
        out = {}
        for i in range(total):
            poses = model.predict(crops[i:i + 1])
            poses = poses[outidx] if isinstance(poses, (list, tuple)) else poses
            out[keys[i]] = get_bbox_from_poses(poses, afmat[i], scale=1.5).astype(int).tolist()
        return out

    kw = dict(batch_size=batch, outidx=outidx)
    legs = {'reference_shape': reference_shape,
            'loop_host': lambda: predict_frame_bboxes_frames(model, store, index, windows, keys, loop='host', **kw),
            'loop_device': lambda: predict_frame_bboxes_frames(model, store, index, windows, keys, loop='device', **kw)}
    try:                                                                          # bind, autotune, capture; and the boxes
        first = {k: fn() for k, fn in legs.items()}
    except ValueError as e:
        res['refused'] = repr(e)
        return res
    res['loop_device_equals_loop_host'] = first['loop_device'] == first['loop_host']
    res['reference_shape_equals_loop_host'] = first['reference_shape'] == first['loop_host']
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():                                               # alternating in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    for k, ts in times.items():
        res[k] = dict(seconds=ts, frames_per_s=[total / t for t in ts], median_frames_per_s=total / float(np.median(ts)),
                      spread_seconds=max(ts) - min(ts), spread_frames_per_s=total / min(ts) - total / max(ts))
    med = {k: float(np.median(ts)) for k, ts in times.items()}
    for a, b in [('loop_device', 'loop_host'), ('loop_device', 'reference_shape'), ('loop_host', 'reference_shape')]:
        spread = max(max(times[k]) - min(times[k]) for k in (a, b))
        res['%s_over_%s' % (a, b)] = dict(ratio_frames_per_s=med[b] / med[a], difference_seconds=med[b] - med[a],
                                          difference_us_per_sample=(med[b] - med[a]) / total * 1e6, spread_seconds=spread,
                                          outside_the_spread=bool(abs(med[b] - med[a]) > spread))
    return res


def bench_launch(torch, launches=2000, n=64, J=16, D=3):
    """dh_pose_boxes_f64 alone: `launches` launches back to back on one stream, timed with device events"""
    from deephar_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2)
    poses = torch.from_numpy(rng.uniform(0.3, 0.9, (n, J, D)).astype(np.float32)).cuda()
    jobs = np.zeros((n, 6), np.int32)
    jobs[:, 1:5] = windows0(rng, n, 720, 1280)
    jobs = torch.from_numpy(jobs).cuda()
    box = torch.empty((n, 4), dtype=torch.int32, device='cuda')
    boxf = torch.empty((n, 4), dtype=torch.float64, device='cuda')
    status = torch.empty((n,), dtype=torch.int32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.dh_pose_boxes_f64(poses.data_ptr(), J * D, J * D, D, 1, J, D - 2, jobs.data_ptr(), 1, n, 1.5, box.data_ptr(),
                                         boxf.data_ptr(), status.data_ptr(), st), 'dh_pose_boxes_f64')
    for _ in range(50):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / launches)
    return dict(items=n, joints=J, channels=D, launches=launches, us_per_launch=us, median_us_per_launch=float(np.median(us)),
                all_ok=bool((status.cpu().numpy() == 0).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frame_boxes.json'))
    ap.add_argument('--samples', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_frame_boxes needs a HIP device'
    rec = {'device': torch.cuda.get_device_name(0), 'frame_boxes': bench_pass(torch, args.samples, args.reps),
           'dh_pose_boxes_f64': bench_launch(torch)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
