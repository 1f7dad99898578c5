"""Measure the crop-and-resize front end on one GPU; writes profiles/frontend_crop.json.

    python tools/bench_frontend.py [--out profiles/frontend_crop.json] [--frames 2048] [--reps 5]

(a) the crop launch alone: 64 jobs out of 720 x 1280 frames, seeded windows of 250 - 900 px -> 256 x 256, device events around
    `iters` launches after a warm-up; algorithmic bytes = clipped window area read + output written; GB/s and the share of the
    8.0 TB/s HBM roof.
    The same jobs through dh_crop_program_build_dev (the program built on the GPU: a layout launch and a table launch), the
    pair timed the same way: `build_dev_ms_per_pair`.
(b) the MPII workload of bench.py (ReceptionNet, 8 blocks, batch 64): Model.predict on pre-cropped uint8 frames,
    predict_from_frames with program='host' (a chunk's crop program built on the host and copied over) and with
    program='device' (only the chunk's jobs staged, the program built on the GPU), alternating in one process, `reps`
    repetitions each, wall clock per call; the differences are reported beside the spread of the baseline leg's repetitions.
(c) where PIL imports: Image.crop(box).resize((256, 256), BILINEAR) on this machine's CPU, one core, per frame -- the CPU
    baseline the front end replaces; the machine's core count is recorded with it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_GBS = 8000.0


def windows(rng, n, H, W):
    out = []
    for _ in range(n):
        side = int(rng.integers(250, 901))
        cx, cy = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((cx - side // 2, cy - side // 2, cx - side // 2 + side, cy - side // 2 + side))
    return np.array(out, dtype=int)


def clipped_area(b, H, W):
    return max(0, min(b[2], W) - max(b[0], 0)) * max(0, min(b[3], H) - max(b[1], 0))


def bench_launch(torch, iters=50, warmup=5):
    from deephar_amd import functional as F
    rng = np.random.default_rng(0)
    H, W, n = 720, 1280, 64
    frames = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(8)]
    boxes = windows(rng, n, H, W)
    jobs = [(j % len(frames), tuple(int(v) for v in boxes[j]), j % 2) for j in range(n)]
    out = torch.empty(n * 256 * 256 * 3, dtype=torch.uint8, device='cuda')
    for _ in range(warmup):
        F.crop_resize(frames, jobs, (256, 256), out=out, item_pitch=256 * 256 * 3)
    torch.cuda.synchronize()
    # time the launch only: the program is built and uploaded once
    import ctypes as C
    from deephar_amd import _lib
    lib = _lib.load()
    srcs = (_lib.CropSrc * len(frames))(*[_lib.CropSrc(t.data_ptr(), 3 * W, H, W) for t in frames])
    cj = (_lib.CropJob * n)(*[_lib.CropJob(s, b[0], b[1], b[2], b[3], f) for s, b, f in jobs])
    nbytes = C.c_size_t(0)
    _lib.check(lib.dh_crop_program_bytes(cj, n, len(frames), 256, 256, C.byref(nbytes)))
    host = torch.empty(nbytes.value, dtype=torch.uint8, pin_memory=True)
    t0 = time.perf_counter()
    _lib.check(lib.dh_crop_program_build_host(srcs, len(frames), cj, n, 256, 256, host.data_ptr(), nbytes.value))
    build_ms = (time.perf_counter() - t0) * 1e3
    prog = host.cuda()
    st = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        _lib.check(lib.dh_crop_resize_u8(prog.data_ptr(), n, 256, 256, out.data_ptr(), 256 * 256 * 3, st))
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / iters
    # the same program built on the device: both tables uploaded once, the launch pair timed like the crop launch
    cap = C.c_size_t(0)
    _lib.check(lib.dh_crop_program_max_bytes(n, len(frames), 256, 256, C.byref(cap)))
    srcs_dev = torch.from_numpy(np.frombuffer(bytes(srcs), np.uint8).copy()).cuda()
    jobs_dev = torch.from_numpy(np.frombuffer(bytes(cj), np.uint8).copy()).cuda()
    built = torch.zeros(cap.value, dtype=torch.uint8, device='cuda')
    status = torch.empty(n, dtype=torch.int32, device='cuda')

    def build_pair():
        _lib.check(lib.dh_crop_program_build_dev(srcs_dev.data_ptr(), len(frames), jobs_dev.data_ptr(), n, 256, 256, built.data_ptr(),
                                                 cap.value, status.data_ptr(), st))
    for _ in range(warmup):
        build_pair()
    torch.cuda.synchronize()
    same = bool((built[:nbytes.value] == prog).all()) and not bool(status.any())
    ev2 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    pair_iters = 40 * iters                                  # (a pair is microseconds: enough of them for a window of milliseconds)
    ev2[0].record()
    for _ in range(pair_iters):
        build_pair()
    ev2[1].record()
    torch.cuda.synchronize()
    pair_ms = ev2[0].elapsed_time(ev2[1]) / pair_iters       # back-to-back pairs on one stream: a rate, not one pair's latency
    read = sum(clipped_area(b, H, W) for b in boxes) * 3
    written = n * 256 * 256 * 3
    gbs = (read + written) / (ms * 1e-3) / 1e9
    return dict(jobs=n, source='720x1280', output='256x256', windows_px='250-900, seeded', iters=iters, ms_per_launch=ms,
                us_per_frame=ms * 1e3 / n, bytes_read=int(read), bytes_written=int(written), gb_per_s=gbs,
                share_of_hbm_roof=gbs / HBM_ROOF_GBS, program_bytes=int(nbytes.value), program_build_ms_host=build_ms,
                build_dev_ms_per_pair=pair_ms, build_dev_pairs_timed=pair_iters, build_dev_capacity_bytes=int(cap.value), build_dev_equals_host_program=same)


def bench_predict(torch, total, reps, batch=64, blocks=8):
    from bench import build_mpii
    from deephar_amd import frontend
    rng = np.random.default_rng(1)
    model = build_mpii(blocks)
    H, W = 720, 1280
    full = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(32)]
    index = np.arange(total) % len(full)
    boxes = windows(rng, total, H, W)
    store = frontend.FrameStore(full)
    crops = rng.integers(0, 256, (total, 256, 256, 3), dtype=np.uint8)            # pre-cropped frames: the baseline's input
    legs = {'predict_precropped_u8': lambda: model.predict(crops, batch_size=batch),
            'predict_from_frames': lambda: frontend.predict_from_frames(model, store, index, boxes, batch_size=batch),
            'predict_from_frames_program_device': lambda: frontend.predict_from_frames(model, store, index, boxes, batch_size=batch,
                                                                                       program='device')}
    for fn in legs.values():                                                     # bind, autotune, capture, staging
        fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():                                               # alternating in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    res = {'frames_per_leg': total, 'batch': batch, 'blocks': blocks, 'repetitions': reps}
    for k, ts in times.items():
        res[k] = dict(seconds=ts, frames_per_s=[total / t for t in ts], median_frames_per_s=total / float(np.median(ts)))
    base, front = times['predict_precropped_u8'], times['predict_from_frames']
    res['difference_ms_per_batch'] = (float(np.median(front)) - float(np.median(base))) / (total / batch) * 1e3
    res['baseline_spread_ms_per_batch'] = (max(base) - min(base)) / (total / batch) * 1e3
    res['front_end_relative_to_baseline'] = float(np.median(base)) / float(np.median(front))
    dev = times['predict_from_frames_program_device']
    res['program_device'] = {
        'difference_to_baseline_ms_per_batch': (float(np.median(dev)) - float(np.median(base))) / (total / batch) * 1e3,
        'difference_to_program_host_ms_per_batch': (float(np.median(dev)) - float(np.median(front))) / (total / batch) * 1e3,
        'relative_to_baseline': float(np.median(base)) / float(np.median(dev)),
        'relative_to_program_host': float(np.median(front)) / float(np.median(dev)),
        'ahead_of_program_host_by_more_than_the_baseline_spread':
            bool((float(np.median(front)) - float(np.median(dev))) > (max(base) - min(base)))}
    return res


def bench_pil(nframes=64):
    try:
        import PIL
        from PIL import Image
    except ImportError:
        return None
    rng = np.random.default_rng(0)
    H, W = 720, 1280
    img = Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    boxes = windows(rng, nframes, H, W)
    t0 = time.perf_counter()
    for b in boxes:
        np.asarray(img.crop(tuple(int(v) for v in b)).resize((256, 256), Image.BILINEAR))
    ms = (time.perf_counter() - t0) / nframes * 1e3
    return dict(label='CPU baseline: PIL crop().resize(BILINEAR) on one core of this machine', pillow=PIL.__version__,
                ms_per_frame=ms, frames=nframes, cpu_count=os.cpu_count())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frontend_crop.json'))
    ap.add_argument('--frames', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_frontend needs a HIP device'
    rec = {'device': torch.cuda.get_device_name(0), 'crop_launch': bench_launch(torch)}
    rec['mpii_predict'] = bench_predict(torch, args.frames, args.reps)
    step_ms = 64 / rec['mpii_predict']['predict_precropped_u8']['median_frames_per_s'] * 1e3
    rec['crop_share_of_step'] = rec['crop_launch']['ms_per_launch'] / step_ms
    rec['pil_cpu'] = bench_pil()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
