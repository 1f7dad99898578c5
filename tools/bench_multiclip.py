"""Measure the multi-clip action vote on one GPU; writes profiles/multiclip_votes.json.

    python tools/bench_multiclip.py [--out profiles/multiclip_votes.json] [--sequences 64] [--clips 3] [--reps 5]

The PennAction merge model of bench.py's penn_merge workload (16-frame clips, 4 blocks, 15 actions) over 720 x 1280 frames:
`sequences` test sequences of `clips` hop windows each, every clip as it is and mirrored, one window per clip.  Three legs
alternate in one process, `reps` repetitions each, wall clock per call:
    reference_shape   the loop of evaltools.action._multiclip: one model.predict of ONE pre-cropped clip per item, all outputs to
                      the host, the product there (the crops are made beforehand and not timed)
    loop_host         multiclip_votes_frames(loop='host') at the workload's batch of 4 clips: crops on the GPU, packed outputs to
                      the host, vote_products there
    loop_device       multiclip_votes_frames(loop='device') at batch 4: dh_vote_products_f64 behind every forward, the products
                      and labels to the host once
Reported per leg: clips/s of every repetition, their median and the spread between repetitions; per pair of legs the ratio of
the medians and whether the difference of the medians is outside the repetition spread (max - min, in seconds) of the noisier
leg of the pair.  Separately: dh_vote_products_f64 alone (9 sources, 15 classes, 4 items), 2 000 launches back to back on one
stream between two device events.  The weights are synthetic: the labels are whatever such a network gives.  The device
loop's products are compared with the host loop's and the reference shape's once and the answers recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_pass(torch, nseq, clips, reps, batch=4, stored=48):
    from bench import build_penn_merge
    from deephar_amd import frontend
    from deephar_amd import functional as Fn
    from deephar_amd.evaltools import action, clip_window
    rng = np.random.default_rng(1)
    model = build_penn_merge()
    T = int(model.inputs[0].shape[0])
    OH, OW = int(model.inputs[0].shape[1]), int(model.inputs[0].shape[2])
    outidx = [k for k, v in enumerate(model.outputs) if len(v.shape) == 1]
    C = int(model.outputs[outidx[0]].shape[0])
    H, W = 720, 1280
    store = frontend.FrameStore([rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(stored)])
    index, windows, hflip, seq, keys = [], [], [], [], []
    for i in range(nseq):
        for f in range(clips):
            first = int(rng.integers(0, stored - T + 1))
            cx, cy, side = rng.uniform(0.3 * W, 0.7 * W), rng.uniform(0.3 * H, 0.7 * H), rng.uniform(250.3, 700.7)
            w = clip_window(np.array([cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2]))
            for h in (0, 1):
                index.append(np.arange(first, first + T))
                windows.append(w)
                hflip.append(h)
                seq.append(i)
                keys.append('%04d.%03d.%d' % (i, f, h))
    index, windows, hflip, seq = np.stack(index), np.stack(windows), np.array(hflip), np.array(seq, np.int32)
    total = len(seq)
    a_true = np.eye(C)[rng.integers(0, C, nseq)]
    res = {'sequences': nseq, 'clips_per_sequence': clips, 'items': total, 'frames_per_clip': T, 'batch': batch, 'repetitions': reps,
           'frames': '720x1280', 'outputs': outidx, 'classes': C}
    # the reference shape's inputs: the same crops, made once (cropped on the GPU, copied out)
    crops = np.stack([Fn.crop_resize(store.tensors, [(int(i), tuple(int(v) for v in windows[k]), bool(hflip[k])) for i in index[k]],
                                     (OH, OW)).cpu().numpy() for k in range(total)])

    def reference_shape():
        a_pred = np.ones((len(outidx), nseq, C))
        for k in range(total):
            pred = model.predict(crops[k:k + 1])
            for b, o in enumerate(outidx):
                a_pred[b, seq[k], :] *= pred[o][0]
        return a_pred

    def drive(loop):
        return action.multiclip_votes_frames(model, store, index, windows, hflip, seq, a_true, keys, batch_size=batch, loop=loop,
                                             outidx=outidx, verbose=0)

    legs = {'reference_shape': reference_shape, 'loop_host': lambda: drive('host'), 'loop_device': lambda: drive('device')}
    first = {k: fn() for k, fn in legs.items()}                                   # bind, autotune, capture; and the answers
    res['loop_device_scores_equal_loop_host'] = bool(np.array_equal(first['loop_device'], first['loop_host']))
    products = frontend.votes_from_frames(model, store, index, windows, hflip, seq, nseq=nseq, outidx=outidx, batch_size=batch)[0]
    res_host = frontend.predict_from_frames(model, store, index, windows, hflip, batch_size=batch)
    host_products, _ = action.vote_products([res_host[o] for o in outidx], seq, nseq)
    res['loop_device_products_equal_loop_host'] = bool(np.array_equal(products, host_products))
    res['reference_shape_products_equal_loop_host'] = bool(np.array_equal(first['reference_shape'], host_products))
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():                                               # alternating in one process
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    for k, ts in times.items():
        res[k] = dict(seconds=ts, clips_per_s=[total / t for t in ts], median_clips_per_s=total / float(np.median(ts)),
                      spread_seconds=max(ts) - min(ts), spread_clips_per_s=total / min(ts) - total / max(ts))
    med = {k: float(np.median(ts)) for k, ts in times.items()}
    for a, b in [('loop_device', 'loop_host'), ('loop_device', 'reference_shape'), ('loop_host', 'reference_shape')]:
        spread = max(max(times[k]) - min(times[k]) for k in (a, b))
        res['%s_over_%s' % (a, b)] = dict(ratio_clips_per_s=med[b] / med[a], difference_seconds=med[b] - med[a],
                                          difference_us_per_clip=(med[b] - med[a]) / total * 1e6, spread_seconds=spread,
                                          outside_the_spread=bool(abs(med[b] - med[a]) > spread))
    return res


def bench_launch(torch, launches=2000, nb=9, C=15, n=4, nseq=16):
    """dh_vote_products_f64 alone: `launches` launches back to back on one stream, timed with device events"""
    from deephar_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2)
    probs = [torch.from_numpy(rng.uniform(0.99, 1.01, (n, C)).astype(np.float32)).cuda() for _ in range(nb)]   # (stays finite)
    srcs = (_lib.VoteSrc * nb)(*[_lib.VoteSrc(p.data_ptr(), C) for p in probs])
    seq = torch.from_numpy(rng.integers(0, nseq, n).astype(np.int32)).cuda()
    acc = torch.ones((nb, nseq, C), dtype=torch.float64, device='cuda')
    label = torch.empty((nb, n), dtype=torch.int32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.dh_vote_products_f64(srcs, nb, C, seq.data_ptr(), n, nseq, acc.data_ptr(), label.data_ptr(), None, st),
                   'dh_vote_products_f64')
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
    return dict(sources=nb, classes=C, items=n, sequences=nseq, launches=launches, us_per_launch=us,
                median_us_per_launch=float(np.median(us)), labels_in_range=bool(((label.cpu().numpy() >= 0) & (label.cpu().numpy() < C)).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multiclip_votes.json'))
    ap.add_argument('--sequences', type=int, default=64)
    ap.add_argument('--clips', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_multiclip needs a HIP device'
    rec = {'device': torch.cuda.get_device_name(0), 'multiclip_votes': bench_pass(torch, args.sequences, args.clips, args.reps),
           'dh_vote_products_f64': bench_launch(torch)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
