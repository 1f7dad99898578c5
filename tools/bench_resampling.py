#!/usr/bin/env python
"""Timings of the learned-resampling kernels (downsampling_type='conv') -> profiles/resampling_conv.json.

Per kernel, at the three up / down shapes of a 256 px SPNet, for 64 and 16 frames, next to the existing kernel doing
comparable work, in ONE process, alternating A / B / A / B ...:
  * dh_conv2d_transpose2x2_f32 (BN + ReLU prologue, residual at the output resolution) beside dh_conv2d_f32 pointwise with
    4 * Cout output columns (same FLOPs, same bytes in and out; BN + ReLU prologue, residual of the GEMM's own shape);
  * the strided separable convolution's depthwise half, dh_dwconv2d_strided_f32 (BN + ReLU prologue), beside dh_dwconv2d_f32 at
    stride 1 on the OUTPUT-sized map (same number of outputs and taps).
HIP events around `--inner` back-to-back launches, median over `--reps` alternations after a warm-up of every shape.
Whole forward: the 'conv' SPNet beside the max-pooling SPNet of the same configuration (pose-only, 2 pyramids, 256 px),
device-resident replays of the bound plan.

    python tools/bench_resampling.py [--out profiles/resampling_conv.json] [--reps 7] [--inner 20] [--frames 64 16]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deephar_amd import _lib, functional as F                       # noqa: E402
from deephar_amd.engine import packing                              # noqa: E402

UP = [(576, 480, 4), (480, 384, 8), (384, 288, 16)]         # transposed conv: Cin, Cout, input side
DOWN = [(288, 32), (384, 16), (480, 8)]                     # strided depthwise: C, input side


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner                # us per launch


def alternate(a, b, reps, inner):
    for fn in (a, b):                                       # warm-up: code objects, LDS limits, caches
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(a, inner))
        tb.append(timed(b, inner))
    return float(np.median(ta)), float(np.median(tb)), [round(v, 2) for v in ta], [round(v, 2) for v in tb]


def bench_convt(lib, st, dev, n, cin, cout, side, reps, inner):
    g = torch.Generator(device='cpu').manual_seed(cin + cout + side)
    x = torch.randn(n, side, side, cin, generator=g).to(dev)
    w = (torch.randn(2, 2, cout, cin, generator=g) / np.sqrt(cin)).numpy()
    sc, sh = (torch.rand(cin, generator=g) + 0.5).to(dev), torch.randn(cin, generator=g).to(dev)
    res = torch.randn(n, 2 * side, 2 * side, cout, generator=g).to(dev)
    y = torch.empty_like(res)
    wt, kp, np_ = F.pack_convt_weight(w, dev)
    a = _lib.ConvtArgs()
    a.x, a.w, a.y, a.pre_scale, a.pre_shift, a.res = x.data_ptr(), wt.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr(), \
        res.data_ptr()
    a.N, a.H, a.W, a.Cin, a.ldx, a.Cout, a.ldy, a.ldr = n, side, side, cin, cin, cout, cout, cout
    a.Kp, a.Np, a.pre_relu, a.post_relu = kp, np_, 1, 0
    # the plain GEMM of the same size: [n * side^2, cin] x [cin, 4 cout], residual and output [n * side^2, 4 cout]
    wp, kp2, np2 = F.pack_conv_weight(packing.convt_matrix(w), dev)
    res2 = res.reshape(n, side, side, 4 * cout)
    y2 = torch.empty_like(res2)
    b = _lib.ConvArgs()
    b.x, b.w, b.y, b.pre_scale, b.pre_shift, b.res1 = x.data_ptr(), wp.data_ptr(), y2.data_ptr(), sc.data_ptr(), sh.data_ptr(), \
        res2.data_ptr()
    b.N, b.H, b.W, b.Cin, b.ldx = n, side, side, cin, cin
    b.OH, b.OW, b.Cout, b.ldy, b.ldr1 = side, side, 4 * cout, 4 * cout, 4 * cout
    b.KH = b.KW = b.SH = b.SW = 1
    b.K, b.Kp, b.Np, b.pre_relu = cin, kp2, np2, 1
    out = dict(kernel='conv2d_transpose2x2', frames=n, Cin=cin, Cout=cout, side_in=side, gflop=2.0 * n * side * side * cin * 4 * cout / 1e9,
               mbytes=4.0 * (x.numel() + 2 * res.numel()) / 1e6, tilings={})
    best = None
    for cfg in range(lib.dh_conv2d_transpose2x2_num_tile_cfgs()):
        _lib.check(lib.dh_conv2d_transpose2x2_f32(C.byref(a), cfg, st), 'convT')
        # the plain GEMM at its library heuristic: what a pointwise layer of this size runs on without autotuning
        ta, tb, ra, rb = alternate(lambda: lib.dh_conv2d_transpose2x2_f32(C.byref(a), cfg, st),
                                   lambda: lib.dh_conv2d_f32(C.byref(b), -1, st), reps, inner)
        out['tilings'][str(cfg)] = dict(convt_us=round(ta, 2), gemm_us=round(tb, 2), convt_runs=ra, gemm_runs=rb)
        if best is None or ta < best[0]:
            best = (ta, tb, cfg)
    _lib.check(lib.dh_conv2d_transpose2x2_f32(C.byref(a), -1, st), 'convT')
    th, tg, _, _ = alternate(lambda: lib.dh_conv2d_transpose2x2_f32(C.byref(a), -1, st),
                             lambda: lib.dh_conv2d_f32(C.byref(b), -1, st), reps, inner)
    # the GEMM's own best tiling among the LDS-DMA ones (what the engine's autotuner would bind)
    gbest = None
    for cfg in range(9, 18):
        if lib.dh_conv2d_f32(C.byref(b), cfg, st) != 0:
            continue
        t = min(timed(lambda: lib.dh_conv2d_f32(C.byref(b), cfg, st), inner) for _ in range(3))
        if gbest is None or t < gbest[0]:
            gbest = (t, cfg)
    torch.cuda.synchronize()
    out.update(convt_heuristic_us=round(th, 2), gemm_heuristic_us=round(tg, 2), ratio_heuristic=round(th / tg, 3),
               convt_best_us=round(best[0], 2), convt_best_cfg=best[2], gemm_best_us=round(gbest[0], 2), gemm_best_cfg=gbest[1],
               ratio_best=round(best[0] / gbest[0], 3), checksum=float(y.double().sum()))
    return out


def bench_dw(lib, st, dev, n, c, side, reps, inner):
    g = torch.Generator(device='cpu').manual_seed(c + side)
    x = torch.randn(n, side, side, c, generator=g).to(dev)
    o = side // 2
    y = torch.empty(n, o, o, c, device=dev)
    w = torch.randn(25, c, generator=g).to(dev)
    sc, sh = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    a = _lib.DwsArgs()
    a.x, a.w, a.y, a.pre_scale, a.pre_shift = x.data_ptr(), w.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr()
    a.N, a.H, a.W, a.C, a.ldx, a.ldy, a.OH, a.OW = n, side, side, c, c, c, o, o
    a.KH = a.KW = 5
    a.SH = a.SW = 2
    a.PT = a.PL = 1
    a.pre_relu = 1
    x1 = x[:, :o, :o].contiguous()
    y1 = torch.empty_like(x1)
    b = _lib.DwArgs()
    b.x, b.w, b.y, b.pre_scale, b.pre_shift = x1.data_ptr(), w.data_ptr(), y1.data_ptr(), sc.data_ptr(), sh.data_ptr()
    b.N, b.H, b.W, b.C, b.ldx, b.ldy = n, o, o, c, c, c
    b.KH = b.KW = 5
    b.PT = b.PL = 2
    b.pre_relu = 1
    _lib.check(lib.dh_dwconv2d_strided_f32(C.byref(a), st), 'strided dw')
    _lib.check(lib.dh_dwconv2d_f32(C.byref(b), st), 'dw')
    ta, tb, ra, rb = alternate(lambda: lib.dh_dwconv2d_strided_f32(C.byref(a), st), lambda: lib.dh_dwconv2d_f32(C.byref(b), st),
                               reps, inner)
    return dict(kernel='dwconv2d_strided', frames=n, C=c, side_in=side, side_out=o, strided_us=round(ta, 2), stride1_us=round(tb, 2),
                ratio=round(ta / tb, 3), strided_runs=ra, stride1_runs=rb, mbytes_strided=4.0 * (x.numel() + y.numel()) / 1e6,
                mbytes_stride1=8.0 * y1.numel() / 1e6, checksum=float(y.double().sum()))


def bench_forward(n, reps, inner):
    from deephar_amd import graph, utils, weights
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import spnet
    out = {}
    x = np.random.default_rng(0).uniform(-1, 1, (n, 256, 256, 3)).astype(np.float32)
    models = {}
    for ds in ('maxpooling', 'conv'):
        graph.reset_naming()
        cfg = ModelConfig((256, 256, 3), utils.pa16j2d, num_actions=[], num_pyramids=2, action_pyramids=[], downsampling_type=ds)
        m = spnet.build(cfg)
        weights.init_synthetic(m, seed=0)
        m.predict(x, batch_size=n)                           # binds, autotunes, captures the graph
        models[ds] = m
    runs = {ds: [] for ds in models}

    def replay(m):
        ex = m.executor
        bp = ex.bind(n)
        ex.forward(bp)

    for ds, m in models.items():
        for _ in range(3):
            replay(m)
    torch.cuda.synchronize()
    for _ in range(reps):
        for ds, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(m.executor.stream):
                e0.record()
                for _ in range(inner):
                    replay(m)
                e1.record()
            e1.synchronize()
            runs[ds].append(e0.elapsed_time(e1) / inner)
    for ds, m in models.items():
        out[ds] = dict(ms_per_forward=round(float(np.median(runs[ds])), 4), runs_ms=[round(v, 4) for v in runs[ds]],
                       launches=len(m.executor.bind(n).calls) - len(m.executor.bind(n).noop_calls), plan_steps=len(m.plan.steps),
                       gflop=round(m.plan.total_flops(n) / 1e9, 2))
    out['ratio_conv_over_maxpooling'] = round(out['conv']['ms_per_forward'] / out['maxpooling']['ms_per_forward'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'resampling_conv.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--frames', type=int, nargs='+', default=[64, 16])
    ap.add_argument('--no-forward', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resampling needs a HIP device: there is no CPU path and no timing without one')
    lib = _lib.load()
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    name = C.create_string_buffer(64)
    cus = C.c_int()
    lib.dh_device_info(0, name, 64, C.byref(cus))
    doc = dict(device=name.value.decode(), cus=cus.value, reps=args.reps, inner=args.inner,
               method='HIP events around `inner` back-to-back launches; A / B alternated `reps` times in one process, medians',
               transposed_conv=[], strided_depthwise=[], forward={})
    for n in args.frames:
        for cin, cout, side in UP:
            r = bench_convt(lib, st, dev, n, cin, cout, side, args.reps, args.inner)
            doc['transposed_conv'].append(r)
            print('convT  n=%-3d %d@%d^2 -> %d@%d^2: %.1f us (cfg %d) vs plain GEMM %.1f us (cfg %d)  ratio %.2f | heuristic %.1f vs %.1f'
                  % (n, cin, side, cout, 2 * side, r['convt_best_us'], r['convt_best_cfg'], r['gemm_best_us'], r['gemm_best_cfg'],
                     r['ratio_best'], r['convt_heuristic_us'], r['gemm_heuristic_us']), flush=True)
        for c, side in DOWN:
            r = bench_dw(lib, st, dev, n, c, side, args.reps, args.inner)
            doc['strided_depthwise'].append(r)
            print('dw s2  n=%-3d %d@%d^2 -> %d^2: %.1f us vs stride-1 on %d^2 %.1f us  ratio %.2f'
                  % (n, c, side, r['side_out'], r['strided_us'], r['side_out'], r['stride1_us'], r['ratio']), flush=True)
    if not args.no_forward:
        for n in args.frames:
            doc['forward']['frames_%d' % n] = f = bench_forward(n, args.reps, max(4, args.inner // 4))
            print('forward n=%-3d conv %.3f ms (%d launches) vs max-pooling %.3f ms (%d launches)  ratio %.3f'
                  % (n, f['conv']['ms_per_forward'], f['conv']['launches'], f['maxpooling']['ms_per_forward'],
                     f['maxpooling']['launches'], f['ratio_conv_over_maxpooling']), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
