#!/usr/bin/env python
"""Timings of Conv2DTranspose on the split-bf16 precision ladder (dh_conv2d_transpose2x2_split_f32) -> profiles/resampling_conv_bf16.json.

Per launch, at the three up-scaling shapes of a 256 px SPNet and `--frames` frames, per mode ('bf16x3' / 'bf16x2' / 'bf16'), in ONE
process, alternating A / B / A / B ...:
  * the split transposed convolution (BN + ReLU prologue, residual at the output resolution) beside the fp32 transposed
    convolution dh_conv2d_transpose2x2_f32 on the same buffers -- what the mode buys on this layer;
  * the same beside the plain split GEMM of the same M x K x N (dh_conv2d_f32 pointwise, w_split of the mode, ReLU prologue,
    residual of the GEMM's own shape; the family has no BN prologue there) -- what prologue + depth-to-space cost on the split
    path (the fp32 kernel's figure is 1.03-1.15x, profiles/resampling_conv.json).
Whole forward: the 'conv' SPNet (256 px, pose-only, `--pyramids`) per mode, bound as this library binds it ("new") and bound
with the transposed convolutions left on the fp32 kernel under the mode -- the binding of the commit before this layer joined
the ladder ("parent": every other launch is the same code); two separately bound parents give the run-to-run spread.
Device-resident graph replays, alternated in one process.

    python tools/bench_resampling_bf16.py [--out profiles/resampling_conv_bf16.json] [--reps 7] [--inner 20] [--frames 64]
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
from bench_resampling import UP, alternate, timed                   # noqa: E402

MODES = {m: (packing.MODE_PARTS[m], c) for m, c in packing.LAYOUT_CODES['standard'].items()}   # mode -> (parts, dh_conv_args.w_split)


def bench_convt(lib, st, dev, n, cin, cout, side, reps, inner):
    g = torch.Generator(device='cpu').manual_seed(cin + cout + side)
    x = torch.randn(n, side, side, cin, generator=g).to(dev)
    w = (torch.randn(2, 2, cout, cin, generator=g) / np.sqrt(cin)).numpy()
    sc, sh = (torch.rand(cin, generator=g) + 0.5).to(dev), torch.randn(cin, generator=g).to(dev)
    res = torch.randn(n, 2 * side, 2 * side, cout, generator=g).to(dev)
    y = torch.empty_like(res)
    keep = []

    def convt_args(wt, kp, np_):
        a = _lib.ConvtArgs()
        a.x, a.w, a.y, a.pre_scale, a.pre_shift, a.res = x.data_ptr(), wt.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr(), \
            res.data_ptr()
        a.N, a.H, a.W, a.Cin, a.ldx, a.Cout, a.ldy, a.ldr = n, side, side, cin, cin, cout, cout, cout
        a.Kp, a.Np, a.pre_relu, a.post_relu = kp, np_, 1, 0
        keep.append(wt)
        return a

    a32 = convt_args(*F.pack_convt_weight(w, dev))
    res2 = res.reshape(n, side, side, 4 * cout)
    y2 = torch.empty_like(res2)
    f32 = lambda: lib.dh_conv2d_transpose2x2_f32(C.byref(a32), -1, st)
    _lib.check(f32(), 'convT fp32')
    out = dict(frames=n, Cin=cin, Cout=cout, side_in=side, M=n * side * side, K=cin, N=4 * cout,
               gflop=2.0 * n * side * side * cin * 4 * cout / 1e9, modes={})
    for mode, (parts, code) in MODES.items():
        a = convt_args(*F.pack_convt_weight(w, dev, parts=parts))
        assert lib.dh_conv2d_transpose2x2_split_eligible(C.byref(a)) == 1
        split = lambda cfg: lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), parts, cfg, st)
        # the plain split GEMM [n * side^2, cin] x [cin, 4 cout] of the mode
        pk, kp2, np2 = packing.pack_conv_split(packing.convt_matrix(w), parts=parts)
        wp = torch.from_numpy(pk).to(dev)
        keep.append(wp)
        b = _lib.ConvArgs()
        b.x, b.w, b.y, b.res1 = x.data_ptr(), wp.data_ptr(), y2.data_ptr(), res2.data_ptr()
        b.N, b.H, b.W, b.Cin, b.ldx = n, side, side, cin, cin
        b.OH, b.OW, b.Cout, b.ldy, b.ldr1 = side, side, 4 * cout, 4 * cout, 4 * cout
        b.KH = b.KW = b.SH = b.SW = 1
        b.K, b.Kp, b.Np, b.pre_relu, b.w_split = cin, kp2, np2, 1, code
        gemm = lambda cfg: lib.dh_conv2d_f32(C.byref(b), cfg, st)
        tl = {}
        for cfg in range(lib.dh_conv2d_transpose2x2_num_split_tile_cfgs()):
            _lib.check(split(cfg), 'convT split')
            tl[cfg] = min(timed(lambda: split(cfg), inner) for _ in range(3))
        best = min(tl, key=tl.get)
        gl = {}
        for cfg in range(lib.dh_conv2d_num_split_tile_cfgs()):
            if gemm(cfg) != 0:
                continue
            gl[cfg] = min(timed(lambda: gemm(cfg), inner) for _ in range(3))
        gbest = min(gl, key=gl.get)
        _lib.check(split(-1), 'convT split')
        th, tf, rh, rf = alternate(lambda: split(-1), f32, reps, inner)               # library heuristic vs fp32
        tb, tg, rb, rg = alternate(lambda: split(best), lambda: gemm(gbest), reps, inner)   # best vs the plain GEMM's best
        torch.cuda.synchronize()
        out['modes'][mode] = dict(
            split_heuristic_us=round(th, 2), f32_us=round(tf, 2), speedup_vs_f32=round(tf / th, 3),
            split_best_us=round(tb, 2), split_best_cfg=best, gemm_best_us=round(tg, 2), gemm_best_cfg=gbest,
            ratio_vs_plain_split_gemm=round(tb / tg, 3), tilings_us={str(c): round(v, 2) for c, v in tl.items()},
            split_runs=rh, f32_runs=rf, best_runs=rb, gemm_runs=rg, checksum=float(y.double().sum()))
    return out


def bench_forward(n, pyramids, reps, inner):
    from deephar_amd import graph, utils, weights
    from deephar_amd.config import ModelConfig
    from deephar_amd.engine import executor
    from deephar_amd.models import spnet
    lib = _lib.load()
    x = np.random.default_rng(0).uniform(-1, 1, (n, 256, 256, 3)).astype(np.float32)

    class Parent:                                        # the library with the layer left on the fp32 kernel
        def __getattr__(self, name):
            return (lambda *a: 0) if name == 'dh_conv2d_transpose2x2_split_eligible' else getattr(lib, name)

    def build(mode, parent, table):
        graph.reset_naming()
        cfg = ModelConfig((256, 256, 3), utils.pa16j2d, num_actions=[], num_pyramids=pyramids, action_pyramids=[],
                          downsampling_type='conv')
        m = spnet.build(cfg)
        weights.init_synthetic(m, seed=0)
        m.gemm_precision = mode
        m.executor.tune_table = table                    # one autotuning per mode: the three bindings run the same tilings
        load = executor._lib.load
        if parent:
            executor._lib.load = lambda: Parent()
        try:
            m.predict(x, batch_size=n)                   # binds, autotunes, captures the graph
        finally:
            executor._lib.load = load
        codes = sorted({s.attrs.get('w_split') for s in m.plan.steps if s.kind == 'convtranspose'})
        assert codes == ([0] if parent or mode == 'f32' else [MODES[mode][1]]), codes
        return m

    def replay(m):
        ex = m.executor
        ex.forward(ex.bind(n))

    out = {}
    for mode in ('f32',) + tuple(MODES):
        table = {}
        names = ('new', 'parent', 'parent_again') if mode != 'f32' else ('new', 'parent_again')
        models = {k: build(mode, k != 'new', table) for k in names}
        for m in models.values():
            for _ in range(3):
                replay(m)
        torch.cuda.synchronize()
        runs = {k: [] for k in models}
        for _ in range(reps):
            for k, m in models.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(m.executor.stream):
                    e0.record()
                    for _ in range(inner):
                        replay(m)
                    e1.record()
                e1.synchronize()
                runs[k].append(e0.elapsed_time(e1) / inner)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        base = med.get('parent', med['new'])
        out[mode] = dict(ms={k: round(v, 4) for k, v in med.items()}, runs_ms={k: [round(t, 4) for t in v] for k, v in runs.items()},
                         new_over_parent=round(med['new'] / base, 4), parent_again_over_parent=round(med['parent_again'] / base, 4),
                         frames_per_s_new=round(n / med['new'] * 1e3, 1))
        del models
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'resampling_conv_bf16.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--forward-frames', type=int, default=16)
    ap.add_argument('--pyramids', type=int, nargs='+', default=[2, 8])
    ap.add_argument('--no-forward', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resampling_bf16 needs a HIP device: there is no CPU path and no timing without one')
    lib = _lib.load()
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    name = C.create_string_buffer(64)
    cus = C.c_int()
    lib.dh_device_info(0, name, 64, C.byref(cus))
    doc = dict(device=name.value.decode(), cus=cus.value, reps=args.reps, inner=args.inner,
               method='HIP events around `inner` back-to-back launches / graph replays; A / B alternated `reps` times in one '
                      'process, medians.  forward.parent = the same library with the transposed convolutions bound to the fp32 '
                      'kernel under the mode (the binding before this layer joined the ladder); parent_again = a second, '
                      'separately bound parent: its ratio to parent is the run-to-run spread',
               transposed_conv=[], forward={})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(doc, fh, indent=1)

    for cin, cout, side in UP:
        r = bench_convt(lib, st, dev, args.frames, cin, cout, side, args.reps, args.inner)
        doc['transposed_conv'].append(r)
        for mode, v in r['modes'].items():
            print('convT n=%d %d@%d^2 -> %d@%d^2 %-6s: %.1f us (heuristic) vs fp32 %.1f us: %.2fx | best cfg %d %.1f us vs plain split '
                  'GEMM %.1f us (cfg %d): %.2f | tilings %s' % (
                      args.frames, cin, side, cout, 2 * side, mode, v['split_heuristic_us'], v['f32_us'], v['speedup_vs_f32'],
                      v['split_best_cfg'], v['split_best_us'], v['gemm_best_us'], v['gemm_best_cfg'], v['ratio_vs_plain_split_gemm'],
                      v['tilings_us']), flush=True)
        save()
    if not args.no_forward:
        for pyr in args.pyramids:
            doc['forward']['pyramids_%d' % pyr] = f = dict(frames=args.forward_frames, **bench_forward(
                args.forward_frames, pyr, args.reps, max(4, args.inner // 4)))
            for mode in ('f32',) + tuple(MODES):
                v = f[mode]
                print('forward %d pyramids n=%d %-6s: %s ms  new/parent %.4f  parent again/parent %.4f  %.0f frames/s' % (
                    pyr, args.forward_frames, mode, v['ms'], v['new_over_parent'], v['parent_again_over_parent'],
                    v['frames_per_s_new']), flush=True)
            save()
    print('wrote', args.out)


if __name__ == '__main__':
    main()
