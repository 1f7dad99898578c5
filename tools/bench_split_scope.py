#!/usr/bin/env python
"""Model.gemm_scope measured in ONE process: 'standard' against 'extended' under every Model.gemm_precision, on the workloads
whose convolutions the extended scope reaches (SPNet: ntu_spnet, speed2d), the instances ALTERNATING over several rounds as in
tools/bench_precision_ladder.py -- a difference between the scopes is read against the run-to-run spread of the same process on
the same card.

    python tools/bench_split_scope.py [--workloads ntu_spnet,speed2d] [--modes f32,bf16x3,bf16x2,bf16] [--rounds 5]
                                      [--out profiles/split_scope.json]

Three records:
  * the device step of each workload, modes x scopes (bench.py's builders, set-up routines and `timed`; 10 steps after 3
    warm-up steps, one GPU);
  * mpii as the control: its convolutions are all of the standard scope, so its launch list must be the same under both scopes
    -- asserted here, launch by launch (entry point, packing of the mode, tiling);
  * per layer: the SPNet entry-flow 3 x 3 convolutions (128 x 128 x 48 -> 96, 64 x 64 x 144 -> 288 and its stride-2 sibling
    from 128 x 128) on the fp32 kernels (halo-resident where that rule takes the layer, else the best tap-major tiling) and
    under w_split = 5 / 6 / 7, and a BatchNormalization-prologue 1 x 1 of the NTU plan (64 x 64 x 192 -> 96) beside its fp32
    launch; best tiling each, HIP events.
Nothing here predicts a speed-up: the table says what was measured, slower rows included."""
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
SCOPES = ('standard', 'extended')
BASE = {5: 1, 6: 3, 7: 4}


def setup(workload, mode, scope):
    """One resident, bound and tuned instance -> step, streams, pairs, frames per step, the bound launches."""
    wl = bench.WORKLOADS[workload]
    a = types.SimpleNamespace(no_graph=False, input='f32', force_cfg=None, force_collective=False, no_overlap=False)
    model = wl['build']()
    model.gemm_precision, model.gemm_scope = mode, scope
    if wl['clips']:
        step, pairs, bound, streams, frames, flops, check, par, restage = bench.setup_clips(workload, model, wl['per_gpu'], 1, 0, a)
        scm = bench.LAST_SCM[0]
        plans = [scm.frame_model.plan, scm.head_model.plan]
    else:
        step, bound, streams, frames, flops, check, restage = bench.setup_frame_workload(model, wl['per_gpu'], wl['T'], a, 1, 0)
        pairs = None
        plans = [model.plan]
    convs = [s for p in plans for s in p.steps if s.kind == 'conv']
    codes = [s.attrs.get('w_split', 0) for s in convs]
    flops_all = sum(s.flops(1) for s in convs)
    flops_split = sum(s.flops(1) for s in convs if s.attrs.get('w_split', 0) in (1, 3, 4, 5, 6, 7))
    # one entry per bound launch: entry point, step kind, packing of the mode (5 / 6 / 7 named as 1 / 3 / 4), tiling
    launches = [(getattr(fn, '__name__', str(fn)), st.kind, BASE.get(st.attrs.get('w_split', 0), st.attrs.get('w_split', 0)),
                 st.attrs.get('tile_cfg', -1)) for bp, _ in bound for fn, _, st in bp.calls]
    return dict(step=step, streams=streams, pairs=pairs, frames=frames, check=check, keep=(model, bound), launches=launches,
                split_convs=sum(1 for c in codes if c in (1, 3, 4, 5, 6, 7)), convs=len(codes),
                conv_flops_on_ladder=round(flops_split / max(flops_all, 1), 4))


def scopes(workload, modes, steps, warmup, rounds):
    import torch
    keys = [(m, s) for m in modes for s in SCOPES]
    inst = {k: setup(workload, *k) for k in keys}
    ms = {k: [] for k in keys}
    for r in range(rounds):
        for k in (keys if r % 2 == 0 else keys[::-1]):          # alternate, and alternate the order
            i = inst[k]
            dt = bench.timed(i['step'], i['streams'], steps, warmup, 1, i['pairs'])
            ms[k].append(1e3 * dt / steps)
    out = {'workload': bench.WORKLOADS[workload]['name'], 'steps': steps, 'warmup': warmup, 'rounds': rounds,
           'frames_per_step': inst[keys[0]]['frames'], 'modes': {}}
    for m in modes:
        row = {}
        for s in SCOPES:
            v, i = ms[(m, s)], inst[(m, s)]
            med = statistics.median(v)
            row[s] = {'step_ms_median': round(med, 4), 'step_ms_rounds': [round(x, 4) for x in v],
                      'spread_fraction': round((max(v) - min(v)) / med, 4), 'frames_per_s': round(1e3 * i['frames'] / med, 1),
                      'split_convs': i['split_convs'], 'convs': i['convs'], 'conv_flops_on_ladder': i['conv_flops_on_ladder'],
                      'outputs_finite': bool(np.all(np.isfinite(i['check']())))}
        gain = row['standard']['step_ms_median'] / row['extended']['step_ms_median'] - 1.0
        spread = max(row['standard']['spread_fraction'], row['extended']['spread_fraction'])
        row['extended_vs_standard'] = {'gain_fraction': round(gain, 4), 'spread_fraction': spread,
                                       'differs_by_more_than_spread': bool(abs(gain) > spread)}
        out['modes'][m] = row
    del inst
    torch.cuda.empty_cache()
    return out


def control(mode='bf16'):
    """mpii: every convolution the ladder reaches is of the standard scope -- the two scopes bind the same launches."""
    import torch
    a, b = setup('mpii', mode, 'standard'), setup('mpii', mode, 'extended')
    assert len(a['launches']) == len(b['launches']) and a['launches'], (len(a['launches']), len(b['launches']))
    for i, (u, v) in enumerate(zip(a['launches'], b['launches'])):
        assert u == v, 'mpii launch %d differs between the scopes: %r / %r' % (i, u, v)
    ya, yb = a['check'](), b['check']()
    assert np.array_equal(ya, yb), 'mpii outputs differ between the scopes'
    out = {'workload': 'mpii', 'mode': mode, 'launches': len(a['launches']), 'split_convs': a['split_convs'],
           'launch_list_identical': True, 'outputs_bit_identical': True}
    del a, b
    torch.cuda.empty_cache()
    return out


# (name, (N, H, W, Cin, Cout), k, stride, BN prologue): per-frame geometry of the NTU plan, 8 frames
LAYERS = [('entry 3x3 128x128x48->96', (8, 128, 128, 48, 96), 3, 1, False),
          ('entry 3x3 64x64x144->288', (8, 64, 64, 144, 288), 3, 1, False),
          ('entry 3x3 stride 2 128x128x144->288', (8, 128, 128, 144, 288), 3, 2, False),
          ('shortcut 1x1 BN+ReLU 64x64x192->96', (8, 64, 64, 192, 96), 1, 1, True)]


def layers(reps=20):
    import torch
    from deephar_amd import _lib, functional as F
    from deephar_amd.engine import packing
    lib = _lib.load()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    out = []
    for name, (n, h, w, cin, cout), ks, st, bn in LAYERS:
        x = torch.from_numpy(rng.uniform(-1, 1, (n, h, w, cin)).astype(np.float32)).to(dev)
        k = (rng.standard_normal((ks, ks, cin, cout)) / np.sqrt(ks * ks * cin)).astype(np.float32)
        ps = torch.from_numpy(rng.uniform(0.5, 1.5, cin).astype(np.float32)).to(dev) if bn else None
        pb = torch.zeros(cin, device=dev) if bn else None
        kw = dict(strides=(st, st), pre_scale=ps, pre_shift=pb, pre_relu=bn)
        rec = {'layer': name, 'reps': reps, 'kernels': {}}

        def best(run, ncfg):
            times = {}
            for cfg in range(ncfg):
                try:
                    run(cfg)
                except _lib.DeepharHipError as e:
                    if 'rc=-2' not in str(e):
                        raise
                    continue
                t = float('inf')
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        run(cfg)
                    e1.record()
                    e1.synchronize()
                    t = min(t, 1e3 * e0.elapsed_time(e1) / reps)
                times[cfg] = round(t, 2)
            cfg = min(times, key=times.get)
            return {'best_tile_cfg': cfg, 'us_per_launch': times[cfg], 'us_per_tile_cfg': times}
        pk = packing.pack_conv(k)
        packed = (torch.from_numpy(pk[0]).to(dev), pk[1], pk[2])
        rec['kernels']['f32 tap-major'] = best(lambda cfg: F.conv2d(x, k, packed=packed, tile_cfg=cfg, **kw), lib.dh_conv2d_num_tile_cfgs())
        if ks > 1 and st == 1:
            try:
                ph = packing.pack_conv_halo(k)
                hp = (torch.from_numpy(ph[0]).to(dev), ph[1], ph[2])
                rec['kernels']['f32 halo-resident'] = best(lambda cfg: F.conv2d(x, k, packed=hp, halo=True, tile_cfg=cfg, **kw),
                                                           lib.dh_conv2d_num_halo_tile_cfgs())
            except _lib.DeepharHipError:
                pass
        for mode, parts in (('bf16x3', 3), ('bf16x2', 2), ('bf16', 1)):
            ps_ = packing.pack_conv_split(k, parts=parts)
            sp = (torch.from_numpy(ps_[0]).to(dev), ps_[1], ps_[2])
            rec['kernels'][mode + ' extended'] = best(
                lambda cfg: F.conv2d(x, k, packed=sp, precision=mode, scope='extended', tile_cfg=cfg, **kw),
                lib.dh_conv2d_num_split_tile_cfgs())
        f32 = min(v['us_per_launch'] for n_, v in rec['kernels'].items() if n_.startswith('f32'))
        rec['vs_best_f32'] = {n_: round(f32 / v['us_per_launch'], 3) for n_, v in rec['kernels'].items()}
        out.append(rec)
    return {'layers': out, 'note': 'eager launches back to back (host-side argument marshalling included: an upper bound for '
                                   'the short ones); vs_best_f32 > 1: faster than the faster fp32 kernel'}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--workloads', default='ntu_spnet,speed2d')
    ap.add_argument('--modes', default=','.join(MODES))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-control', action='store_true')
    ap.add_argument('--no-layers', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'split_scope.json'))
    args = ap.parse_args()
    import torch
    modes = [m for m in args.modes.split(',') if m]
    assert all(m in MODES for m in modes), modes
    res = {'tool': 'tools/bench_split_scope.py', 'device': torch.cuda.get_device_name(0),
           'protocol': 'modes x scopes alternating inside one process; median over rounds of the device step (ms); '
                       'spread = (max - min) / median', 'workloads': {}}
    if not args.no_layers:
        res['per_layer'] = layers()
        print(json.dumps({'per_layer': res['per_layer']}), flush=True)
    if not args.no_control:
        res['control'] = control()
        print(json.dumps({'control': res['control']}), flush=True)
    for w in [v for v in args.workloads.split(',') if v]:
        res['workloads'][w] = scopes(w, modes, args.steps, args.warmup, args.rounds)
        print(json.dumps({w: res['workloads'][w]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
