#!/usr/bin/env python
"""Headline benchmark of the pose-regression hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload mpii|h36m|penn_merge|ntu_spnet]
        (N > 1 without torch.distributed.run around it: bench.py starts the N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Workloads (BASELINE.json `configs`):
  mpii        (default; configs[1], the configuration `metric` is quoted on) ReceptionNet 8 blocks, J=16, 2 contexts,
              5x5: one step = one forward over a batch of 64 synthetic 256x256x3 frames per GPU.  Frames shard over
              ranks with no data-path collective (weak scaling).
  h36m        (configs[2]) ReceptionNet dim=3, 8 blocks, J=17, 16 depth maps (exp/h36m/eval_h36m.py:42-48): batch 128
              per GPU, frames shard like mpii.
  penn_merge  (configs[3]) merge model, 16-frame clips, 4 blocks, 15 actions, 4 clips per GPU and step;
  ntu_spnet   (configs[4]) SPNet pa17j3d, 60 actions, 32-frame clips, 8 clips per GPU and step.
  speed2d     the reference's OWN speed protocol (exp/pennaction/eval_speed2d.py:31-79): SPNet-Penn, 6 pyramids, actions on
              all six, pose_replica=True, 8-frame clips; for every prediction block b the truncated
              Model(full.input, full.outputs[2b:2b+2]), one warm-up predict, then 250 clips through
              predict(x, batch_size=2) on HOST arrays, wall clock -> `speed2d.fps_per_block` (18 entries).  A step of the
              contract line (`value`) is one device-resident forward of the LAST block's model on 2 clips = 16 frames.
              Runs with the engine's latency-regime setting (Model.num_streams = 2, stream_policy = 'tail') unless
              --streams / --stream-policy say otherwise.
              Clip workloads are FRAME-SHARDED: every rank runs T/N frames of all N x clips_per_gpu clips through the
              frame stage (conv stack + decoder + kronecker pooling), ONE RCCL all-gather of the packed
              [clips, T/N, J, C] tensor, then the (tiny) action head replicated on every rank -- all device resident
              (deephar_amd/parallel.py).  `collective_us` is the all-gather's share of a step (HIP events).
One step is timed with the inputs already resident in HBM and the outputs left in HBM: value = frames all ranks
processed / max-over-ranks wall time of exactly K steps bracketed by barriers + device synchronisation.
A plain run sets up, runs W untimed and K timed steps, and prints ONE JSON line from rank 0 (`value`, `ms_per_step`, ...).
    --dump-outputs DIR  after the timed steps, rank 0 writes every model output of the last step (what a caller of the
                        timed path receives) as DIR/output_<k>.npy, float32, in model order; same arguments, same inputs.
    --full              everything beyond the headline figure as well (below); --dump-steps also runs the per-kernel pass.
With --full the line also carries
  roofline     : the dominant kernel by summed time (an MFMA conv instantiation, named as rocprofv3 names it):
                 algorithmic FLOPs per launch (from the plan: 2 * M * K * Cout) / average launch duration, measured
                 with HIP events on the launch stream in an eager pass right after the timed region (kernels inside
                 a replayed hipGraph cannot be bracketed); peak = 157.3 TFLOP/s fp32 MFMA (MI355X_MICROARCH.md);
                 `traffic` = HBM bytes per launch from the separate rocprofv3 --pmc passes over THE SAME launch --
                 instantiation, M x K x N and epilogue (profiles/pmc_dominant_kernel.json, written by
                 tools/profile_round.py from `bench.py --replay-step`), else null.
  predict_fps  : (mpii, N=1) what a caller of Model.predict gets -- host numpy arrays in, host arrays out, wall clock
                 over 2 048 frames after one warm-up call (method of exp/pennaction/eval_speed2d.py:70-77), for float32
                 frames and for raw uint8 frames (normalised inside the first convolution).  Never `value`.
  cpu_baseline : the CPU oracle (a port; TensorFlow/Keras are not installable here) on the host cores of this box:
                 batch 16, median of 5 after one warm-up.  N=1, rank 0 only.
  and the mpii line's bf16x3, frame_sharded_clips and compact h36m / ntu_spnet / speed2d legs, speed2d's per-block
  protocol and the clip workloads' serial-form comparison (--no-* options drop them one by one).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # RCCL across processes needs dmabuf IPC on this driver

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_HBM_GBS = 8000.0
TILES = [(2, 2, 2, 3), (2, 2, 2, 2), (4, 1, 1, 3), (4, 1, 1, 2), (4, 1, 1, 1), (2, 1, 1, 3), (2, 1, 1, 2),
         (2, 1, 1, 1), (1, 1, 1, 1)]
# split-bf16 tilings (csrc/gemm1x1s.hip launch_gemm1x1_split): cfg -> ((WM, WN, TM, TN), LDS stages); wide: cfg -> WM
SPLIT_TILES = {i: (t, 2) for i, t in enumerate(TILES)}
SPLIT_TILES.update({9: ((8, 1, 1, 3), 3), 10: ((4, 1, 1, 3), 3), 11: ((8, 1, 1, 2), 3), 12: ((4, 2, 1, 3), 2),
                    13: ((4, 2, 2, 3), 2)})
SPLIT_WIDE = {14: 4, 15: 2}


# ---- models ------------------------------------------------------------------------------------------------------
def build_mpii(blocks=8):
    from deephar_amd import graph, weights
    from deephar_amd.models import reception
    graph.reset_naming()
    m = reception.build((256, 256, 3), 16, dim=2, num_blocks=blocks, num_context_per_joint=2, ksize=(5, 5),
                        concat_pose_confidence=False)
    weights.init_synthetic(m, seed=0)
    return m


def build_h36m():
    """exp/h36m/eval_h36m.py:42-48: 3-D pose, 8 blocks, 17 joints, 16 depth maps per joint, 5x5 kernels."""
    from deephar_amd import graph, weights
    from deephar_amd.models import reception
    graph.reset_naming()
    m = reception.build((256, 256, 3), 17, dim=3, num_blocks=8, depth_maps=16, ksize=(5, 5))
    weights.init_synthetic(m, seed=0)
    return m


def build_penn_merge():
    """exp/pennaction/eval_penn_ar_pe_merge.py:42-57: 16-frame clips, 4 blocks, J=16, 15 actions."""
    from deephar_amd import graph, weights
    from deephar_amd.models import reception, action
    graph.reset_naming()
    pe = reception.build((256, 256, 3), 16, dim=2, num_blocks=4, num_context_per_joint=2, ksize=(5, 5))
    m = action.build_merge_model(pe, 15, (256, 256, 3), 16, 16, 4, pose_dim=2, pose_net_version='v1',
                                 output_poses=True)
    weights.init_synthetic(m, seed=0)
    return m


def build_ntu_spnet():
    """exp/ntu/eval_ntu_multitask.py:34-38 with the 32-frame clips BASELINE.json asks for."""
    from deephar_amd import graph, weights, utils
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import spnet
    graph.reset_naming()
    cfg = ModelConfig((32, 256, 256, 3), utils.pa17j3d, num_actions=[60], num_pyramids=2, action_pyramids=[1, 2],
                      num_levels=4, pose_replica=False, num_pose_features=192, num_visual_features=192)
    m = spnet.build(cfg)
    weights.init_synthetic(m, seed=0)
    return m


SPEED2D_CFG = dict(num_frames=8, num_joints=16, dim=2, num_actions=[15], num_pyramids=6,
                   action_pyramids=[1, 2, 3, 4, 5, 6], num_levels=4, kernel_size=(5, 5), growth=96, image_div=8,
                   num_pose_features=160, num_visual_features=160, sam_alpha=1, pose_replica=True)


def build_speed2d():
    """exp/pennaction/eval_speed2d.py:31-36,50: ModelConfig((8,) + (256, 256, 3), pa16j2d, num_actions=[15], num_pyramids=6,
    action_pyramids=[1..6], num_levels=4, pose_replica=True, num_pose_features=160, num_visual_features=160)."""
    from deephar_amd import graph, weights, utils
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import spnet
    graph.reset_naming()
    c = SPEED2D_CFG
    cfg = ModelConfig((c['num_frames'], 256, 256, 3), utils.pa16j2d, num_actions=c['num_actions'],
                      num_pyramids=c['num_pyramids'], action_pyramids=c['action_pyramids'], num_levels=c['num_levels'],
                      pose_replica=c['pose_replica'], num_pose_features=c['num_pose_features'],
                      num_visual_features=c['num_visual_features'])
    m = spnet.build(cfg)
    weights.init_synthetic(m, seed=0)
    return m


WORKLOADS = {
    'mpii': dict(build=build_mpii, clips=False, per_gpu=64, T=1,
                 name='MPII single-person 256x256, ReceptionNet 8 blocks J=16 ctx=2 k=5, pose-only forward, batch=64 '
                      'per GPU (BASELINE.json configs[1])'),
    'h36m': dict(build=build_h36m, clips=False, per_gpu=128, T=1,
                 name='Human3.6M 3-D pose 256x256, ReceptionNet 8 blocks J=17 dim=3 D=16 k=5, pose-only forward, batch=128 '
                      'per GPU (BASELINE.json configs[2])'),
    'penn_merge': dict(build=build_penn_merge, clips=True, per_gpu=4, T=16,
                       name='PennAction pose+action merge model, 16-frame 256x256 clips, 4 blocks, 4 clips per GPU, '
                            'frame-shard + RCCL all-gather (BASELINE.json configs[3])'),
    'ntu_spnet': dict(build=build_ntu_spnet, clips=True, per_gpu=8, T=32,
                      name='NTU multitask SPNet, 32-frame 256x256 clips, 8 clips per GPU, frame-shard + RCCL all-gather '
                           '(BASELINE.json configs[4])'),
    'speed2d': dict(build=build_speed2d, clips=False, per_gpu=2, T=8,
                    name='exp/pennaction/eval_speed2d.py protocol: SPNet-Penn 2-D pose + action, 6 pyramids, actions on all, '
                         'pose_replica, 8-frame 256x256 clips, truncated model of the LAST prediction block, 2 clips = 16 '
                         'frames per step (the small-batch / latency regime)'),
}


# ---- CPU baseline --------------------------------------------------------------------------------------------------
def cpu_model_string():
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def cpu_baseline(model, workload, blocks):
    """The CPU oracle (PyTorch-CPU fp32; a port -- TensorFlow/Keras are not installable here) on this box's host cores, on
    a BOUNDED sample of the same workload: a batch of 16 frames (mpii, h36m) or one clip (penn_merge: 16 frames,
    ntu_spnet: 32 frames); median of up to 5 runs after one warm-up, at most ~25 s."""
    import torch
    from deephar_amd import weights
    from oracle.naming import Weights
    # all cores up to 32: beyond that PyTorch-CPU's conv threading on a many-socket host gets slower, not
    # faster (measured: 256 threads -> 0.05 frames/s on the GPU box)
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    rng = np.random.default_rng(0)
    if workload in ('mpii', 'h36m'):
        from oracle import reception as oref
        wd = Weights(weights.as_dict(model))
        frames = 16
        x = rng.uniform(-1, 1, (frames, 256, 256, 3)).astype(np.float32)
        if workload == 'mpii':
            kw = dict(num_context_per_joint=2, num_blocks=blocks, ksize=(5, 5), concat_pose_confidence=False)
            run = lambda: oref.forward(wd, x, 16, 2, **kw)
        else:
            run = lambda: oref.forward(wd, x, 17, 3, num_blocks=8, depth_maps=16, ksize=(5, 5))
        what, src = 'a batch of %d frames' % frames, 'oracle/reception.py'
    elif workload == 'penn_merge':
        from oracle import action as oact
        wd = weights.as_dict(model)
        frames = 16
        x = rng.uniform(-1, 1, (1, 16, 256, 256, 3)).astype(np.float32)
        run = lambda: oact.forward_merge(wd, x, 15, 16, 4, pose_dim=2, pose_net_version='v1', output_poses=True)
        what, src = 'one 16-frame clip', 'oracle/action.py'
    elif workload == 'speed2d':
        from oracle import spnet as osp
        wd = weights.as_dict(model)
        frames = 16
        x = rng.uniform(-1, 1, (2, 8, 256, 256, 3)).astype(np.float32)
        ocfg = {k: v for k, v in SPEED2D_CFG.items() if k != 'num_frames'}
        run = lambda: osp.forward(wd, x, ocfg)
        what, src = 'one batch of two 8-frame clips (every prediction block: the last block\'s model needs them all)', 'oracle/spnet.py'
    else:
        from oracle import spnet as osp
        wd = weights.as_dict(model)
        frames = 32
        x = rng.uniform(-1, 1, (1, 32, 256, 256, 3)).astype(np.float32)
        ocfg = dict(num_joints=17, dim=3, num_actions=[60], num_pyramids=2, action_pyramids=[1, 2], num_levels=4,
                    kernel_size=(5, 5), growth=96, image_div=8, num_pose_features=192, num_visual_features=192,
                    sam_alpha=1, pose_replica=False)
        run = lambda: osp.forward(wd, x, ocfg)
        what, src = 'one 32-frame clip', 'oracle/spnet.py'
    run()  # warm-up
    ts = []
    t_all = time.perf_counter()
    for _ in range(5):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
        if time.perf_counter() - t_all > 25.0:      # bounded sample on a slow host
            break
    med = float(np.median(ts))
    return dict(value=round(frames / med, 2), unit='frames/s', cores=cores, kind='port', cpu=cpu_model_string(),
                host_logical_cpus=os.cpu_count(),
                sample='CPU-oracle baseline (stand-in for the reference TF-CPU path; TF/Keras absent from the image): '
                       '%s of the same 256x256x3 workload through %s (PyTorch-CPU fp32, %d threads), median of %d runs '
                       'after 1 warm-up, %.2f s per run' % (what, src, cores, len(ts), med))


# ---- kernel naming / roofline -----------------------------------------------------------------------------------------
def kernel_name(s):
    """The template instantiation a conv step launches, spelled as rocprofv3 demangles it."""
    cfg = s.attrs.get('tile_cfg', -1)
    if s.attrs.get('grouped'):
        return 'conv_dw_group_kernel (1x1 shortcut conv + the unit\'s depthwise conv in one launch)'
    if s.attrs.get('split_k'):
        return 'conv_splitk_kernel'
    if s.attrs.get('first_layer'):
        return 'conv_stem_kernel<%d, %d, %d, %s>' % (s.attrs['kh'], s.attrs['kw'], s.attrs['Cout'] // 32,
                                                     'true' if s.attrs.get('x_u8') else 'false')
    if cfg < 0:
        return 'conv (library-picked tiling)'
    b = lambda v: 'true' if v else 'false'
    a = s.attrs
    if a.get('w_split') == 2:
        return 'conv_halo_kernel<%d, %d, %s>' % (a['kw'], max(cfg, 0) + 1, b(a['pre_relu']))
    if a.get('w_split'):
        kxk = not (a['kh'] == a['kw'] == 1 and a['sh'] == a['sw'] == 1 and a['pt'] == a['pl'] == 0)
        if cfg in SPLIT_WIDE:
            return 'gemm1x1s_wide_kernel<%d, %s, %s, %s>' % (SPLIT_WIDE[cfg], b(a['up2']), b(a['pre_relu']), b(kxk))
        t, ns = SPLIT_TILES[cfg]
        return 'gemm1x1s_kernel<%d, %d, %d, %d, %s, %s, %s, %d>' % (t + (b(a['up2']), b(a['pre_relu']), b(kxk), ns))
    t = TILES[cfg % 9]
    if cfg >= 9:
        kxk = not (a['kh'] == a['kw'] == 1 and a['sh'] == a['sw'] == 1 and a['pt'] == a['pl'] == 0)
        return 'gemm1x1_kernel<%d, %d, %d, %d, %s, %s, %s>' % (t + (b(a['up2']), b(a['pre_relu']), b(kxk)))
    vec4 = s.ins['x'].C % 4 == 0 and s.ins['x'].ld % 4 == 0
    return 'conv_igemm_kernel<%d, %d, %d, %d, %s, %s>' % (t + (b(vec4), b(a['up2'])))


def epilogue_tag(s):
    """What a conv launch does after the accumulation, as a short tag: part of the identity of a measured launch
    (a second residual is 37 MB more algorithmic traffic on the dominant shape)."""
    a = s.attrs
    parts = []
    if a.get('pre_relu'):
        parts.append('prerelu')
    if 'post_bn' in s.params or 'post_affine' in s.params:
        parts.append('bn')
    if s.ins.get('res1') is not None:
        parts.append('res1')
    if s.ins.get('res2') is not None:
        parts.append('res2down' if a.get('res2_down') else 'res2')
    if a.get('post_relu'):
        parts.append('relu')
    if a.get('up2'):
        parts.append('up2')
    if s.outs.get('ypool') is not None:
        parts.append('pool')
    return '+'.join(parts) or 'plain'


ABSORBED = set()      # id() of the steps of the last profiled plans whose work runs inside a grouped / paired launch


def real_launches(bound):
    """Kernel launches of one forward: the plan's steps minus those a grouped / paired launch absorbed
    (BoundPlan.group_launches: dh_conv2d_dw_group_f32, dh_conv2d_pair_f32)."""
    return sum(len(bp.calls) - len(bp.noop_calls) for bp, _ in bound)


def profile_plans(bound):
    """bound: [(BoundPlan, stream_ptr)].  Per-step HIP-event times of an eager pass -> (rows, kinds)."""
    rows, kinds = [], {}
    ABSORBED.clear()
    for bp, sp in bound:
        times = bp.profile(sp, reps=3)
        steps = [c[2] for c in bp.calls]             # includes the stand-alone uint8 normalisation launches, in order
        ABSORBED.update(id(bp.calls[i][2]) for i in bp.noop_calls)
        for s, ms in zip(steps, times):
            n = bp.n
            rows.append((s, float(ms), n))
            k = kinds.setdefault(s.kind, dict(ms=0.0, flops=0.0, bytes=0.0, launches=0))
            k['ms'] += float(ms)
            k['flops'] += s.flops(n)
            k['bytes'] += s.bytes(n)
            k['launches'] += 1
    return rows, kinds


def roofline(rows, kinds, total_flops_per_step, ms_per_step):
    conv_kinds = [k for k in ('conv',) if k in kinds]
    conv = dict(ms=sum(kinds[k]['ms'] for k in conv_kinds), flops=sum(kinds[k]['flops'] for k in conv_kinds),
                launches=sum(kinds[k]['launches'] for k in conv_kinds))
    eager_total_ms = sum(ms for _, ms, _ in rows)
    # [r05] The line is keyed on the dominant LAUNCH SHAPE -- M x K x N plus epilogue, the unit SURVEY 8d prices -- not on a
    # template instantiation: an instantiation also runs other shapes (round 4's `frac` averaged one over 18 launches of
    # mixed shapes and could not be looked up in profiles/), and which of the near-equal tilings runs the dominant shape
    # differs from box to box.  `kernel` = the instantiation(s) that ran that shape here; `traffic` = the PMC passes of
    # tools/profile_round.py over the same shape + epilogue on the same instantiation (every tiling the autotuner
    # alternates between is profiled), null only when none matches.
    by_shape = {}
    for idx, (s, ms, n) in enumerate(rows):
        if s.kind != 'conv':
            continue
        x, y = s.ins['x'], s.outs['y']
        key = (n * x.lead(3) * y.shape[-3] * y.shape[-2] // (4 if s.attrs['up2'] else 1), s.attrs['K'], s.attrs['Cout'],
               epilogue_tag(s))
        sh = by_shape.setdefault(key, dict(ms=0.0, launches=0, flops=0.0, bytes=s.bytes(n), step=idx, kernels={}))
        sh['ms'] += ms
        sh['flops'] += s.flops(n)
        sh['launches'] += 1
        kn = kernel_name(s)
        sh['kernels'][kn] = sh['kernels'].get(kn, 0) + 1
    (m_, k_, n_, epi_), main = max(by_shape.items(), key=lambda kv: kv[1]['ms'])
    dom_name = max(main['kernels'].items(), key=lambda kv: kv[1])[0]
    achieved = main['flops'] / (main['ms'] * 1e-3) / 1e12
    traffic, traffic_src, pmc_extra = None, None, {}
    pmc_path = os.path.join(ROOT, 'profiles', 'pmc_dominant_kernel.json')
    if os.path.exists(pmc_path):
        with open(pmc_path) as f:
            pmc = json.load(f)
        for ent in pmc.get('launches', []):
            if ent['kernel'] == dom_name and ent['shape_mkn'] == [m_, k_, n_] and ent['epilogue'] == epi_ and \
                    abs(ent['algorithmic_bytes_per_launch'] - main['bytes']) <= 1e-6 * main['bytes']:
                traffic = ent['fetch_bytes_per_launch'] + ent['write_bytes_per_launch']
                traffic_src = ent['source']
                pmc_extra = {'traffic_over_algorithmic': round(traffic / main['bytes'], 4)}
                if 'mfma_busy_fraction' in ent:
                    pmc_extra['pmc_mfma_busy_fraction'] = ent['mfma_busy_fraction']
                break
    out = {'bound': 'mfma', 'kernel': dom_name, 'kernels_on_main_shape': main['kernels'],
           'achieved': round(achieved, 2), 'peak': PEAK_FP32_MFMA_TFLOPS, 'unit': 'TFLOP/s',
           'frac': round(achieved / PEAK_FP32_MFMA_TFLOPS, 4), 'traffic': traffic,
           'traffic_unit': 'bytes/launch (HBM read + write, PMC) of the main shape', 'traffic_source': traffic_src,
           'keyed_on': 'the launch shape (M x K x N + epilogue) with the largest summed time; achieved = its algorithmic '
                       'FLOPs / its average launch duration (HIP events, eager pass)',
           'main_shape_mkn': [m_, k_, n_], 'main_shape_epilogue': epi_, 'main_shape_step_index': main['step'],
           'main_shape_launches_per_step': main['launches'],
           'main_shape_avg_launch_us': round(1e3 * main['ms'] / main['launches'], 2),
           'avg_launch_us': round(1e3 * main['ms'] / main['launches'], 2),
           'algorithmic_bytes_per_launch': main['bytes'],
           'algorithmic_gflop_per_launch': round(main['flops'] / main['launches'] / 1e9, 3),
           'launches_per_step': main['launches'],
           'share_of_step_time': round(main['ms'] / eager_total_ms, 4),
           'all_mfma_conv_kernels': {'launches_per_step': conv['launches'],
                                     'achieved': round(conv['flops'] / (conv['ms'] * 1e-3) / 1e12, 2),
                                     'frac': round(conv['flops'] / (conv['ms'] * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4),
                                     'gflop_per_step': round(conv['flops'] / 1e9, 2)},
           'whole_forward_frac': round(total_flops_per_step / (ms_per_step * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)}
    out.update(pmc_extra)
    extra = {'kernel_time_share': {k: round(v['ms'] / eager_total_ms, 4) for k, v in sorted(kinds.items())},
             'hbm_bound_kernels': {k: {'GBps': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9, 1),
                                       'frac_of_8TBps': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)}
                                   for k, v in sorted(kinds.items()) if k in ('dwconv', 'pool') and v['ms'] > 0},
             # (includes the 16x16 / 8x8 levels, whose 5-38 MB launches are latency-, not bandwidth-bound; the 32x32 depthwise
             #  runs at 4.3-4.5 TB/s, torch's copy_ of the same tensor at 5.1: tools/micro/hbm_copy.py)
             'latency_bound_kernels': {k: {'launches': v['launches'], 'avg_us': round(1e3 * v['ms'] / v['launches'], 1),
                                           'MB_per_launch': round(v['bytes'] / v['launches'] / 1e6, 2)}
                                       for k, v in sorted(kinds.items()) if k in ('sam', 'sam_ctx', 'context_agg') and v['ms'] > 0}}
    return out, extra


# ---- Model.predict boundary ------------------------------------------------------------------------------------------
def predict_boundary(model, batch, frames=2048):
    """Wall-clock frames/s of Model.predict on HOST arrays (H2D of the inputs, hipGraph replays, D2H of every output),
    one warm-up call first -- the reference's own timing method (exp/pennaction/eval_speed2d.py:70-77)."""
    rng = np.random.default_rng(7)
    res = {}
    for tag in ('f32', 'u8'):
        reps = -(-frames // 256)              # 256 distinct frames, tiled: drawing 400 M random floats takes seconds
        if tag == 'f32':
            x = np.tile(rng.uniform(-1, 1, (256, 256, 256, 3)).astype(np.float32), (reps, 1, 1, 1))[:frames]
        else:
            x = np.tile(rng.integers(0, 256, (256, 256, 256, 3), dtype=np.uint8), (reps, 1, 1, 1))[:frames]
        model.predict(x, batch_size=batch)      # warm-up call (binds / tunes / captures the plan, pins the staging ring)
        t0 = time.perf_counter()
        out = model.predict(x, batch_size=batch)
        dt = time.perf_counter() - t0
        assert len(out[0]) == frames
        res[tag] = round(frames / dt, 1)
    return res


def speed2d_protocol(full_model, args, tune_table):
    """exp/pennaction/eval_speed2d.py:60-79 on the HIP engine: for every prediction block b the truncated
    Model(full.input, full.outputs[2b:2b+2]); `_ = m.predict(x[0:1])`; then wall clock around
    `m.predict(x, batch_size=2)` over num_clips = 250 clips of 8 frames on HOST arrays; fps = 250 * 8 / seconds.
    This engine specialises a plan per batch size (arena, tilings, hipGraph), so the reference's one-clip warm-up leaves the
    two-clip plan cold: `fps_per_block_protocol_exact` is the first timed call (it includes binding, tuning misses and graph
    capture of the two-clip plan), `fps_per_block` the same call again (what every later call of a caller's loop sees).  The
    tilings found for one truncated model are shared with the next (same layers, same shapes)."""
    from deephar_amd import Model
    clips, T = args.speed2d_clips, SPEED2D_CFG['num_frames']
    rng = np.random.default_rng(7)
    distinct = min(clips, 10)                   # 10 distinct clips, tiled: drawing 400 M random floats takes seconds
    x = np.tile(rng.uniform(-1, 1, (distinct, T, 256, 256, 3)).astype(np.float32), (-(-clips // distinct), 1, 1, 1, 1))[:clips]
    nb = len(full_model.outputs) // 2
    cold, warm, launches, gflop = [], [], [], []
    blocks = range(nb) if args.speed2d_blocks is None else [int(b) for b in args.speed2d_blocks.split(',')]
    for b in blocks:
        m = Model(full_model.input, full_model.outputs[2 * b:2 * b + 2])
        if args.streams is not None:
            m.num_streams = args.streams
        if args.stream_policy is not None:
            m.stream_policy = args.stream_policy
        m.executor.tune_table = tune_table
        m.executor.use_graph = not args.no_graph
        m.predict(x[0:1])                                           # "Warming up the new model."
        t0 = time.perf_counter()
        out = m.predict(x, batch_size=2)
        cold.append(round(clips * T / (time.perf_counter() - t0), 1))
        t0 = time.perf_counter()
        out = m.predict(x, batch_size=2)
        warm.append(round(clips * T / (time.perf_counter() - t0), 1))
        assert len(out) == 2 and len(out[0]) == clips and all(np.all(np.isfinite(o)) for o in out)
        bp2 = m.executor.bound.get(2)
        launches.append(len(bp2.calls) - len(bp2.noop_calls) if bp2 is not None else len(m.plan.steps))
        gflop.append(round(m.plan.total_flops(2) / 1e9, 2))
        del m
    return {'protocol': 'exp/pennaction/eval_speed2d.py:55-79', 'num_clips': clips, 'num_frames': T, 'batch_size': 2,
            'blocks': list(blocks), 'fps_per_block': warm, 'fps_per_block_protocol_exact': cold,
            'launches_per_call': launches, 'gflop_per_call': gflop,
            'whole_forward_frac_per_block': [round(g * 1e9 * f / (2 * T) / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)
                                             for g, f in zip(gflop, warm)],
            'note': 'host float32 arrays in, host arrays out, wall clock incl. H2D / D2H; fps_per_block = second timed call '
                    '(two-clip plan warm), fps_per_block_protocol_exact = first timed call after the one-clip warm-up'}


def setup_clips(workload, model, per_gpu, world, rank, args, load_tune=None, save_tune=None, total_clips=None):
    """Frame-sharded clip workload: frame stage on T/world frames of every clip -> ONE all-gather -> replicated head.
    Weak scaling: per_gpu * world clips per step (every rank keeps per_gpu * T frames); total_clips: a FIXED number of clips
    whatever the world (strong scaling: T/world frames of them per rank)."""
    import torch
    from deephar_amd import parallel
    wl = WORKLOADS[workload]
    T = wl['T']
    clips = per_gpu * world if total_clips is None else total_clips
    scm = parallel.ShardedClipModel(model, rank=rank, world=world, always_collective=bool(getattr(args, 'force_collective', False)),
                                    overlap=not getattr(args, 'no_overlap', False))
    LAST_SCM[0] = scm
    fm, hm, info = scm.frame_model, scm.head_model, scm.info
    for mm in (fm, hm):
        mm.executor.use_graph = not args.no_graph
        if load_tune:
            load_tune(mm.executor)
    x = np.random.default_rng(1234 + rank).uniform(-1, 1, (clips, info['Tl'], 256, 256, 3)).astype(np.float32)
    x_dev = torch.from_numpy(x).to(fm.executor.device)          # this rank's frames, resident in HBM
    pairs = []

    def step():
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        pairs.append(ev)
        scm.forward_device(x_dev, events=ev)

    step()                                                      # binds / tunes both stages
    pairs.clear()
    if save_tune:
        save_tune([fm.executor.tune_table, hm.executor.tune_table])
    fbp = fm.executor.bound[clips]
    hbp = hm.executor.bound[clips]
    bound = [(fbp, fm.executor.stream_ptr), (hbp, hm.executor.stream_ptr)]
    streams = [fm.executor.stream, hm.executor.stream, _LazyCommStream(scm)]
    flops = fm.plan.total_flops(clips) + hm.plan.total_flops(clips)
    check = lambda: scm.last_outputs[0].cpu().numpy()
    parallelism = 'frame-shard x%d: T/%d frames of %d clips per rank, one packed all-gather [%d, %d, J, %d] fp32, ' \
                  'head replicated' % (world, world, clips, clips, info['Tl'], info['packed_channels'])
    return step, pairs, bound, streams, clips * T, flops, check, parallelism, (lambda: None)


def setup_frame_workload(model, n, T, args, world, rank, load_tune=None, save_tune=None):
    """Replicas, no collective: a batch of n items (frames, or T-frame clips) resident in HBM, plus a second resident copy
    to re-stage from.  -> (step, bound, streams, frames per step over all ranks, flops per step, check, restage)"""
    import torch
    plan, ex = model.plan, model.executor
    ex.use_graph = not args.no_graph
    if load_tune:
        load_tune(ex)
    u8 = args.input == 'u8'
    bp = ex.bind(n, u8_norm=1 if u8 else None)
    if save_tune:
        save_tune([ex.tune_table])
    if args.force_cfg:                   # A/B aid: 'M,K,N:cfg' pins the tiling of every conv launch of that shape
        shape, cfg = args.force_cfg.split(':')
        mkn = tuple(int(v) for v in shape.split(','))
        for i, (fn, cargs, st) in enumerate(bp.calls):
            if st.kind == 'conv' and not st.attrs.get('split_k') and not st.attrs.get('first_layer') and \
                    not st.attrs.get('grouped'):
                a0 = cargs[0]._obj
                if (a0.N * a0.OH * a0.OW, a0.K, a0.Cout) == mkn:
                    bp.calls[i] = (fn, (cargs[0], int(cfg)), st)
                    st.attrs['tile_cfg'] = int(cfg)
    ishape = (n,) + tuple(model.inputs[0].shape)       # [n, 256, 256, 3] frames, or [n, T, 256, 256, 3] clips (speed2d)
    if u8:
        x = np.random.default_rng(1234 + rank).integers(0, 256, ishape, dtype=np.uint8)
    else:
        x = np.random.default_rng(1234 + rank).uniform(-1, 1, ishape).astype(np.float32)
    with torch.cuda.stream(ex.stream):
        ex.set_inputs(bp, [x])           # inputs resident in HBM before the timed region
        x_dev = torch.from_numpy(x).to(ex.device)
    ex.stream.synchronize()

    def step():
        # the input buffer is re-used by later activations inside one forward, so every step re-stages the
        # frames from a second HBM-resident copy (device-to-device, inside the timed region)
        with torch.cuda.stream(ex.stream):
            if not u8:        # (the uint8 staging buffer lives outside the arena and is never overwritten)
                bp.tensor(plan.inputs[0]).copy_(x_dev, non_blocking=True)
            ex.forward(bp)

    def restage():
        with torch.cuda.stream(ex.stream):
            if not u8:
                bp.tensor(plan.inputs[0]).copy_(x_dev)

    check = lambda: bp.tensor(plan.outputs[-2]).cpu().numpy()
    return step, [(bp, ex.stream_ptr)], [ex.stream], world * n * T, plan.total_flops(n), check, restage


def compact_leg(workload, args, rank):
    """[r06] A short run of ANOTHER workload appended to the default (mpii) line at N = 1, so that the driver's own
    `python bench.py` record carries every BASELINE configuration and the reference's speed protocol, not only configs[1]
    (VERDICT r05 missing #5): 10 timed steps after 3 warm-up steps of the same device-resident step `--workload <w>` times,
    the per-kernel pass, and the dominant launch shape priced like `roofline` (PMC traffic joined from
    profiles/pmc_dominant_kernel.json).  Full lines with cpu_baseline: `python bench.py --workload <w>`."""
    import copy
    import torch
    wl = WORKLOADS[workload]
    a = copy.copy(args)
    a.input, a.force_cfg, a.force_collective = 'f32', None, False
    full = wl['build']()
    model = full
    if workload == 'speed2d':
        from deephar_amd import Model
        a.streams, a.stream_policy = 2, 'tail'
        nb = len(full.outputs) // 2
        model = Model(full.input, full.outputs[2 * (nb - 1):2 * nb])
        model.num_streams, model.stream_policy = a.streams, a.stream_policy
    pairs = None
    if wl['clips']:
        step, pairs, bound, streams, frames, flops, check, par, restage = setup_clips(workload, model, wl['per_gpu'], 1, rank, a)
    else:
        step, bound, streams, frames, flops, check, restage = setup_frame_workload(model, wl['per_gpu'], wl['T'], a, 1, rank)
    steps = 10
    dt = timed(step, streams, steps, 3, 1, pairs)
    pose = check()
    restage()
    rows, kinds = profile_plans(bound)
    ms = 1e3 * dt / steps
    roof, _ = roofline(rows, kinds, flops, ms)
    keep = ('kernel', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'traffic_over_algorithmic', 'pmc_mfma_busy_fraction',
            'main_shape_mkn', 'main_shape_epilogue', 'main_shape_avg_launch_us', 'main_shape_launches_per_step',
            'algorithmic_bytes_per_launch', 'share_of_step_time')
    leg = {'workload': wl['name'], 'value': round(frames * steps / dt, 1), 'unit': 'frames/s', 'steps': steps,
           'ms_per_step': round(ms, 3), 'frames_per_step': frames, 'launches_per_step': real_launches(bound), 'plan_steps': len(rows),
           'streams': model.plan.nstreams if not wl['clips'] else 1,
           'whole_forward_frac': roof['whole_forward_frac'], 'gflop_per_step': round(flops / 1e9, 1),
           'outputs_finite_in_range': bool(np.all(np.isfinite(pose)) and pose[..., :2].min() >= 0 and pose[..., :2].max() <= 1),
           'roofline': {k: roof[k] for k in keep if k in roof}}
    if workload == 'speed2d' and not args.no_predict:
        # the reference's own number for three of the eighteen prediction blocks (first pose block, last pose block, last
        # action block), through Model.predict on host arrays like eval_speed2d.py:70-77, 100 clips instead of 250
        a.speed2d_clips, a.speed2d_blocks = 100, '0,8,17'
        sp = speed2d_protocol(full, a, model.executor.tune_table)
        leg['fps_per_block'] = dict(zip(('block0', 'block8', 'block17'), sp['fps_per_block']))
        leg['fps_per_block_note'] = 'Model.predict(x, batch_size=2) on host arrays, %d clips, second timed call' % sp['num_clips']
        leg['launches_per_call'] = dict(zip(('block0', 'block8', 'block17'), sp['launches_per_call']))
    del model, full, step, bound, check, restage, rows
    torch.cuda.empty_cache()
    return leg


LAST_SCM = [None]        # the ShardedClipModel of the last setup_clips call (its serial form is timed beside the pipelined one)


class _LazyCommStream:
    """The collective's own stream of a pipelined ShardedClipModel (created at its first step)."""

    def __init__(self, scm):
        self.scm = scm

    def synchronize(self):
        if self.scm._comm_stream is not None:
            self.scm._comm_stream.synchronize()


def serial_form_ms(scm, step, streams, pairs, world, steps=10):
    """[r06] The same clip step with the streams in their SERIAL form (frame stage of step i + 1 behind the collective of
    step i, deephar_amd/parallel.py): pipelined - serial = what the pipelining hides of the collective and the head stage."""
    if not scm.overlap:
        return None
    scm.synchronize()
    scm.overlap = False
    try:
        dt = timed(step, streams, steps, 2, world, pairs)
    finally:
        scm.synchronize()
        scm.overlap = True
    return 1e3 * dt / steps


def timed(step, streams, steps, warmup, world, pairs=None):
    """W untimed steps, then exactly K steps bracketed by barrier + device synchronisation; max over ranks."""
    import torch
    import torch.distributed as dist

    def drain():
        for s_ in streams:
            s_.synchronize()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    drain()
    if pairs is not None:
        pairs.clear()
    if world > 1:
        dist.barrier()
    host = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        h0 = time.perf_counter()
        step()
        host += time.perf_counter() - h0
    drain()
    t_local = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    # this rank's own clock (before the closing barrier) and the host time it spent enqueueing: with the per-rank
    # collective_us they decompose a multi-GPU step into compute, collective and launch cost
    LAST_TIMED.update(rank_ms_per_step=1e3 * t_local / steps, host_enqueue_us_per_step=1e6 * host / steps)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device='cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


LAST_TIMED = {}

DUMP_LIMIT_BYTES = 64 << 20


def step_outputs(model, bound, clips):
    """Every model output of the last step, in model order (device tensors): what a caller of the timed path receives."""
    if clips:
        return list(LAST_SCM[0].last_outputs)
    bp = bound[0][0]
    return [bp.tensor(v) for v in model.plan.outputs]


def dump_outputs(path, tensors):
    """DIR/output_<k>.npy, float32.  Over DUMP_LIMIT_BYTES in all, an output larger than its even share of the limit is
    replaced by a fixed sample of its flattened elements (seeded, sorted indices: the same positions from run to run)."""
    import torch
    arrays = [np.ascontiguousarray(t.detach().to(torch.float32).cpu().numpy()) for t in tensors]
    share = DUMP_LIMIT_BYTES // max(1, len(arrays))
    over = sum(a.nbytes for a in arrays) > DUMP_LIMIT_BYTES
    os.makedirs(path, exist_ok=True)
    for k, a in enumerate(arrays):
        if over and a.nbytes > share:
            idx = np.sort(np.random.default_rng(k).choice(a.size, share // 4, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, 'output_%02d.npy' % k), a)


def per_rank_table(world, collective_us):
    """Every rank's {rank, ms_per_step (own clock), host_enqueue_us_per_step, collective_us} gathered to all ranks."""
    import torch.distributed as dist
    mine = dict(rank=int(os.environ.get('RANK', '0')), ms_per_step=round(LAST_TIMED.get('rank_ms_per_step', 0.0), 3),
                host_enqueue_us_per_step=round(LAST_TIMED.get('host_enqueue_us_per_step', 0.0), 1),
                collective_us=collective_us)
    if world == 1:
        return [mine]
    table = [None] * world
    dist.all_gather_object(table, mine)
    return table


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def _spawned_rank(local_rank, world, port, argv):
    """Entry of a rank started by `python bench.py --gpus N` itself (no torch.distributed.run around it)."""
    os.environ.update(RANK=str(local_rank), LOCAL_RANK=str(local_rank), WORLD_SIZE=str(world),
                      MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    sys.argv = [sys.argv[0]] + list(argv)
    main()


def dry_run(args, world, rank):
    """--dry-run: the launcher, the rendezvous, the rank-major all-gather + frame re-ordering view of
    deephar_amd/parallel.py and the one-JSON-line contract on the gloo backend, no HIP device (CPU test of the
    `--gpus N` path; measures nothing about the product)."""
    import torch
    import torch.distributed as dist
    from deephar_amd import parallel
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo', rank=rank, world_size=world)
    clips, T, J, C = 2, 4 * world, 4, 8
    tl = T // world
    local = torch.full((clips, tl, J, C), float(rank))
    buf, us = None, []
    for k in range(args.warmup + args.steps):
        if k == args.warmup:
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
        c0 = time.perf_counter()
        buf = parallel.all_gather_rank_major(local, world=world, out=buf)
        us.append(1e6 * (time.perf_counter() - c0))
        frames = parallel.frames_view(buf).reshape(clips, T, J, C)
        assert all(bool((frames[:, r * tl:(r + 1) * tl] == r).all()) for r in range(world))
    t_local = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    LAST_TIMED.update(rank_ms_per_step=1e3 * t_local / args.steps, host_enqueue_us_per_step=float(np.mean(us[args.warmup:])))
    per_rank = per_rank_table(world, round(float(np.mean(us[args.warmup:])), 2))
    # the strong-scaling leg of the contract line (a FIXED clip batch, T / world frames of it per rank), same collective
    strong = None
    if world > 1 and 8 % world == 0:
        tl_s = 8 // world
        loc = torch.full((clips, tl_s, J, C), float(rank))
        sbuf = None
        dist.barrier()
        s0 = time.perf_counter()
        for _ in range(args.steps):
            sbuf = parallel.all_gather_rank_major(loc, world=world, out=sbuf)
            fr = parallel.frames_view(sbuf).reshape(clips, 8, J, C)
            assert all(bool((fr[:, r * tl_s:(r + 1) * tl_s] == r).all()) for r in range(world))
        dist.barrier()
        sdt = torch.tensor([time.perf_counter() - s0], dtype=torch.float64)
        dist.all_reduce(sdt, op=dist.ReduceOp.MAX)
        strong = {'scaling': 'strong', 'clips_per_step': clips, 'frames_per_rank': tl_s,
                  'value': round(clips * 8 * args.steps / float(sdt), 1), 'unit': 'frames/s'}
    if rank == 0:
        print(json.dumps({'metric': 'dry run of the multi-rank launcher (gloo, CPU): no product measurement', 'per_rank': per_rank,
                          'dry_run': True, 'backend': 'gloo', 'value': round(clips * world * T * args.steps / float(dt), 1),
                          'unit': 'frames/s', 'n_gpus': world, 'rccl_ranks': world, 'steps': args.steps,
                          'warmup': args.warmup, 'ms_per_step': round(1e3 * float(dt) / args.steps, 3),
                          'collective_us': round(float(np.mean(us[args.warmup:])), 2), 'higher_is_better': True,
                          'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
                          'per_rank_ms_min_max': [min(r['ms_per_step'] for r in per_rank), max(r['ms_per_step'] for r in per_rank)],
                          'strong_scaling': strong,
                          'config': {'workload': 'launcher dry run', 'global_batch': clips * world}}))
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--workload', choices=sorted(WORKLOADS), default='mpii')
    ap.add_argument('--full', action='store_true',
                    help='also measure and check what the headline figure does not need: per-kernel pass and roofline, '
                         'CPU baseline, Model.predict boundary, bf16x3 / clip / compact legs, speed2d protocol, serial form')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='write every model output of the last timed step to DIR/output_<k>.npy (float32)')
    ap.add_argument('--batch', type=int, default=None, help='frames (mpii) or clips (clip workloads) per GPU per step')
    ap.add_argument('--blocks', type=int, default=8, help='mpii only')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-predict', action='store_true', help='skip the Model.predict boundary measurement')
    ap.add_argument('--gemm', choices=('f32', 'bf16x3'), default=None,
                    help='GEMM arithmetic of the measured model (default: the product default, f32 = fp32 MFMA)')
    ap.add_argument('--no-bf16x3', action='store_true', help='mpii: skip the split-bf16 leg appended to the line')
    ap.add_argument('--no-clip-leg', action='store_true',
                    help='mpii: skip the short frame-sharded penn_merge run appended to the line')
    ap.add_argument('--no-graph', action='store_true', help='launch kernels eagerly instead of hipGraph replay')
    ap.add_argument('--dump-steps', default=None, help='write the per-kernel profile (JSON) to this path')
    ap.add_argument('--streams', type=int, default=None,
                    help='HIP streams for independent model branches (default: the engine default)')
    ap.add_argument('--stream-policy', choices=('list', 'tail'), default=None,
                    help="with --streams 2: 'tail' = the second stream runs a suffix of the step list (SPNet's action stream "
                         "beside its pose stream; engine/schedule.py)")
    ap.add_argument('--input', choices=('f32', 'u8'), default='f32',
                    help="mpii: f32 = normalised float frames resident in HBM (what the reference's predict() is "
                         "handed); u8 = raw uint8 frames resident in HBM, normalised inside the first convolution")
    ap.add_argument('--tune-cache', default=None,
                    help='JSON file with the autotuned conv tilings: loaded if present (no tuning launches, '
                         'keeps rocprofv3 kernel stats clean), written otherwise')
    ap.add_argument('--force-collective', action='store_true',
                    help='clip workloads at N = 1: issue the RCCL all_gather_into_tensor anyway (a world of one would '
                         'short-cut to a view) -- `collective_us` is then the cost of the RCCL call path on one GPU')
    ap.add_argument('--no-overlap', action='store_true',
                    help='clip workloads: serial stream form (the frame stage of step i + 1 waits for the collective of step i) '
                         'instead of the pipelined one (two send / gather slots, the collective on its own stream)')
    ap.add_argument('--dry-run', action='store_true',
                    help='launcher / rendezvous / all-gather / JSON contract on the gloo backend, no HIP device')
    ap.add_argument('--replay-step', type=int, default=None,
                    help='profiling aid (tools/profile_round.py): bind the workload, run ONE forward, then launch step '
                         'number I of the bound plan(s) --replay-reps times with its in-model arguments and exit; the '
                         'PMC passes of rocprofv3 read the last launches of that kernel')
    ap.add_argument('--replay-reps', type=int, default=4)
    ap.add_argument('--replay-cfg', type=int, default=None,
                    help='with --replay-step on a conv step: force this tiling for the replayed launches (bit-identical; '
                         'lets the PMC passes cover the tilings the autotuner alternates between from box to box)')
    ap.add_argument('--speed2d-clips', type=int, default=250, help='speed2d: clips per timed predict (eval_speed2d.py:30)')
    ap.add_argument('--speed2d-blocks', default=None, help='speed2d: comma list of prediction blocks to time (default: all 18)')
    ap.add_argument('--force-cfg', default=None,
                    help="A/B aid (frame workloads): 'M,K,N:cfg' pins the tiling of every conv launch of that shape "
                         '(bit-identical; the step time of the WHOLE forward under one tiling or another)')
    ap.add_argument('--no-extra-legs', action='store_true',
                    help='mpii at N = 1: skip the compact h36m / ntu_spnet / speed2d legs appended to the line')
    ap.add_argument('--predict-frames', type=int, default=2048,
                    help='frames per Model.predict boundary measurement (SURVEY.md 8d: >= 2 000)')
    ap.add_argument('--pre-predict', default=None,
                    help="diagnostic: run Model.predict on host arrays of an MPII model first ('f32', 'u8', 'alloc': only allocate "
                         "and free the host array) -- does it slow the device-resident step that follows?")
    args = ap.parse_args()

    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` on its own: start the N ranks here (one process per GPU, 127.0.0.1 rendezvous on
        # a free port); every rank re-enters main() with RANK / LOCAL_RANK / WORLD_SIZE set, rank 0 prints the line
        import torch.multiprocessing as mp
        mp.spawn(_spawned_rank, args=(args.gpus, _free_port(), sys.argv[1:]), nprocs=args.gpus, join=True)
        return

    import torch
    import torch.distributed as dist

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.dry_run:
        return dry_run(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a HIP device (the product path has no CPU fallback)')
    torch.cuda.set_device(local_rank)
    if args.pre_predict:
        rng0 = np.random.default_rng(7)
        if args.pre_predict == 'alloc':
            x0 = np.tile(rng0.uniform(-1, 1, (256, 256, 256, 3)).astype(np.float32), (8, 1, 1, 1))
            del x0
        else:
            m0 = build_mpii(8)
            if args.pre_predict == 'u8':
                x0 = np.tile(rng0.integers(0, 256, (256, 256, 256, 3), dtype=np.uint8), (8, 1, 1, 1))
            else:
                x0 = np.tile(rng0.uniform(-1, 1, (256, 256, 256, 3)).astype(np.float32), (8, 1, 1, 1))
            m0.predict(x0, batch_size=64)
            m0.predict(x0, batch_size=64)
            del m0, x0
        import gc
        gc.collect()
    if world > 1 or args.force_collective:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if world == 1:
            os.environ.setdefault('MASTER_PORT', str(_free_port()))
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', local_rank))

    def barrier():
        if world > 1:
            dist.barrier()

    wl = WORKLOADS[args.workload]
    per_gpu = args.batch or wl['per_gpu']
    model = wl['build'](args.blocks) if args.workload == 'mpii' else wl['build']()
    if args.workload in ('h36m', 'speed2d'):
        args.no_bf16x3 = args.no_clip_leg = True
    if args.workload == 'speed2d' and args.streams is None and args.stream_policy is None:
        # the latency regime's engine setting (what INTEGRATION.md recommends for a couple of clips per call): SPNet's action
        # stream on a second stream, one-directional dependencies (engine/schedule.py: assign_streams_tail); measured
        # 6.24 -> 5.01 ms per call, bit-identical.  `--streams 1` gives the one-stream number.
        args.streams, args.stream_policy = 2, 'tail'
    if args.streams is not None:
        model.num_streams = args.streams
    if args.stream_policy is not None:
        model.stream_policy = args.stream_policy
    if args.gemm is not None:
        model.gemm_precision = args.gemm

    def load_tune(ex):
        if args.tune_cache and os.path.exists(args.tune_cache):
            with open(args.tune_cache) as f:
                ex.tune_table.update({tuple(tuple(v) if isinstance(v, list) else v for v in json.loads(k)): c
                                      for k, c in json.load(f).items()})

    def save_tune(tables):
        if args.tune_cache and rank == 0 and not os.path.exists(args.tune_cache):
            merged = {}
            for t in tables:
                merged.update(t)
            with open(args.tune_cache, 'w') as f:
                json.dump({json.dumps(list(k)): v for k, v in merged.items()}, f)

    collective_us = None

    def setup_frames(model, tune=True):
        return setup_frame_workload(model, per_gpu, wl['T'], args, world, rank, load_tune if tune else None,
                                    save_tune if tune else None)

    full_model = None
    if args.workload == 'speed2d':
        # the model a step runs is the truncated model of the LAST prediction block (eval_speed2d.py:62-68, bidx = 17: the
        # last two action outputs, which need every pose and action block before them)
        from deephar_amd import Model
        full_model = model
        nb = len(full_model.outputs) // 2
        model = Model(full_model.input, full_model.outputs[2 * (nb - 1):2 * nb])
        if args.streams is not None:
            model.num_streams = args.streams
        if args.stream_policy is not None:
            model.stream_policy = args.stream_policy
        args.no_bf16x3 = args.no_clip_leg = True

    if not wl['clips']:
        step, bound, streams, frames_per_step, flops_per_step, check, restage = setup_frames(model)
        parallelism = 'frame-shard x%d (replicas, no collective)' % world
        pairs = None
    else:
        (step, pairs, bound, streams, frames_per_step, flops_per_step, check, parallelism, restage) = \
            setup_clips(args.workload, model, per_gpu, world, rank, args, load_tune, save_tune)

    if args.replay_step is not None:
        step()
        for s_ in streams:
            s_.synchronize()
        calls = [(bp, sp, c) for bp, sp in bound for c in bp.calls]
        bp, sp, (fn, cargs, st) = calls[args.replay_step]
        if args.replay_cfg is not None and st.kind == 'conv':
            cargs = (cargs[0], args.replay_cfg)
            st.attrs['tile_cfg'] = args.replay_cfg
        for _ in range(args.replay_reps):
            rc = fn(*cargs, sp)
            assert rc == 0, rc
        torch.cuda.synchronize()
        print(json.dumps({'replayed_step': args.replay_step, 'kind': st.kind, 'name': st.name,
                          'kernel': kernel_name(st) if st.kind == 'conv' else st.kind, 'reps': args.replay_reps,
                          'algorithmic_bytes': st.bytes(bp.n), 'gflop': st.flops(bp.n) / 1e9}))
        return

    dt = timed(step, streams, args.steps, args.warmup, world, pairs)
    ms_per_step = 1e3 * dt / args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_outputs(model, bound, wl['clips']))
    serial_ms = None
    if wl['clips']:
        collective_us = round(1e3 * float(np.mean([a.elapsed_time(b) for a, b in pairs])), 2)
    per_rank = per_rank_table(world, collective_us)           # (a collective: every rank calls it)
    if args.full and wl['clips'] and (world > 1 or args.force_collective):
        serial_ms = serial_form_ms(LAST_SCM[0], step, streams, pairs, world)

    # sanity: outputs finite and in range
    pose = check()
    ok = bool(np.all(np.isfinite(pose)) and pose[..., :2].min() >= 0 and pose[..., :2].max() <= 1)

    # ---- per-kernel pass (HIP events on the launch stream) ----------------------------------------------
    roof, extra, rows = None, {}, []
    if args.full or args.dump_steps:
        restage()
        rows, kinds = profile_plans(bound)
        roof, extra = roofline(rows, kinds, flops_per_step, ms_per_step)
        roof['launches_per_forward'] = real_launches(bound)      # (plan steps minus those absorbed by grouped / paired launches)
        roof['plan_steps'] = len(rows)

    # The full line also measures the opt-in split-bf16 GEMM mode (Model.gemm_precision = 'bf16x3'): same model, same
    # batch, same timing; reported under "bf16x3", never as `value` (the headline stays on the fp32-MFMA path).
    split_leg = None
    if args.full and args.workload == 'mpii' and model.gemm_precision == 'f32' and not args.no_bf16x3:
        sm = wl['build'](args.blocks)
        sm.gemm_precision = 'bf16x3'
        if args.streams is not None:
            sm.num_streams = args.streams
        sstep, sbound, sstreams, sframes, sflops, scheck, srestage = setup_frames(sm, tune=False)
        sdt = timed(sstep, sstreams, args.steps, args.warmup, world, None)
        spose = scheck()
        srestage()
        srows, skinds = profile_plans(sbound)
        sroof, sextra = roofline(srows, skinds, sflops, 1e3 * sdt / args.steps)
        # six bf16 MFMAs per 16 k-values of a 32x32 tile: the matrix-core ceiling in fp32-equivalent FLOP/s
        sroof['peak'] = round(2500.0 / 6.0, 1)
        sroof['peak_note'] = 'dense bf16 MFMA peak (2.5 PFLOP/s) / 6 partial products, in fp32-equivalent TFLOP/s'
        for key in ('frac',):
            sroof[key] = round(sroof['achieved'] / sroof['peak'], 4)
        # v_mfma_f32_32x32x16_bf16 only sustains the nominal rate on constant operands: a bare MFMA stream on random bf16
        # values runs at 1.89 PFLOP/s here (power-limited clock; tools/micro/mfma_data_power.hip,
        # profiles/r02_mfma_data_power.txt).  `frac` stays priced against the nominal peak.
        sroof['frac_of_sustained_on_random_operands'] = round(sroof['achieved'] / (1890.0 / 6.0), 4)
        sroof['all_mfma_conv_kernels']['frac_of_fp32_mfma_peak'] = sroof['all_mfma_conv_kernels'].pop('frac')
        sroof['whole_forward_frac_of_fp32_mfma_peak'] = sroof.pop('whole_forward_frac')
        split_leg = {'value': round(sframes * args.steps / sdt, 1), 'unit': 'frames/s',
                     'ms_per_step': round(1e3 * sdt / args.steps, 3), 'steps': args.steps,
                     'dtype': 'f32 operands split exactly into 3 x bf16, 6 partial products on v_mfma_f32_32x32x16_bf16, '
                              'fp32 accumulate (csrc/gemm1x1s.hip); first conv / BN-prologue convs stay on the fp32 path',
                     'parity': 'same tests and tolerances as the default path: tests/test_gpu_bf16x3.py, '
                               'profiles/parity_r02_bf16x3.json',
                     'outputs_finite_in_range': bool(np.all(np.isfinite(spose)) and spose[..., :2].min() >= 0 and
                                                     spose[..., :2].max() <= 1),
                     'roofline': sroof, 'kernel_time_share': sextra['kernel_time_share']}
        if world == 1 and not args.no_predict:
            sfps = predict_boundary(sm, per_gpu, args.predict_frames)
            split_leg['predict_fps_f32'], split_leg['predict_fps_u8'] = sfps['f32'], sfps['u8']
        del sm

    # The full (mpii) line also carries a short run of the frame-sharded clip path, so that a multi-GPU run of the
    # contract command exercises the RCCL all-gather leg as well (BASELINE.json configs[3]); every rank takes part.
    clip_leg = None
    if args.full and args.workload == 'mpii' and not args.no_clip_leg:
        cw = WORKLOADS['penn_merge']
        cstep, cpairs, _, cstreams, cframes, _, ccheck, cpar, _ = setup_clips('penn_merge', cw['build'](), cw['per_gpu'],
                                                                             world, rank, args)
        cdt = timed(cstep, cstreams, 10, 2, world, cpairs)
        cpose = ccheck()
        clip_leg = {'workload': cw['name'], 'value': round(cframes * 10 / cdt, 1), 'unit': 'frames/s', 'scaling': 'weak',
                    'steps': 10, 'ms_per_step': round(1e2 * cdt, 3), 'parallelism': cpar, 'rccl_ranks': world,
                    'collective_us': round(1e3 * float(np.mean([a.elapsed_time(b) for a, b in cpairs])), 2),
                    'outputs_finite_in_range': bool(np.all(np.isfinite(cpose)) and cpose.min() >= 0 and cpose.max() <= 1)}
        if world > 1 or args.force_collective:
            cser = serial_form_ms(LAST_SCM[0], cstep, cstreams, cpairs, world)
            if cser is not None:
                clip_leg['serial_form_ms_per_step'] = round(cser, 3)
                clip_leg['hidden_by_pipelining_us'] = round(1e3 * cser - 1e5 * cdt, 1)
        if world > 1:
            # [r06] ... and the same model under STRONG scaling: the 4 clips of the one-GPU step whatever the world, T / N
            # frames of them per rank -- the curve that shows what the collective and the replicated head cost
            del cstep, ccheck
            sstep, spairs, _, sstreams, sframes, _, scheck, spar, _ = setup_clips('penn_merge', cw['build'](), cw['per_gpu'], world,
                                                                             rank, args, total_clips=cw['per_gpu'])
            sdt_ = timed(sstep, sstreams, 10, 2, world, spairs)
            clip_leg['strong_scaling'] = {'clips_per_step': cw['per_gpu'], 'value': round(sframes * 10 / sdt_, 1), 'unit': 'frames/s',
                                          'scaling': 'strong', 'steps': 10, 'ms_per_step': round(1e2 * sdt_, 3), 'parallelism': spar,
                                          'collective_us': round(1e3 * float(np.mean([a.elapsed_time(b) for a, b in spairs])), 2)}

    # [r06] ... and, at N = 1, compact legs of the other BASELINE configurations and of the reference's speed protocol
    extra_legs = {}
    if args.full and args.workload == 'mpii' and world == 1 and not args.no_extra_legs and not args.no_clip_leg \
            and args.input == 'f32' and model.gemm_precision == 'f32':
        for w in ('h36m', 'ntu_spnet', 'speed2d'):
            extra_legs[w] = compact_leg(w, args, rank)

    if rank == 0:
        out = {
            'metric': 'frames/sec whole-node, 256x256 MPII pose fwd' if args.workload == 'mpii' else
                      'frames/sec whole-node, 256x256 Human3.6M 3-D pose fwd' if args.workload == 'h36m' else
                      'frames/sec, SPNet-Penn 2-D pose + action, 8-frame clips, 2 clips per call (eval_speed2d.py protocol, '
                      'last prediction block)' if args.workload == 'speed2d' else
                      'frames/sec whole-node, 256x256 pose + action fwd (%s)' % args.workload,
            'value': round(frames_per_step * args.steps / dt, 1),
            'unit': 'frames/s',
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(ms_per_step, 3),
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': None,
            'dtype': 'f32' if model.gemm_precision == 'f32' else 'f32 (operands split exactly into 3 x bf16, fp32 accumulate)',
            'data': 'synthetic',
            'config': {'workload': wl['name'] if args.workload != 'mpii' or (args.blocks == 8 and per_gpu == 64) else
                       'MPII single-person 256x256, ReceptionNet %d blocks, batch=%d per GPU' % (args.blocks, per_gpu),
                       'global_batch': per_gpu * world, 'frames_per_step': frames_per_step, 'parallelism': parallelism,
                       'hipgraph': not args.no_graph, 'streams': model.plan.nstreams, 'input': args.input,
                       'gemm': model.gemm_precision,
                       'outputs_finite_in_range': ok},
            'full': args.full,
        }
        if roof is not None:
            out['roofline'] = roof
        out.update(extra)
        out['per_rank'] = per_rank
        if collective_us is not None:
            out['collective_us'] = collective_us
            out['rccl_ranks'] = world
            out['collective_forced_at_world_1'] = bool(world == 1 and args.force_collective)
            out['stream_form'] = 'serial' if args.no_overlap else 'pipelined (frame stage of step i + 1 beside the all-gather ' \
                                 'and head stage of step i: two send / gather slots, collective on its own stream)'
            if serial_ms is not None:
                out['serial_form_ms_per_step'] = round(serial_ms, 3)
                out['hidden_by_pipelining_us'] = round(1e3 * (serial_ms - ms_per_step), 1)
        ms_ranks = [r['ms_per_step'] for r in per_rank]
        out['per_rank_ms_min_max'] = [min(ms_ranks), max(ms_ranks)]
        if clip_leg is not None:
            out['frame_sharded_clips'] = clip_leg
        if split_leg is not None:
            out['bf16x3'] = split_leg
        out.update(extra_legs)
        if args.full and args.workload == 'mpii' and world == 1 and not args.no_predict:
            fps = predict_boundary(model, per_gpu, args.predict_frames)
            out['predict_fps_f32'], out['predict_fps_u8'] = fps['f32'], fps['u8']
            out['predict_note'] = 'Model.predict on host numpy arrays, %d frames in batches of %d, wall clock incl. ' \
                                  'H2D of the frames and D2H of all outputs, after one warm-up call' % (
                                      args.predict_frames, per_gpu)
        if args.full and args.workload == 'speed2d' and world == 1 and not args.no_predict:
            out['speed2d'] = speed2d_protocol(full_model, args, model.executor.tune_table)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(full_model if full_model is not None else model, args.workload, args.blocks)
        if args.dump_steps:
            dump = [dict(kind=s.kind, name=s.name, kernel=kernel_name(s) if s.kind == 'conv' else s.kind,
                         ms=ms, gflop=s.flops(n) / 1e9, mbytes=s.bytes(n) / 1e6, absorbed=id(s) in ABSORBED,
                         out=list(next(iter(s.outs.values())).shape) if s.outs else None) for s, ms, n in rows]
            with open(args.dump_steps, 'w') as f:
                json.dump(dump, f, indent=1)
        # RCCL writes its version banner through C stdio, which a redirected stdout holds back until exit -- behind the JSON
        # line.  Flush it first: the contract line is the LAST line this process prints.
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
    if world > 1 or args.force_collective:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
