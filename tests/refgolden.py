"""Shared description of the golden cases produced by tests/golden/make_reference_golden.py (the reference's own
model code executed on oracle/refrun/minikeras.py in the build container)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_models.npz')
# the '<tag>_s' cases: SPNet on well-conditioned vectors (tests/wellcond.py: video clips + fitted heat-map heads);
# the fitted head kernels travel with the outputs, so a test rebuilds exactly the weights the reference code ran on
GOLDEN_SMOOTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_models_smooth.npz')
# [r05] the '<tag>' cases of REAL_CASES: the BASELINE configurations at their real size (8 blocks at 256 px; the merge
# model exactly as exp/pennaction/eval_penn_ar_pe_merge.py:51-57 builds it: T = 16, 4 blocks, nine action heads;
# SPNet-NTU at T = 32 / 256 px, where spnet.py:100 switches time_stride to 2) -- outputs only
GOLDEN_REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_models_real.npz')
# the '<tag>_rect' cases: non-square frames, (rows, columns) in RECT_FRAMES -- 2-block ReceptionNet 2-D with context in both
# orientations, 2-block ReceptionNet 3-D, and the SPNet of tests/test_gpu_rect_models.py (T = 4, two pyramids, actions on both,
# pose_replica) on per-pixel-noise clips with un-calibrated heads (a stress case like 'spnet2dr') -- outputs only
GOLDEN_RECT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_models_rect.npz')
RECT_FRAMES = {'rec2d_rect': (192, 256), 'rec2d_rect_t': (256, 192), 'rec3d_rect': (192, 256), 'spnet2dr_rect': (128, 192)}
SPNET_CASES = {'spnet3d': (4, 'pa17j3d', 60, 2, [1, 2], 192, False),
               'spnet2d': (16, 'pa16j2d', 15, 2, [2], 160, False),
               'spnet2dr': (8, 'pa16j2d', 15, 6, [5, 6], 160, True),
               'spnet3d_32': (32, 'pa17j3d', 60, 2, [1, 2], 192, False),
               # [r06] the model of the reference's speed protocol, exp/pennaction/eval_speed2d.py:31-43: six pyramids,
               # actions on ALL six, pose_replica=True, 8-frame clips at 256 px (18 pose + 18 action outputs)
               'spnet2d_speed': (8, 'pa16j2d', 15, 6, [1, 2, 3, 4, 5, 6], 160, True),
               'spnet2dr_rect': (4, 'pa16j2d', 15, 2, [1, 2], 160, True)}
SPNET_RES = {'spnet3d_32': 256, 'spnet2d_speed': 256}          # input resolution (default 128)
# seed of the video clip / peak positions of a '<tag>_s' case (31 + the case's rank among the round-5 cases; fixed numbers
# since round 6 so that a new case does not move the old ones)
SMOOTH_SEEDS = {'spnet2d': 31, 'spnet2dr': 32, 'spnet3d': 33, 'spnet3d_32': 34, 'spnet2d_speed': 35}
# cases whose heads are fitted with one bisection factor PER JOINT (wellcond._scale_per_joint, the round-4 rule of
# tests/test_gpu_spnet_flat.py); the others keep the common factor their committed goldens were made with.  [r06]
# 'spnet3d_32' moved here: under the common factor the reference code's own fp32 run sat 1.0e-3 px from its fp64 run
# (a vector that cannot resolve the bar in plain fp32)
FIT_PER_JOINT = ('spnet3d_32', 'spnet2d_speed')


def case_input(tag, shape):
    seed = int.from_bytes(tag.encode(), 'little') % (2 ** 31)
    return np.random.default_rng(seed).uniform(-1, 1, shape)


def smooth_input(tag, res=None):
    """(clips float32 [1, T, res, res, 3], peak positions [T, J, 2]) of a '<tag>_s' case."""
    import wellcond
    from deephar_amd import utils
    T, lay = SPNET_CASES[tag[:-2]][:2]
    res = res or SPNET_RES.get(tag[:-2], 128)
    J = getattr(utils, lay).num_joints
    seed = SMOOTH_SEEDS[tag[:-2]]
    return wellcond.video_clips(1, T, res, seed), wellcond.joint_positions(1, T, J, seed)


def spnet_ocfg(tag):
    from deephar_amd import utils
    T, lay, nact, pyr, apyr, feats, rep = SPNET_CASES[tag[:-2] if tag.endswith('_s') else tag]
    layout = getattr(utils, lay)
    return dict(num_joints=layout.num_joints, dim=layout.dim, num_actions=[nact], num_pyramids=pyr,
                action_pyramids=apyr, num_levels=4, kernel_size=(5, 5), growth=96, image_div=8,
                num_pose_features=feats, num_visual_features=feats, sam_alpha=1, pose_replica=rep)


def golden_file(tag):
    return GOLDEN_RECT if tag in RECT_CASES else GOLDEN_REAL if tag in REAL_CASES else GOLDEN_SMOOTH if tag.endswith('_s') else GOLDEN


def golden(tag):
    g = np.load(golden_file(tag))
    n = int(g['%s/nout' % tag])
    return [g['%s/f32/%d' % (tag, i)] for i in range(n)], [g['%s/f64/%d' % (tag, i)] for i in range(n)]


def build_case(tag):
    """-> (product model with synthetic weights, input array float64, callable running the CPU oracle(dtype))"""
    import torch
    from deephar_amd import graph, weights, utils
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import reception, action, spnet
    from oracle import reception as oref, action as oact, spnet as osp
    graph.reset_naming()
    if tag == 'rec2d':
        kw = dict(num_context_per_joint=2, num_blocks=2, ksize=(5, 5), concat_pose_confidence=False)
        m = reception.build((256, 256, 3), 16, dim=2, **kw)
        x = case_input(tag, (2, 256, 256, 3))
        run = lambda wd, dt: oref.forward(wd, x, 16, 2, dtype=dt, **kw)
    elif tag == 'rec3d':
        kw = dict(num_blocks=2, depth_maps=16, ksize=(5, 5), export_heatmaps=True)
        m = reception.build((256, 256, 3), 17, dim=3, **kw)
        x = case_input(tag, (2, 256, 256, 3))
        run = lambda wd, dt: oref.forward(wd, x, 17, 3, dtype=dt, **kw)
    elif tag in ('rec2d_rect', 'rec2d_rect_t'):
        kw = dict(num_context_per_joint=2, num_blocks=2, ksize=(5, 5), concat_pose_confidence=False)
        m = reception.build(RECT_FRAMES[tag] + (3,), 16, dim=2, **kw)
        x = case_input(tag, (2,) + RECT_FRAMES[tag] + (3,))
        run = lambda wd, dt: oref.forward(wd, x, 16, 2, dtype=dt, **kw)
    elif tag == 'rec3d_rect':
        kw = dict(num_blocks=2, depth_maps=16, ksize=(5, 5))
        m = reception.build(RECT_FRAMES[tag] + (3,), 17, dim=3, **kw)
        x = case_input(tag, (2,) + RECT_FRAMES[tag] + (3,))
        run = lambda wd, dt: oref.forward(wd, x, 17, 3, dtype=dt, **kw)
    elif tag == 'rec2d_8':      # configs[1]: 8 blocks, 2 contexts per joint (exp/mpii/eval_mpii_singleperson.py:46-50)
        kw = dict(num_context_per_joint=2, num_blocks=8, ksize=(5, 5), concat_pose_confidence=False)
        m = reception.build((256, 256, 3), 16, dim=2, **kw)
        x = case_input(tag, (2, 256, 256, 3))
        run = lambda wd, dt: oref.forward(wd, x, 16, 2, dtype=dt, **kw)
    elif tag == 'rec3d_8':      # configs[2]: 8 blocks, J = 17, 16 depth maps (exp/h36m/eval_h36m.py:42-48)
        kw = dict(num_blocks=8, depth_maps=16, ksize=(5, 5))
        m = reception.build((256, 256, 3), 17, dim=3, **kw)
        x = case_input(tag, (2, 256, 256, 3))
        run = lambda wd, dt: oref.forward(wd, x, 17, 3, dtype=dt, **kw)
    elif tag == 'merge2d_16':   # configs[3]: exp/pennaction/eval_penn_ar_pe_merge.py:51-57 (nine action heads, no poses)
        pe = reception.build((256, 256, 3), 16, dim=2, num_blocks=4, num_context_per_joint=2, ksize=(5, 5),
                             concat_pose_confidence=False)
        m = action.build_merge_model(pe, 15, (256, 256, 3), 16, 16, 4, pose_dim=2, pose_net_version='v1',
                                     full_trainable=False)
        x = case_input(tag, (1, 16, 256, 256, 3))
        okw = dict(pose_dim=2, pose_net_version='v1', output_poses=False, num_context_per_joint=2)
        run = lambda wd, dt: oact.forward_merge(wd, x, 15, 16, 4, dtype=dt, **okw)
    elif tag in ('merge2d', 'merge3d'):
        dim, J, ver = (2, 16, 'v1') if tag == 'merge2d' else (3, 20, 'v2')
        pe_kw = dict(num_context_per_joint=2, num_blocks=2, ksize=(5, 5)) if dim == 2 else \
            dict(num_blocks=2, depth_maps=8, ksize=(5, 5))
        pe = reception.build((128, 128, 3), J, dim=dim, **pe_kw)
        m = action.build_merge_model(pe, 15, (128, 128, 3), 4, J, 2, pose_dim=dim, depth_maps=8,
                                     pose_net_version=ver, output_poses=True)
        x = case_input(tag, (2, 4, 128, 128, 3))
        okw = dict(pose_dim=dim, depth_maps=8, pose_net_version=ver, output_poses=True,
                   num_context_per_joint=2 if dim == 2 else 0)
        run = lambda wd, dt: oact.forward_merge(wd, x, 15, J, 2, dtype=dt, **okw)
    elif tag in SPNET_CASES or (tag.endswith('_s') and tag[:-2] in SPNET_CASES):
        T, lay, nact, pyr, apyr, feats, rep = SPNET_CASES[tag[:-2] if tag.endswith('_s') else tag]
        layout = getattr(utils, lay)
        res = SPNET_RES.get(tag[:-2] if tag.endswith('_s') else tag, 128)
        rows, cols = RECT_FRAMES.get(tag, (res, res))
        cfg = ModelConfig((T, rows, cols, 3), layout, num_actions=[nact], num_pyramids=pyr, action_pyramids=apyr,
                          num_levels=4, pose_replica=rep, num_pose_features=feats, num_visual_features=feats)
        m = spnet.build(cfg)
        x = smooth_input(tag)[0] if tag.endswith('_s') else case_input(tag, (1, T, rows, cols, 3))
        ocfg = spnet_ocfg(tag)
        run = lambda wd, dt, taps=None: osp.forward(wd, x, ocfg, dtype=dt, taps=taps)
    else:
        raise KeyError(tag)
    weights.init_synthetic(m, seed=0)
    if tag.endswith('_s'):
        import wellcond
        g = np.load(golden_file(tag))
        pre = '%s/head/' % tag
        wellcond.apply_heads(m, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
    wd = weights.as_dict(m)
    return m, x, (lambda dt, **kw: run(wd, dt, **kw))


CASES = ['rec2d', 'rec3d', 'merge2d', 'merge3d', 'spnet3d', 'spnet2d', 'spnet2dr']
SMOOTH_CASES = ['spnet3d_s', 'spnet2d_s', 'spnet2dr_s']
RECT_CASES = ['rec2d_rect', 'rec2d_rect_t', 'rec3d_rect', 'spnet2dr_rect']
REAL_CASES = ['rec2d_8', 'rec3d_8', 'merge2d_16', 'spnet3d_32_s', 'spnet2d_speed_s']
