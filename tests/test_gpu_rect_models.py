"""Whole models on non-square and on larger frames: Model.predict against the fp64 CPU oracle.

Every other model test builds its network at 256 x 256 or 128 x 128.  A landscape and a portrait crop are different plans
(tests/test_rect_host.py): 24 x 32 maps pool in the convolution epilogue (W == 32) and open with the first-layer kernel
(128 output columns), 32 x 24 maps do neither; SPNet at 128 x 192 pools in 5 launches, at 192 x 128 in 3; its read-out maps
run from 16 x 24 down to 2 x 3.  Maps of 48 x 48 and 40 x 52 are beyond the LDS slab of the fused 2-D decoder: the planner
keeps the two read-outs and the aggregation apart there (rule R5b; before it knew the limit, predict raised).

Bars: those of tests/test_gpu_models.py -- coordinates at the flat 1e-3 px against fp64 (paritylog.check records
|hip - fp64| next to |fp32 oracle - fp64|), SPNet on per-pixel noise through spnet_parity's conditioned stress check.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paritylog                                   # noqa: E402
from paritylog import PX_TOL, check as _check      # noqa: E402
from test_gpu_models import _build, _oracle, _spnet, spnet_parity      # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = [(192, 256), (256, 192)]
CTX = dict(num_context_per_joint=2, concat_pose_confidence=False)
_ids = lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s)


def _frames(seed, n, frame):
    return np.random.default_rng(seed).uniform(-1, 1, (n,) + frame + (3,)).astype(np.float32)


def _first_layer_rule(hip_lib, m, n):
    """dh_conv2d_uses_first_layer_kernel of the model's first convolution as the engine bound it for batch n"""
    from deephar_amd.engine import binding
    from deephar_amd import _lib
    name, structs, _ = binding.bind(m.plan.steps[0], n, binding.FakeEnv(n))
    assert name == 'dh_conv2d_f32' and isinstance(structs[0], _lib.ConvArgs) and structs[0].Cin == 3
    structs[0].w = 16                                   # (any non-null address: the rule reads the geometry)
    return hip_lib.dh_conv2d_uses_first_layer_kernel(C.byref(structs[0]))


def _readout(plan):
    return [s.kind for s in plan.steps if s.kind in ('sam', 'sam_ctx', 'context_agg')]


# ---- ReceptionNet at 192 x 256 and 256 x 192 ------------------------------------------------------------------------------
@pytest.mark.parametrize('frame', FRAMES, ids=_ids)
def test_reception_2d_context_on_non_square_frames(frame, hip_lib, cuda):
    """J = 16, two contexts per joint, 2 blocks, batch 2, seeds 0 and 1: poses at the flat 1e-3 px, visibility at 1e-5
    relative; context confidences away from the aggregation's pole, heat maps neither flat nor one-hot.  The plan is the one
    of its orientation: pooled second outputs and the first-layer kernel at W = 32 / 128 output columns only."""
    m, wd = _build(2, 2, 16, input_shape=frame + (3,), **CTX)
    H, W = frame[0] // 8, frame[1] // 8
    sams = [s for s in m.plan.steps if s.kind == 'sam_ctx']
    assert len(sams) == 2 and all(s.ins['h'].shape[-3:-1] == (H, W) for s in sams)
    pooled = sum(1 for s in m.plan.steps if s.outs.get('ypool') is not None)
    assert (pooled > 0) == (W == 32), (W, pooled)
    assert _first_layer_rule(hip_lib, m, 2) == (1 if frame[1] // 2 == 128 else 0)
    for seed in (0, 1):
        x = _frames(seed, 2, frame)
        hip = m.predict(x, batch_size=2)
        o32, _ = _oracle(wd, x, 2, 2, 16, torch.float32, **CTX)
        o64, t64 = _oracle(wd, x, 2, 2, 16, torch.float64, **CTX)
        assert len(hip) == 4 and [h.shape for h in hip] == [o.shape for o in o64]
        for b in range(2):
            vc = t64['vc%d' % (b + 1)].reshape(2, 16, 2).sum(axis=2)
            assert np.all(vc > 1.0), 'synthetic context confidences too close to 0'
            _check('pose%d.%s.seed%d' % (b + 1, _ids(frame), seed), hip[2 * b], o32[2 * b], o64[2 * b], PX_TOL)
            _check('vis%d.%s.seed%d' % (b + 1, _ids(frame), seed), hip[2 * b + 1], o32[2 * b + 1], o64[2 * b + 1], 1e-5, rel=True)
        assert t64['heatmaps2'].shape[1:3] == (H, W) and 1.0 < t64['heatmaps2'].std() < 30.0


@pytest.mark.parametrize('frame', FRAMES, ids=_ids)
def test_reception_3d_on_non_square_frames(frame, hip_lib, cuda):
    """J = 17, 16 depth maps, 2 blocks, batch 2, seeds 0 and 1: xyz at the flat 1e-3 px, visibility at 1e-6."""
    m, wd = _build(3, 2, 17, input_shape=frame + (3,), depth_maps=16)
    H, W = frame[0] // 8, frame[1] // 8
    assert all(s.ins['h'].shape[-3:-1] == (H, W) for s in m.plan.steps if s.kind in ('sam', 'depth_means'))
    assert (sum(1 for s in m.plan.steps if s.outs.get('ypool') is not None) > 0) == (W == 32)
    for seed in (0, 1):
        x = _frames(seed, 2, frame)
        hip = m.predict(x, batch_size=2)
        o32, _ = _oracle(wd, x, 3, 2, 17, torch.float32, depth_maps=16)
        o64, _ = _oracle(wd, x, 3, 2, 17, torch.float64, depth_maps=16)
        assert len(hip) == 2 and hip[0].shape == (2, 17, 4)
        for b in range(2):
            _check('xyz%d.%s.seed%d' % (b + 1, _ids(frame), seed), hip[b][..., :3], o32[b][..., :3], o64[b][..., :3], PX_TOL)
            _check('vis%d.%s.seed%d' % (b + 1, _ids(frame), seed), hip[b][..., 3:], o32[b][..., 3:], o64[b][..., 3:], 1e-6)


# ---- maps beyond the fused decoder's LDS slab ----------------------------------------------------------------------------------
@pytest.mark.parametrize('frame', [(384, 384), (320, 416)], ids=_ids)
def test_reception_2d_context_on_maps_beyond_the_fused_decoder(frame, hip_lib, cuda):
    """48 x 48 and 40 x 52 maps, 1 block, batch 1, seeds 0 and 1: two soft-argmax launches (the unstaged narrow kernel) and one
    aggregation in place of dh_softargmax2d_context_f32, which refuses such maps -- same bars."""
    m, wd = _build(2, 1, 16, input_shape=frame + (3,), **CTX)
    assert _readout(m.plan) == ['sam', 'sam', 'context_agg']
    for seed in (0, 1):
        x = _frames(seed, 1, frame)
        hip = m.predict(x, batch_size=1)
        o32, _ = _oracle(wd, x, 2, 1, 16, torch.float32, **CTX)
        o64, t64 = _oracle(wd, x, 2, 1, 16, torch.float64, **CTX)
        assert np.all(t64['vc1'].reshape(1, 16, 2).sum(axis=2) > 1.0)
        _check('pose.%s.seed%d' % (_ids(frame), seed), hip[0], o32[0], o64[0], PX_TOL)
        _check('vis.%s.seed%d' % (_ids(frame), seed), hip[1], o32[1], o64[1], 1e-5, rel=True)
        assert 1.0 < t64['heatmaps1'].std() < 30.0


# ---- SPNet at 128 x 192 and 192 x 128 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frame,pools', [((128, 192), 5), ((192, 128), 3)], ids=_ids)
def test_spnet_on_non_square_clips(frame, pools, hip_lib, cuda):
    """pa16j2d, T = 4, two pyramids, actions on both, pose_replica, calibrated heads; read-out maps 16 x 24 down to 2 x 3 (and
    transposed).  Through spnet_parity (the conditioned check of the per-pixel-noise cases) with identical arg-max labels."""
    x = np.random.default_rng(11).uniform(-1, 1, (1, 4) + frame + (3,)).astype(np.float32)
    m, cfg, wd, ocfg = _spnet(4, 'pa16j2d', 15, 2, [1, 2], 160, replica=True, calibrate=x, input_shape=(4,) + frame + (3,))
    assert sum(1 for s in m.plan.steps if s.kind == 'pool') == pools
    maps = sorted({s.ins['h'].shape[-3:-1] for s in m.plan.steps if s.kind == 'sam'})
    assert maps == sorted((frame[0] >> k, frame[1] >> k) for k in (3, 4, 5, 6)), maps
    spnet_parity(m, cfg, wd, ocfg, x, 2, [1, 2])


# ---- engine settings on the (192, 256) 2-D model ---------------------------------------------------------------------------------
def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_engine_settings_are_bit_identical_on_non_square_frames(hip_lib, cuda, tmp_path):
    """192 x 256 frames: the exported C plan (dh_forward), two streams, raw uint8 frames against host-normalised ones and
    batch 1 against batch 2 return the bits of Model.predict."""
    from test_gpu_plan_api import _plan
    from deephar_amd.utils.transform import normalize_channels
    frame = (192, 256)
    m, _ = _build(2, 2, 16, input_shape=frame + (3,), **CTX)
    x = _frames(7, 2, frame)
    ref = m.predict(x, batch_size=2)
    # batch 1 against batch 2
    one = [m.predict(x[k:k + 1], batch_size=1) for k in range(2)]
    assert _same([np.concatenate([one[0][i], one[1][i]]) for i in range(len(ref))], ref)
    # the C plan
    path = str(tmp_path / 'rect.dhplan')
    nbytes = m.export_plan(path, 2)
    blob = open(path, 'rb').read()
    assert len(blob) == nbytes
    plan = _plan(hip_lib, blob)
    try:
        assert hip_lib.dh_plan_input_items(plan, 0) == x[0].size
        xd = torch.from_numpy(x).to(cuda)
        outs = [torch.full(r.shape, float('nan'), device=cuda) for r in ref]
        ins_p = (C.c_void_p * 1)(xd.data_ptr())
        outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        assert hip_lib.dh_forward(plan, ins_p, 2, outs_p, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert _same([o.cpu().numpy() for o in outs], ref)
    finally:
        assert hip_lib.dh_plan_destroy(plan) == 0
    # raw uint8 frames
    frames = np.random.default_rng(5).integers(0, 256, x.shape, dtype=np.uint8)
    host = normalize_channels(frames.astype(np.float32))
    assert host.dtype == np.float32
    assert _same(m.predict(frames, batch_size=2), m.predict(host, batch_size=2))
    # two streams (last: it re-plans)
    m.num_streams = 2
    assert m.plan.nstreams == 2
    assert _same(m.predict(x, batch_size=2), ref) and _same(m.predict(x, batch_size=2), ref)        # capture, then replay


@pytest.mark.parametrize('mode', ['bf16x3', 'bf16'])
def test_gemm_precision_modes_on_non_square_frames(mode, hip_lib, cuda, monkeypatch):
    """Model.gemm_precision on the 192 x 256 model under the rule of test_gpu_bf16_modes.test_models_within_the_emulated_bar:
    the engine stays within max(1e-3 px, 2 x emu_px) of the fp64 oracle, emu_px being the distance of the CPU emulation of the
    mode (tests/bf16_modes_ref.py) from it; the mode is engaged and differs from the fp32 path."""
    import bf16_modes_ref as B
    frame = (192, 256)
    m, wd = _build(2, 2, 16, input_shape=frame + (3,), **CTX)
    x = _frames(0, 2, frame)
    oracle = lambda dt: _oracle(wd, x, 2, 2, 16, dt, **CTX)[0]
    poses = lambda o: [v[..., :2] for v in o[::2]]
    o64 = oracle(torch.float64)
    f32 = m.predict(x, batch_size=2)
    with monkeypatch.context() as mp:
        B.emulate(mp, B.PARTS[mode])
        emu = oracle(torch.float64)
    emu_px = B.px(poses(emu), poses(o64))
    m.gemm_precision = mode
    hip = m.predict(x, batch_size=2)
    nsplit = sum(1 for s in m.plan.steps if s.kind == 'conv' and s.attrs.get('w_split'))
    hip_px, vs_f32 = B.px(poses(hip), poses(o64)), B.px(poses(hip), poses(f32))
    bar = max(1e-3, 2.0 * emu_px)
    print('%s at 192 x 256: emulation %.3e px, engine %.3e px from fp64 (bar %.3e), %.3e px from the fp32 path, %d split convs'
          % (mode, emu_px, hip_px, bar, vs_f32, nsplit))
    cat = lambda outs: np.concatenate([np.asarray(v, np.float64).ravel() for v in poses(outs)])
    paritylog.record('rect192x256.%s.pose' % mode, cat(hip), cat(oracle(torch.float32)), cat(o64), case='rect_bf16_modes',
                     mode=mode, emu_px=emu_px, bar_px=bar)
    assert all(np.all(np.isfinite(v)) for v in hip)
    assert nsplit >= 20, nsplit
    assert vs_f32 > 0, 'the %s plan returned the fp32 path\'s bits' % mode
    assert hip_px <= bar, '%s: %.3e px from the fp64 oracle, bar %.3e px (emulation %.3e px)' % (mode, hip_px, bar, emu_px)


# ---- the reference code's own outputs on non-square frames --------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['rec2d_rect', 'rec2d_rect_t', 'rec3d_rect', 'spnet2dr_rect'])
def test_hip_matches_reference_code_goldens_on_non_square_frames(tag, hip_lib, cuda):
    """The engine against the golden vectors the reference's own model code produced on 192 x 256, 256 x 192 and (SPNet)
    128 x 192 frames (tests/golden/make_reference_golden.py --rect), under the rules of
    test_gpu_models.test_hip_matches_reference_code_goldens: coordinates within a flat 1e-3 px of the reference code's fp64
    run; the SPNet golden (per-pixel noise, un-calibrated heads) as a stress case with identical arg-max labels."""
    from refgolden import build_case, golden
    m, x, run = build_case(tag)
    g32, g64 = golden(tag)
    hip = m.predict(x.astype(np.float32), batch_size=len(x))
    hip = hip if isinstance(hip, list) else [hip]
    assert [h.shape for h in hip] == [g.shape for g in g64]
    tols = None
    if tag.startswith('spnet'):
        t64 = {}
        run(torch.float64, taps=t64)
        tols = [paritylog.conditioned_tolerance(t64[k], t64.get(k[:-len('/logits')] + '/dlogits'))
                for k in t64 if k.endswith('/logits')]
    for k, (h, a, b) in enumerate(zip(hip, g32, g64)):
        if b.ndim == 2 and tag.startswith('spnet'):
            _check('%s.act%d' % (tag, k), h, a, b, 1e-5)
            assert np.array_equal(h.argmax(-1), b.argmax(-1))
        elif tols is not None:
            flat = lambda v: v.reshape((-1,) + v.shape[-2:])
            txy, _, tc = tols[k]
            paritylog.check_conditioned('%s.out%d.xy' % (tag, k), flat(h)[..., :2], flat(a)[..., :2], flat(b)[..., :2], txy)
            paritylog.check_conditioned('%s.out%d.c' % (tag, k), flat(h)[..., 2], flat(a)[..., 2], flat(b)[..., 2], tc, px=False)
        elif tag == 'rec3d_rect':           # [N, 17, 4] = xyz + visibility
            _check('%s.xyz%d' % (tag, k), h[..., :3], a[..., :3], b[..., :3], PX_TOL)
            _check('%s.vis%d' % (tag, k), h[..., 3:], a[..., 3:], b[..., 3:], 1e-6)
        else:                               # pose [N, 16, 2], visibility [N, 16, 1] per block
            _check('%s.out%d' % (tag, k), h, a, b, PX_TOL if b.shape[-1] != 1 else 1e-5, rel=(b.shape[-1] == 1))
