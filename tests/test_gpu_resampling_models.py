"""GPU graph / model tests of the learned-resampling flavour (downsampling_type='conv'): a mini pyramid out of the public
builders, the pose-only SPNet against the fp64 / fp32 restatement of tests/resample_ref.py, and a clip SPNet with actions
across engine settings and through the C-level plan executor."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paritylog                                   # noqa: E402
import resample_ref as R                           # noqa: E402
import wellcond                                    # noqa: E402
from paritylog import PX_TOL                       # noqa: E402

pytestmark = pytest.mark.gpu


def _all_off():
    from deephar_amd.engine.rules import RuleSet
    return RuleSet(**{f.name: False for f in dataclasses.fields(RuleSet) if f.type is bool})


# ---- 9. mini pyramid ------------------------------------------------------------------------------------------------------
MINI_LAYERS, _mini_pyramid = R.MINI_LAYERS, R.build_mini_pyramid      # (shared with the host tests)


@pytest.fixture(scope='module')
def mini():
    m, wd = _mini_pyramid()
    x = np.random.default_rng(21).standard_normal((2, 16, 16, 96)).astype(np.float32)
    return wd, x, R.mini_pyramid(wd, x, dtype=torch.float32), R.mini_pyramid(wd, x, dtype=torch.float64)


@pytest.mark.parametrize('rules', ['default', 'all_off'])
def test_mini_pyramid(rules, mini, hip_lib, cuda):
    """Three down-scaling and three up-scaling units with lateral adds, [2, 16, 16, 96] -> 2 x 2 x 192 -> [2, 16, 16, 96].
    Tolerance: tests/test_gpu_ops.py compares ONE fused convolution with atol 3e-5 + rtol 2e-5 (fp32 sums in another
    order: a few ulp times sqrt(K)); the longest path here crosses MINI_LAYERS = 9 such layers whose synthetic weights keep
    the activations O(1) (unit gain per layer), so the per-layer errors add at worst linearly: 9 x that tolerance.  And the
    result is no further from fp64 than a few times the fp32 CPU restatement."""
    from deephar_amd.engine.rules import RuleSet
    wd, x, o32, o64 = mini
    m, wd2 = _mini_pyramid()
    assert all(np.array_equal(wd[k], wd2[k]) for k in wd)
    m.rules = RuleSet() if rules == 'default' else _all_off()
    kinds = [s.kind for s in m.plan.steps]
    assert kinds.count('convtranspose') == 3 and sum(1 for s in m.plan.steps if s.kind == 'dwconv' and s.attrs.get('sh') == 2) == 3
    assert ('eltwise' in kinds) == (rules == 'all_off')
    got = m.predict(x, batch_size=2)
    assert got.shape == o64.shape == (2, 16, 16, 96) and np.all(np.isfinite(got))
    err = np.abs(got - o32)
    tol = MINI_LAYERS * (3e-5 + 2e-5 * np.abs(o32))
    e_hip, e_cpu = np.abs(got - o64).max(), np.abs(o32 - o64).max()
    print('mini pyramid [%s]: |hip - o32| %.3e (tol at that element %.3e), |hip - o64| %.3e, |o32 - o64| %.3e, |y| max %.2f'
          % (rules, err.max(), tol.flat[err.argmax()], e_hip, e_cpu, np.abs(o64).max()))
    assert np.all(err <= tol)
    assert e_hip <= 4 * e_cpu + 1e-6
    # one frame alone gives the bits it has inside the batch
    assert np.array_equal(m.predict(x[:1], batch_size=1), got[:1])


# ---- 10. pose-only SPNet ----------------------------------------------------------------------------------------------------
def _pose_spnet(layout):
    from deephar_amd import graph, utils, weights
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import spnet
    graph.reset_naming()
    lay = getattr(utils, layout)
    cfg = ModelConfig((128, 128, 3), lay, num_actions=[], num_pyramids=2, action_pyramids=[], downsampling_type='conv')
    m = spnet.build(cfg)
    weights.init_synthetic(m, seed=0)
    rcfg = dict(num_joints=lay.num_joints, dim=lay.dim, num_pyramids=2, num_levels=4, kernel_size=(5, 5), growth=96,
                image_div=8, sam_alpha=1)
    return m, rcfg


@pytest.mark.parametrize('layout', ['pa16j2d', 'pa17j3d'])
def test_pose_spnet_conv_flavour(layout, hip_lib, cuda):
    """128 px, two pyramids, two frames: poses through the conditioned 1e-3 px check of spnet_parity (tests/test_gpu_models.py),
    against the restated forward.  Non-vacuity (1 < logit std < 30) is judged on the fp64 restatement; heads outside the
    range are rescaled here, towards the std of 6 init_synthetic aims for."""
    from deephar_amd import weights
    m, rcfg = _pose_spnet(layout)
    x = np.random.default_rng(11).uniform(-1, 1, (2, 128, 128, 3)).astype(np.float32)
    for attempt in range(4):
        wd = weights.as_dict(m)
        t64 = {}
        o64 = R.spnet_pose_forward(wd, x, rcfg, dtype=torch.float64, taps=t64)
        blocks = [k[:-len('/logits')] for k in t64 if k.endswith('/logits')]
        stds = {b: float(t64[b + '/logits'].std()) for b in blocks}
        print('logit std (pass %d): %s' % (attempt, ' '.join('%s=%.2f' % kv for kv in stds.items())))
        bad = {b + '_heatmaps_conv1': 6.0 / s for b, s in stds.items() if not 2.0 < s < 20.0}
        if not bad:
            break
        weights.rescale_layers(m, bad)
    assert len(blocks) == 6
    for b in blocks:
        assert 1.0 < stds[b] < 30.0, 'heat-map logits of %s are flat or one-hot (std %.2f): vacuous test' % (b, stds[b])
    o32 = R.spnet_pose_forward(wd, x, rcfg, dtype=torch.float32)
    hip = m.predict(x, batch_size=2)
    assert len(hip) == 6 and [h.shape for h in hip] == [o.shape for o in o64]
    dim = rcfg['dim']
    for k, b in enumerate(blocks):
        tol_xy, tol_z, tol_c = paritylog.conditioned_tolerance(t64[b + '/logits'], t64.get(b + '/dlogits'))
        paritylog.check_conditioned('%s.xy' % b, hip[k][..., :2], o32[k][..., :2], o64[k][..., :2], tol_xy)
        if dim == 3:
            paritylog.check_conditioned('%s.z' % b, hip[k][..., 2], o32[k][..., 2], o64[k][..., 2], tol_z)
        paritylog.check_conditioned('%s.conf' % b, hip[k][..., dim], o32[k][..., dim], o64[k][..., dim], tol_c, px=False)


# ---- 11. clip SPNet with actions ---------------------------------------------------------------------------------------------
def test_clip_spnet_with_actions_across_engine_settings_and_through_the_c_plan(hip_lib, cuda, tmp_path):
    from deephar_amd import graph, utils, weights
    from deephar_amd.config import ModelConfig
    from deephar_amd.engine.rules import RuleSet
    from deephar_amd.models import spnet
    graph.reset_naming()
    cfg = ModelConfig((4, 128, 128, 3), utils.pa17j3d, num_actions=[10], num_pyramids=2, action_pyramids=[1, 2],
                      downsampling_type='conv')
    m = spnet.build(cfg)
    weights.init_synthetic(m, seed=0)
    n, T = 2, 4
    # The 1e-3 px bar is the project's bar for read-outs conditioned like a trained network's (tests/wellcond.py: S <= 0.05):
    # on per-pixel noise with un-fitted heads two fp32 evaluations that only ORDER their sums differently -- the CPU
    # restatement against itself in fp64 included, see test_pose_spnet_conv_flavour's records -- are 1 .. 1.5e-3 px apart.
    # So: one smooth video cut into the clips, heads fitted to one peak per joint, conditioning asserted on the fp64
    # restatement of the pose stream (which the action stream does not feed back into).
    x = wellcond.video_cuts(n, T, 128, 13)
    rcfg = dict(num_joints=17, dim=3, num_pyramids=2, num_levels=4, kernel_size=(5, 5), growth=96, image_div=8, sam_alpha=1)
    frames = x.reshape((n * T,) + x.shape[2:])
    R.fit_pose_heads(m, rcfg, frames, wellcond.scene_positions(n, T, 17, 13))
    t64 = {}
    p64 = R.spnet_pose_forward(weights.as_dict(m), frames, rcfg, dtype=torch.float64, taps=t64)
    stats = wellcond.assert_well_conditioned(t64, 'conv flavour')
    print('conditioning:', {b: round(s['S_max'], 3) for b, s in stats.items()})
    npose = spnet.get_num_predictions(2, 4)

    def run(**opts):
        for k, v in opts.items():
            setattr(m, k, v)
        m.executor.autotune = False              # (every tiling gives the same bits; keeps the test to seconds)
        return m.predict(x, batch_size=n)

    base = run(rules=RuleSet())
    assert len(base) == 2 * npose and all(np.all(np.isfinite(o)) for o in base)
    for a in base[npose:]:
        assert a.shape == (n, 10) and np.allclose(a.sum(-1), 1.0, atol=1e-5)
    for k in range(npose):                       # (reported: the engine against the fp64 restatement of the pose stream)
        print('pose %d: |hip - o64| = %.3e px' % (k, 256 * np.abs(base[k].reshape(p64[k].shape)[..., :3] - p64[k][..., :3]).max()))
    kinds = [s.kind for s in m.plan.steps]
    assert kinds.count('convtranspose') == 3 and 'upsample_add' not in [s.kind for s in m.plan.steps if s.name and '_uu' in s.name]

    # the C-level executor replays the same launches: bit-identical at the same batch size
    path = str(tmp_path / 'conv_flavour.dhplan')
    m.export_plan(path, n)
    blob = open(path, 'rb').read()
    assert blob[:4] == b'DHPL' and int.from_bytes(blob[4:8], 'little') == 3        # the new step records: blob version 3
    plan = C.c_void_p()
    assert hip_lib.dh_plan_create(blob, len(blob), C.byref(plan)) == 0
    try:
        xd = torch.from_numpy(x).to(cuda)
        outs = [torch.full(r.shape, float('nan'), device=cuda) for r in base]
        ins_p = (C.c_void_p * 1)(xd.data_ptr())
        outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        assert hip_lib.dh_forward(plan, ins_p, n, outs_p, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        for o, r in zip(outs, base):
            assert np.array_equal(o.cpu().numpy(), r)
    finally:
        assert hip_lib.dh_plan_destroy(plan) == 0

    for name, opts in (('two streams, tail', dict(num_streams=2, stream_policy='tail')),
                       ('all rules off', dict(num_streams=1, stream_policy='list', rules=_all_off()))):
        other = run(**opts)
        for k in range(npose):
            d = np.abs(other[k] - base[k]).max()
            print('%s: pose %d differs by %.3e px' % (name, k, 256 * d))
            assert d <= PX_TOL, (name, k, d)
        for k in range(npose, 2 * npose):
            assert np.array_equal(other[k].argmax(-1), base[k].argmax(-1)), (name, k)
            assert np.allclose(other[k], base[k], atol=1e-5), (name, k)
