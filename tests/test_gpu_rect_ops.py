"""Op-level tests on maps with H != W.

Every other soft-argmax test of the suite runs on square maps, where an exchange of H and W in the kernels' index arithmetic
(two grids gx[W] / gy[H], r = px / W, the LDS layout sgy = sgx + W, the 2 x 2 window guard, the grid copy loops) changes
nothing.  Here every read-out runs on rectangular maps in both orientations, against

  * tests/rectref.py -- an fp64 NumPy statement from the definition, independent of oracle/ops.py -- and oracle/ops.py,
    under the assertions and bars of tests/test_gpu_ops.py::test_softargmax2d;
  * itself on the transposed maps (x and y change places, nothing else moves);
  * known answers on 5 x 9 and 9 x 5 maps.

tests/test_rect_host.py shows on the same inputs that a read-out with H and W exchanged is >= 100 bars away.  The fused
up-sampling epilogue, dh_upsample2x_add_f32 and the first-layer kernel run through the bodies of their square tests.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectref as R                                # noqa: E402
import slabview as SV                              # noqa: E402
import test_gpu_ops as OPS                         # noqa: E402
import test_gpu_slab_ops as SLAB                   # noqa: E402
from oracle import ops as O                        # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 3.9e-6          # 1e-3 px of a 256-px crop in normalised units
DH_EUNSUPPORTED = -2
_ids = lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s)


def _close(got, ref, atol, rtol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    tol = atol + rtol * np.abs(ref)
    print('%s: max err %.3e' % (what, err.max()))
    assert np.all(err <= tol), '%s: max err %.3e (tol %.3e) at %s' % (
        what, err.max(), tol.flat[err.argmax()], np.unravel_index(err.argmax(), err.shape))


# ------------------------------------------------------------------------------------------------------------------------
# dh_softargmax2d_f32
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _sam_ref(shape, alpha):
    """The three references of one (shape, alpha): rectref (fp64), the CPU oracle in fp32 and in fp64.  Read only."""
    h = R.sam_input(shape)
    t = torch.from_numpy(h)
    p, p64 = O.channel_softmax_2d(t, alpha), O.channel_softmax_2d(t.double(), alpha)
    return dict(h=h, rect=R.softargmax(h, alpha, R.SAM_CONF_SCALE),
                prob=p.numpy(), xy=O.softargmax2d_from_prob(p).numpy(), xy64=O.softargmax2d_from_prob(p64).numpy(),
                conf_raw=O.joints_probability(R.SAM_CONF_SCALE * t).numpy(), conf_prob=O.joints_probability(p).numpy(),
                gmax=torch.amax(t, dim=(1, 2)).numpy())


def _sam_run(h, alpha, cuda):
    from deephar_amd import functional as F
    out = F.softargmax2d(torch.from_numpy(np.ascontiguousarray(h)).to(cuda), alpha=alpha, conf_scale=R.SAM_CONF_SCALE,
                         want_prob=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('alpha', R.SAM_ALPHAS)
@pytest.mark.parametrize('shape', sorted(R.SAM_SHAPES), ids=_ids)
def test_softargmax2d_on_rectangular_maps(shape, alpha, hip_lib, cuda):
    """All four instantiations of softargmax2d_kernel (the library says which: asserted) and the grid copy
    loops beyond the 256 threads, on H != W: the assertions and bars of test_gpu_ops.test_softargmax2d against oracle/ops.py,
    and the same bars against rectref's fp64 values."""
    assert SV.sam_variant(hip_lib, *shape) == R.SAM_SHAPES[shape]
    r = _sam_ref(shape, alpha)
    out = _sam_run(r['h'], alpha, cuda)
    what = 'softargmax2d %s alpha %g' % (shape, alpha)
    e64 = np.abs(out['xy'].astype(np.float64) - r['xy64']).max()
    e_rect = np.abs(out['xy'].astype(np.float64) - r['rect']['xy']).max()
    e_cpu = np.abs(r['xy'].astype(np.float64) - r['xy64']).max()
    print('%s: xy |hip - fp64 oracle| %.3e  |hip - rectref| %.3e  |fp32 oracle - fp64 oracle| %.3e' % (what, e64, e_rect, e_cpu))
    assert e64 <= BAR / 2 and e_rect <= BAR / 2, (what, e64, e_rect)
    assert np.abs(out['xy'] - r['xy']).max() <= BAR, what
    _close(out['prob'], r['prob'], 1e-9, 1e-5, what + ' prob')
    _close(out['prob'], r['rect']['prob'], 1e-9, 1e-5, what + ' prob vs rectref')
    _close(out['conf_raw'], r['conf_raw'], 1e-5, OPS.RTOL, what + ' conf_raw')
    _close(out['conf_raw'], r['rect']['conf_raw'], 1e-5, OPS.RTOL, what + ' conf_raw vs rectref')
    _close(out['conf_prob'], r['conf_prob'], 1e-9, 1e-5, what + ' conf_prob')
    _close(out['conf_prob'], r['rect']['conf_prob'], 1e-9, 1e-5, what + ' conf_prob vs rectref')
    assert SV.same_bits(out['gmax'], r['gmax']) and np.array_equal(out['gmax'].astype(np.float64), r['rect']['gmax']), what


@pytest.mark.parametrize('shape', sorted(R.SAM_SHAPES), ids=_ids)
def test_softargmax2d_of_the_transposed_maps(shape, hip_lib, cuda):
    """softargmax(h^T) = softargmax(h) with x and y exchanged: coordinates within 3.9e-6 (each side is within half of that of
    the truth), the global maximum bit for bit, the confidences within the atol of test_softargmax2d (the 2 x 2 windows are
    the same sets of pixels, summed in another order)."""
    h = R.sam_input(shape)
    a = _sam_run(h, 1.0, cuda)
    b = _sam_run(np.swapaxes(h, 1, 2), 1.0, cuda)
    assert SV.sam_variant(hip_lib, shape[0], shape[2], shape[1], shape[3]) == R.SAM_SHAPES[shape]        # (same instantiation)
    d = np.abs(a['xy'][..., ::-1] - b['xy']).max()
    print('transposed %s: xy %.3e' % (shape, d))
    assert d <= BAR
    assert SV.same_bits(a['gmax'], b['gmax'])
    _close(b['conf_raw'], a['conf_raw'], 1e-5, OPS.RTOL, 'conf_raw of the transposed maps')
    _close(b['conf_prob'], a['conf_prob'], 1e-9, 1e-5, 'conf_prob of the transposed maps')
    _close(np.swapaxes(b['prob'], 1, 2), a['prob'], 1e-9, 1e-5, 'prob of the transposed maps')


@functools.lru_cache(maxsize=None)
def _view_case():
    """tests/test_gpu_slab_ops._sam_case for the rectangular view shape, plus rectref's values"""
    r = SLAB._sam_case(R.SAM_VIEW)
    rect = R.softargmax(r['h'], 1.0, 4.0)
    assert np.abs(rect['xy'] - r['xy64']).max() <= 2.0 ** -25       # (the oracle's grids are float32, rectref's exact)
    return r, rect


def test_softargmax2d_on_a_rectangular_view(hip_lib, cuda):
    """12 x 20 maps of 17 channels inside channel slabs: the odd layout (offset 1: scalar staging with its clamped tail) and
    the aligned one (offset 4, pitch 28: float4 staging), xy into [F, J, 3], confidences into the second column of [F, J, 2],
    the probability maps into a 36-channel slab -- the checks of test_gpu_slab_ops.test_softargmax2d_on_views, nothing
    written outside the views, the same bits in every layout."""
    r, rect = _view_case()
    got = {}
    for name in SV.LAYOUTS:
        ld, off = SV.layout(17, name)
        assert name == 'dense' or (ld > 17 and off == (1 if name == 'odd' else 4))
        got[name] = SLAB._sam_launch(hip_lib, cuda, r['h'], ld, off, ldxy=3, ldcr=2, ldcp=2, ldp=36, offp=2)
        SLAB._sam_check(got[name], r, 'softargmax2d 12x20 view ' + name)
        assert np.abs(got[name]['xy'].astype(np.float64) - rect['xy']).max() <= BAR / 2
        _close(got[name]['conf_raw'], rect['conf_raw'], 1e-5, OPS.RTOL, 'conf_raw vs rectref ' + name)
    for k in SLAB.SAM_OUTPUTS:
        SLAB._all_same_bits({n: g[k] for n, g in got.items()}, 'softargmax2d 12x20 ' + k)


def test_softargmax2d_xy_times_conf_on_rectangular_maps(hip_lib, cuda):
    """dh_sam_args.xy_times_conf on 12 x 20 maps at offset 1 of a slab: against rectref's fp64 xy * conf_prob, and bit for
    bit the fp32 product of the xy and conf_prob the launch returns with the flag off."""
    r, rect = _view_case()
    ref64 = rect['xy'] * rect['conf_prob']
    ld, off = SV.layout(17, 'odd')
    plain = SLAB._sam_launch(hip_lib, cuda, r['h'], ld, off, want=('xy', 'conf_prob'), ldxy=3, ldcp=2)
    want = plain['xy'] * plain['conf_prob']
    assert want.dtype == np.float32
    for outputs in (('xy', 'conf_prob'), ('xy',)):
        on = SLAB._sam_launch(hip_lib, cuda, r['h'], ld, off, want=outputs, ldxy=3, ldcp=2, flag=1)
        e = np.abs(on['xy'].astype(np.float64) - ref64).max()
        print('xy_times_conf %s: vs fp64 %.3e' % (outputs, e))
        assert e <= BAR, (outputs, e)
        assert SV.same_bits(on['xy'], want), outputs


@pytest.mark.parametrize('H,W', [(5, 9), (9, 5)])
def test_softargmax2d_known_answers_on_rectangular_maps(H, W, hip_lib, cuda):
    from deephar_amd import functional as F
    run = lambda h, **kw: {k: v.cpu().numpy() for k, v in F.softargmax2d(torch.from_numpy(h).to(cuda), **kw).items()
                           if v is not None}
    # one peak of 30 on -1e4: the four corners and one interior pixel
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 2, 2)]
    h = np.full((1, H, W, len(pts)), -1e4, np.float32)
    for c, (r, q) in enumerate(pts):
        h[0, r, q, c] = 30.0
    xy = run(h)['xy'][0]
    for c, (r, q) in enumerate(pts):
        np.testing.assert_allclose(xy[c], [np.float32(q / (W - 1)), np.float32(r / (H - 1))], atol=1e-7, err_msg=str((r, q)))
    # a 2 x 2 block of ones in each of the four corner windows: conf_raw == 4 conf_scale exactly
    wins = [(0, 0), (0, W - 2), (H - 2, 0), (H - 2, W - 2)]
    h = np.zeros((1, H, W, len(wins)), np.float32)
    for c, (r, q) in enumerate(wins):
        h[0, r:r + 2, q:q + 2, c] = 1.0
    for scale in (1.0, 3.0):
        assert np.array_equal(run(h, conf_scale=scale)['conf_raw'][0, :, 0], np.full(len(wins), 4.0 * scale, np.float32))
    # a single one at (H-1, 0) and at (0, W-1): the only window that holds it sums to 1 -- a window that wrapped round the
    # row's end (guard with H and W exchanged) would not exist or would hold the wrong pixels
    ones = [(H - 1, 0), (0, W - 1)]
    h = np.zeros((1, H, W, len(ones)), np.float32)
    for c, (r, q) in enumerate(ones):
        h[0, r, q, c] = 1.0
    for scale in (1.0, 3.0):
        assert np.array_equal(run(h, conf_scale=scale)['conf_raw'][0, :, 0], np.full(len(ones), scale, np.float32))
    # a constant map
    np.testing.assert_allclose(run(np.full((2, H, W, 5), 0.25, np.float32))['xy'], 0.5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------------
# dh_softargmax2d_context_f32
# ------------------------------------------------------------------------------------------------------------------------
CTX_CASES = [((3, 24, 32, 48), 16, 2), ((3, 32, 24, 48), 16, 2),
             ((2, 12, 16, 52), 12, 3), ((2, 16, 12, 52), 12, 3),       # a view: 48 of 52 channels
             ((1, 6, 8, 64), 16, 2),
             ((1, 40, 48, 48), 16, 2),                                 # the largest map of the model sweep that fits: 123 232 B
             ((1, 45, 45, 48), 16, 2)]                                 # odd extents next to the limit: 129 960 B of 131 072


@pytest.mark.parametrize('shape,joints,nctx', CTX_CASES, ids=_ids)
def test_softargmax2d_context_on_rectangular_maps(shape, joints, nctx, hip_lib, cuda):
    """The assertions of test_gpu_ops.test_softargmax2d_with_context_in_one_launch on H != W: the fp64 aggregation (rectref,
    and oracle/ops.py) within 3.9e-6, the three-launch path within 2e-6, the joint confidences bit for bit those of the
    plain kernel."""
    from deephar_amd import functional as F
    f, hh, ww, ld = shape
    assert SV.sam_ctx_rc(hip_lib, hh, ww, joints, nctx, f) == 0
    rng = np.random.default_rng(sum(shape) + nctx)
    h = OPS._rand(rng, shape, 4.0) + 1.0                     # (positive offset: context confidences away from 0)
    t = torch.from_numpy(h)
    c = joints * (1 + nctx)
    pose, conf = F.softargmax2d_context(t.to(cuda), joints, nctx, 0.8, conf_scale=1.0)
    rs, rc = R.softargmax(h[..., :joints]), R.softargmax(h[..., joints:c])
    assert float(rc['conf_raw'].reshape(f, joints, nctx).sum(-1).min()) > 1.0
    ref = R.context_aggregation(rs['xy'], rc['xy'], rc['conf_raw'], joints, nctx, 0.8)
    hs, hc = t[..., :joints].double(), t[..., joints:c].double()
    pc = O.joints_probability(hc)
    ref_o = O.context_aggregation(O.softargmax2d_from_prob(O.channel_softmax_2d(hs, 1.0)),
                                  O.softargmax2d_from_prob(O.channel_softmax_2d(hc, 1.0)), pc, joints, nctx, 0.8).numpy()
    e, e_o = np.abs(pose.cpu().numpy().astype(np.float64) - ref).max(), np.abs(pose.cpu().numpy().astype(np.float64) - ref_o).max()
    print('context %s: |hip - rectref| %.3e  |hip - fp64 oracle| %.3e' % (shape, e, e_o))
    assert e <= BAR and e_o <= BAR
    _close(conf.cpu().numpy(), O.joints_probability(hs).numpy(), 1e-5, OPS.RTOL, 'joint confidence')
    _close(conf.cpu().numpy(), rs['conf_raw'], 1e-5, OPS.RTOL, 'joint confidence vs rectref')
    d = t.to(cuda)
    a = F.softargmax2d(d[..., :joints].contiguous())
    b = F.softargmax2d(d[..., joints:c].contiguous())
    three = F.context_aggregation(a['xy'], b['xy'], b['conf_raw'], nctx, 0.8)
    assert float((three - pose).abs().max()) <= 2e-6 and torch.equal(a['conf_raw'], conf)


@pytest.mark.parametrize('shape', [(1, 48, 48, 48), (1, 40, 52, 48)], ids=_ids)
def test_softargmax2d_context_refuses_maps_beyond_its_lds_slab(shape, hip_lib, cuda):
    """147 840 B and 133 488 B of LDS > 128 KiB: rc = -2 (DH_EUNSUPPORTED), and the launcher returns before launching
    anything -- the outputs keep their canaries.  (The planner keeps such maps on two soft-argmax launches and one
    aggregation: tests/test_rect_host.py.)"""
    f, hh, ww, ch = shape
    j, nctx = 16, 2
    assert SV.sam_ctx_rc(hip_lib, hh, ww, j, nctx, f) == DH_EUNSUPPORTED
    x = SLAB._In(np.ones(shape, np.float32), ch, 0)
    y, conf = SLAB._Out((f, j, 2), 2, 0), SLAB._Out((f, j, 1), 1, 0)
    gx = SLAB._dev(np.linspace(0.0, 1.0, num=ww).astype(np.float32), cuda)
    gy = SLAB._dev(np.linspace(0.0, 1.0, num=hh).astype(np.float32), cuda)
    a = SLAB._lib().SamArgs()
    a.h, a.gx, a.gy, a.conf_raw = x.ptr, gx.data_ptr(), gy.data_ptr(), conf.ptr
    a.F, a.H, a.W, a.C, a.ldh, a.ldcr = f, hh, ww, ch, ch, 1
    a.alpha, a.conf_scale = 1.0, 1.0
    rc = hip_lib.dh_softargmax2d_context_f32(C.byref(a), j, nctx, 0.8, y.ptr, 2, SLAB._stream())
    torch.cuda.synchronize()
    assert rc == DH_EUNSUPPORTED, rc
    assert np.all(y.get('refused pose') == SV.CANARY) and np.all(conf.get('refused confidence') == SV.CANARY)


# ------------------------------------------------------------------------------------------------------------------------
# fused up-sampling epilogue, dh_upsample2x_add_f32, first-layer kernel: the bodies of the square tests
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cout,cfg', [(288, -1), (96, 5), (576, 11)])
@pytest.mark.parametrize('shape', [(2, 6, 10, 288), (2, 10, 6, 288)], ids=_ids)
def test_conv2d_fused_upsample_add_on_rectangular_maps(shape, cout, cfg, hip_lib, cuda):
    """conv -> BN -> +res1 -> UpSampling2D -> +res2 in the epilogue of the autotuned (-1), a general (5) and an LDS-DMA (11)
    tiling: 6 x 10 -> 12 x 20 and 10 x 6 -> 20 x 12, the output row pitch 2 W differs from 2 H."""
    OPS.test_conv2d_fused_upsample_add(cout, cfg, hip_lib, cuda, shape=shape)


@pytest.mark.parametrize('shape', [(2, 16, 20, 64), (2, 20, 16, 64)], ids=_ids)
def test_conv2d_fused_prologue_epilogue_on_rectangular_maps(shape, hip_lib, cuda):
    """(more than 256 positions: the map stays on the kernel the 16 x 16 test reaches, not the skinny-conv one)"""
    OPS.test_conv2d_fused_prologue_epilogue(hip_lib, cuda, shape=shape)


@pytest.mark.parametrize('case', [(2, 12, 20, 288, 576, 1, 1, False, True, True), (2, 20, 12, 288, 576, 1, 1, False, True, True)],
                         ids=_ids)
def test_conv2d_up2_split_and_dma_tilings_on_rectangular_maps(case, hip_lib, cuda):
    """The `up2` row of SPLIT_CASES at 12 x 20 (and 20 x 12): split-bf16 as close to fp64 as the fp32 path and every split
    tiling bit-identical; every fp32 LDS-DMA tiling bit-identical to the general kernel."""
    OPS.test_conv2d_split_bf16(case, hip_lib, cuda)
    OPS.test_conv2d_dma_gemm_tilings_bitwise(case, hip_lib, cuda)


@pytest.mark.parametrize('shape', [(2, 6, 10, 288), (2, 10, 6, 20)], ids=_ids)
def test_upsample_add_bit_exact_on_rectangular_maps(shape, hip_lib, cuda):
    OPS.test_upsample_add_bit_exact(hip_lib, cuda, shape=shape)


@pytest.mark.parametrize('ks,cout,bn', [(3, 32, True), (7, 64, False)])
@pytest.mark.parametrize('frame', [(192, 256), (256, 192)], ids=_ids)
def test_first_layer_on_rectangular_frames(frame, ks, cout, bn, hip_lib, cuda):
    """192 x 256 frames give 96 x 128 maps: the first-layer kernel takes the layer (dh_conv2d_uses_first_layer_kernel == 1);
    256 x 192 frames give 96 output columns: rule == 0, the general kernel.  Both against the fp32 / fp64 oracle, uint8 frames
    bit for bit the normalised float frames, batch-size invariant (the body of test_first_layer_kernel)."""
    OPS.test_first_layer_kernel(ks, cout, bn, hip_lib, cuda, frame=frame)
