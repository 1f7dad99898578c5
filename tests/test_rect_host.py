"""Host tests (no GPU) that go with tests/test_gpu_rect_ops.py and tests/test_gpu_rect_models.py: non-square and larger maps.

  * planner rule R5b against the fused read-out's LDS limit (launch_softargmax2d_context refuses a slab above 128 KiB; the
    planner restates the limit and must keep the two read-outs and the aggregation apart beyond it);
  * every plan the GPU model tests run binds under binding.FakeEnv with H and W in their places;
  * the random inputs of the op-level tests tell a read-out with H and W exchanged from the right one by far more than
    the bars (tests/rectref.py, swapped=True).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectref as R                                # noqa: E402
import slabview as SV                              # noqa: E402

from deephar_amd import _lib                       # noqa: E402

BAR = 3.9e-6          # 1e-3 px of a 256-px crop in normalised units

# (input rows, input columns) of the whole-model cases of tests/test_gpu_rect_models.py
RECT_FRAMES = ((192, 256), (256, 192))
LARGE_FRAMES = ((384, 384), (320, 416))
SPNET_FRAMES = ((128, 192), (192, 128))


def context_model(rows, cols, blocks=1, **kw):
    """ReceptionNet 2-D with context (J = 16, two contexts per joint) on rows x cols frames"""
    from test_gpu_models import _build
    return _build(2, blocks, 16, input_shape=(rows, cols, 3), num_context_per_joint=2, concat_pose_confidence=False, **kw)[0]


def decoder_only(H, W, J=16, nctx=2):
    """A 1x1 convolution to J (1 + nctx) heat maps on an H x W map and reception.pose_regression_2d_context on them: the
    decoder of the ReceptionNet at a map size its hourglass (two 2 x 2 poolings: multiples of four) cannot be built at."""
    from deephar_amd import graph as G, layers as L
    from deephar_amd.model import Model
    from deephar_amd.models import blocks, reception
    G.reset_naming()
    inp = L.Input((H, W, 8))
    h = L.act_conv(inp, J * (1 + nctx), (1, 1))
    sam_s = blocks.build_softargmax_2d((H, W, J), rho=0, name='sSAM')
    prob_s = blocks.build_joints_probability((H, W, J), name='sjProb')
    sam_c = blocks.build_softargmax_2d((H, W, J * nctx), rho=0, name='cSAM')
    prob_c = blocks.build_joints_probability((H, W, J * nctx), name='cjProb')
    agg = blocks.build_context_aggregation(J, nctx, 0.8, name='Agg')
    pose, visible, _ = reception._decode_2d_context(h, J, sam_s, sam_c, prob_c, agg, prob_s)
    return Model(inputs=inp, outputs=[pose, visible])


def readout(plan):
    return [s.kind for s in plan.steps if s.kind in ('sam', 'sam_ctx', 'context_agg')]


# ---- 1. rule R5b ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols,fused', [(320, 384, True), (288, 448, True),
                                             (320, 416, False), (352, 384, False), (384, 384, False)])
def test_fused_decoder_is_planned_only_inside_its_lds_limit(rows, cols, fused, hip_lib):
    """1-block ReceptionNet 2-D with context.  40 x 48 and 36 x 56 maps (the largest the hourglass can be built at that fit:
    129 392 B) plan `sam_ctx`; 40 x 52, 44 x 48 and 48 x 48 maps (133 488, 135 536 and 147 840 B > 131 072) keep two `sam`
    steps and one `context_agg` -- before the planner knew the limit it planned `sam_ctx` there and Model.predict raised in
    the middle of the launch sequence."""
    H, W = rows // 8, cols // 8
    assert (SV.sam_ctx_rc(hip_lib, H, W) == 0) == fused                        # the case is on the side it is meant for
    plan = context_model(rows, cols).plan
    assert all(s.ins['h'].shape[-3:-1] == (H, W) for s in plan.steps if s.kind in ('sam', 'sam_ctx'))
    assert readout(plan) == (['sam_ctx'] if fused else ['sam', 'sam', 'context_agg']), (H, W, readout(plan))


@pytest.mark.parametrize('H,W,fused', [(45, 45, True), (45, 46, False), (32, 32, True), (3, 300, True), (300, 7, False)])
def test_fused_decoder_limit_on_the_decoder_alone(H, W, fused, hip_lib):
    """The same rule at the map sizes next to the limit, odd ones included (a 360 x 360 crop gives 45 x 45 maps: 129 960 B,
    inside; 45 x 46: 132 844 B, outside), on the decoder behind a 1x1 convolution -- reception.build cannot be built there."""
    with pytest.raises(ValueError):
        context_model(8 * 45, 8 * 45)                      # (why this test has a graph of its own)
    assert (SV.sam_ctx_rc(hip_lib, H, W) == 0) == fused
    assert readout(decoder_only(H, W).plan) == (['sam_ctx'] if fused else ['sam', 'sam', 'context_agg'])


# ---- 2. binding of the plans of tests/test_gpu_rect_models.py --------------------------------------------------------------------
def rect_plans():
    """(name, (input rows, input columns), builder of the model) of every whole-model case"""
    from test_gpu_models import _build, _spnet
    out = []
    for r, c in RECT_FRAMES:
        out.append(('rec2d_%dx%d' % (r, c), (r, c), lambda r=r, c=c: context_model(r, c, blocks=2)))
        out.append(('rec3d_%dx%d' % (r, c), (r, c), lambda r=r, c=c: _build(3, 2, 17, input_shape=(r, c, 3), depth_maps=16)[0]))
    for r, c in LARGE_FRAMES:
        out.append(('rec2d_large_%dx%d' % (r, c), (r, c), lambda r=r, c=c: context_model(r, c)))
    for r, c in SPNET_FRAMES:
        out.append(('spnet_%dx%d' % (r, c), (r, c),
                    lambda r=r, c=c: _spnet(4, 'pa16j2d', 15, 2, [1, 2], 160, replica=True, input_shape=(4, r, c, 3))[0]))
    return out


@pytest.mark.parametrize('name,frame,make', rect_plans(), ids=[p[0] for p in rect_plans()])
def test_rect_plans_bind_with_rows_and_columns_in_place(name, frame, make, hip_lib):
    """Every step binds (FakeEnv); a SamArgs carries (H, W) of its maps in that order -- and the maps have the frame's aspect,
    rows : columns, stated here from the input shape alone --; every conv / depthwise / pooling struct carries (H, W) and
    (OH, OW) of the tensors it reads and writes."""
    from test_binding_host import launches
    rows, cols = frame
    plan = make().plan
    calls, _ = launches(plan, 2)
    assert len(calls) == len(plan.steps) > 0
    seen = set()
    for s, entry, structs, scalars in calls:
        assert hasattr(hip_lib, entry), (s.kind, entry)
        seen.add(s.kind)
        if s.kind in ('sam', 'sam_ctx'):
            a, h = structs[0], s.ins['h']
            assert isinstance(a, _lib.SamArgs) and (a.H, a.W) == h.shape[-3:-1], (s.name, a.H, a.W, h.shape)
            assert a.H * cols == a.W * rows and rows % a.H == 0, (s.name, a.H, a.W)       # rows / H == cols / W: a power of two
            assert a.C == h.C and a.ldh == h.ld and a.F == 2 * h.lead(3)
        elif s.kind == 'conv':
            a, x, y, at = structs[0], s.ins['x'], s.outs['y'], s.attrs
            H, W = x.shape[-3], x.shape[-2]
            if at.get('seg') is not None:
                H, W = H // at['seg']['pool_sh'], W // 2
            if at.get('x_resample', 0):
                H, W = (2 * H, 2 * W) if at['x_resample'] == 1 else (H // 2, W // 2)
            up = 2 if at['up2'] else 1
            assert (a.H, a.W, a.OH, a.OW) == (H, W, y.shape[-3] // up, y.shape[-2] // up), (s.name, a.H, a.W, a.OH, a.OW)
            # TF 'same' / 'valid' output extents from the struct's own fields, rows with rows and columns with columns
            assert a.OH == (a.H + a.SH - 1) // a.SH or a.OH == (a.H - a.KH) // a.SH + 1, (s.name, a.H, a.OH)
            assert a.OW == (a.W + a.SW - 1) // a.SW or a.OW == (a.W - a.KW) // a.SW + 1, (s.name, a.W, a.OW)
            if s.outs.get('ypool') is not None:
                assert s.outs['ypool'].shape[-3:-1] == (a.OH // 2, a.OW // 2)
        elif s.kind == 'dwconv':
            a, x, y = structs[0], s.ins['x'], s.outs['y']
            if isinstance(a, _lib.DwsArgs):
                assert (a.H, a.W, a.OH, a.OW) == x.shape[-3:-1] + y.shape[-3:-1], s.name
            else:
                assert (a.H, a.W) == y.shape[-3:-1], s.name
                assert x.shape[-3:-1] == ((a.H // 2, a.W // 2) if a.up_in else (a.H, a.W)), s.name
        elif s.kind == 'pool':
            a, x, y = structs[0], s.ins['x'], s.outs['y']
            assert (a.H, a.W, a.OH, a.OW) == x.shape[-3:-1] + y.shape[-3:-1], s.name
            assert a.OH == (a.H + a.SH - 1) // a.SH and a.OW == (a.W + a.SW - 1) // a.SW, s.name
    assert {'conv', 'dwconv', 'pool'} <= seen and seen & {'sam', 'sam_ctx'}
    # the first convolution reads the frame itself
    first = calls[0]
    assert first[0].kind == 'conv' and (first[2][0].H, first[2][0].W) == (rows, cols)


def test_the_two_orientations_are_different_plans():
    """A landscape and a portrait crop go down different kernels: 24 x 32 maps have the 2x2 pooling in the epilogue of the
    convolution in front of it (planner rule R7 keys on W == 32, or W in (8, 16) with H W % 32 == 0), 32 x 24 maps pool in
    launches of their own; SPNet at 128 x 192 pools in 5 launches, at 192 x 128 in 3."""
    counts = {}
    for r, c in RECT_FRAMES:
        plan = context_model(r, c, blocks=2).plan
        counts[(r, c)] = (sum(1 for s in plan.steps if s.outs.get('ypool') is not None),
                          sum(1 for s in plan.steps if s.kind == 'pool'))
        assert readout(plan) == ['sam_ctx', 'sam_ctx']
    assert counts[(192, 256)] == (4, 2) and counts[(256, 192)] == (0, 6), counts
    from test_gpu_models import _spnet
    pools = [sum(1 for s in _spnet(4, 'pa16j2d', 15, 2, [1, 2], 160, replica=True, input_shape=(4, r, c, 3))[0].plan.steps
                 if s.kind == 'pool') for r, c in SPNET_FRAMES]
    assert pools == [5, 3], pools


# ---- 3. the op-level inputs can tell H from W ----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', sorted(R.SAM_SHAPES), ids=lambda s: 'x'.join(map(str, s)))
def test_sam_shapes_reach_their_instantiation_and_tell_rows_from_columns(shape, hip_lib):
    """Each shape of the GPU test reaches the instantiation it is there for (slabview.sam_variant: the library's answer), and on
    its random input a read-out with the roles of H and W exchanged (rectref.softargmax(swapped=True): x normalised by H - 1,
    r = px / H, the window guard with H and W exchanged) is at least 100 x the bar away from the right one, on the
    coordinates and the raw confidence at either alpha and on the soft-max confidence at alpha 1: an exchange in the kernel cannot hide inside the tolerance."""
    assert SV.sam_variant(hip_lib, *shape) == R.SAM_SHAPES[shape]
    assert shape[1] != shape[2]
    h = R.sam_input(shape)
    prob_tells = []
    for alpha in R.SAM_ALPHAS:
        good = R.softargmax(h, alpha, R.SAM_CONF_SCALE)
        bad = R.softargmax(h, alpha, R.SAM_CONF_SCALE, swapped=True)
        dxy = np.abs(good['xy'] - bad['xy']).max()
        dcr = np.abs(good['conf_raw'] - bad['conf_raw'])
        dcp = np.abs(good['conf_prob'] - bad['conf_prob'])
        print(shape, alpha, 'xy %.3e conf_raw %.3e conf_prob %.3e' % (dxy, dcr.max(), (dcp / good['conf_prob']).max()))
        assert dxy >= 100 * BAR
        assert np.any(dcr >= 100 * (1e-5 + 2e-5 * np.abs(good['conf_raw'])))          # (test_softargmax2d: atol 1e-5, rtol 2e-5)
        prob_tells.append(bool(np.any(dcp >= 100 * (1e-9 + 1e-5 * np.abs(good['conf_prob'])))))      # (atol 1e-9, rtol 1e-5)
        # what the exchange cannot move stays put: the check is about the index arithmetic alone
        assert np.array_equal(good['gmax'], bad['gmax']) and np.array_equal(good['prob'], bad['prob'])
    # (at alpha 2.5 the probability maps of the larger shapes are nearly one-hot: whatever window holds the peak sums to almost
    #  the same, exchanged or not -- the window arithmetic of the second pass is told apart at alpha 1)
    assert prob_tells[R.SAM_ALPHAS.index(1.0)], prob_tells


def test_rectref_on_square_maps_is_its_own_swap_and_agrees_with_the_oracle():
    """rectref against oracle/ops.py in fp64 on a 7 x 11 map (1e-12; coordinates 2**-25), and swapped=True on a square map is the identity."""
    import torch
    from oracle import ops as O
    h = R.sam_input((2, 7, 11, 5))
    t = torch.from_numpy(h).double()
    got = R.softargmax(h, 2.5, 4.0)
    p = O.channel_softmax_2d(t, 2.5)
    assert np.abs(got['prob'] - p.numpy()).max() <= 1e-12
    # (the oracle's grids are the reference's float32 weights, rectref's are exact: half a float32 ulp of a value <= 1)
    assert np.abs(got['xy'] - O.softargmax2d_from_prob(p).numpy()).max() <= 2.0 ** -25
    assert np.abs(got['conf_raw'] - O.joints_probability(4.0 * t).numpy()).max() <= 1e-12
    assert np.abs(got['conf_prob'] - O.joints_probability(p).numpy()).max() <= 1e-12
    sq = R.sam_input((2, 9, 9, 3))
    a, b = R.softargmax(sq, 1.0, 4.0), R.softargmax(sq, 1.0, 4.0, swapped=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)
