"""CPU references and launch helpers for the extended split-bf16 scope (Model.gemm_scope = 'extended', dh_conv_args.w_split =
5 / 6 / 7, csrc/gemm1x1s_ext.hip).  TEST INFRASTRUCTURE: nothing here is used by the package.

The contract is the one of tests/bf16_modes_ref.py.  What the extended scope adds to the layers of a mode:
  * K x K convolutions with Cin % 16 == 0 (the standard scope: Cin % 32 == 0) -- `emulate` below;
  * pointwise convolutions with a BatchNormalization prologue.  The oracle applies BN and ReLU before it calls conv2d, so the
    operand that is split is the post-prologue one, and bf16_modes_ref.emulate evaluates every pointwise convolution as E_P
    already: nothing to add for them."""
import ctypes as C

import numpy as np
import torch

import bf16_modes_ref as R

CODES = {'bf16x3': 1, 'bf16x2': 3, 'bf16': 4}
WIDE_CODES = {'bf16x3': 5, 'bf16x2': 6, 'bf16': 7}


def emulate(monkeypatch, parts):
    """bf16_modes_ref.emulate with the extended scope's K x K rule: oracle.ops.conv2d evaluates every pointwise convolution
    and every K x K convolution with Cin % 16 == 0 as E_P for the rest of the test."""
    from oracle import ops
    orig = ops.conv2d

    def conv2d(x, kernel, strides=(1, 1), padding='same'):
        kh, kw, cin, _ = kernel.shape
        if (kh == 1 and kw == 1) or cin % 16 == 0:
            return R.conv_ep(orig, x, kernel, strides, padding, parts)
        return orig(x, kernel, strides, padding)

    monkeypatch.setattr(ops, 'conv2d', conv2d)
    return orig


def exact_operand(rng, shape):
    """hi + lo with hi in {+-1, +-1.5}, lo in +-{4 .. 7} * 2^-12: the RNE split is exactly (hi, lo, 0); with K <= 288 and a
    scale of at most 2 every kept term of P <= 2 is a multiple of 2^-13 and sum |terms| < 2^24 * 2^-13, so any fp32
    accumulation order is exact (tests/test_gpu_convt_split.py: _exact_operand)."""
    hi = rng.choice(np.array([1.0, -1.0, 1.5, -1.5], np.float32), shape)
    lo = (rng.integers(4, 8, shape) * rng.choice(np.array([1, -1]), shape)).astype(np.float32) * np.float32(2.0 ** -12)
    return hi, lo


def operand(x, ps=None, pb=None, relu=False):
    """The fp32 activation operand of the kernels, relu?(fmaf(x, ps, pb)), as a float32 tensor (the product is exact in fp64,
    the sum rounds to 53 bits, then to 24: differs from the fused rounding on a tie of the second rounding only)."""
    a = torch.from_numpy(np.ascontiguousarray(x)).double()
    if ps is not None:
        a = (a * torch.from_numpy(ps).double() + torch.from_numpy(pb).double()).float().double()
    if relu:
        a = torch.clamp(a, min=0)
    return a.float()


def same_pad(size, k, s):
    out = -(-size // s)
    return max((out - 1) * s + k - size, 0) // 2, out


def conv_on_views(lib, x, cin, w, cout, kh, kw, stride, code, y, tile_cfg=-1, pre=None, pre_relu=False, post=None,
                  post_relu=False, res1=None):
    """dh_conv2d_f32 on channel-slab views: x [N, H, W, ldx] (the first `cin` channels are the input), y [N, OH, OW, ldy] (the
    first `cout` channels are written), w = (packed tensor, Kp, Np), TF-SAME padding.  Returns the return code."""
    from deephar_amd import _lib
    n, h, w_, ldx = x.shape
    pt, oh = same_pad(h, kh, stride)
    pl, ow = same_pad(w_, kw, stride)
    assert tuple(y.shape[:3]) == (n, oh, ow) and x.is_contiguous() and y.is_contiguous()
    a = _lib.ConvArgs()
    a.x, a.w, a.y = x.data_ptr(), w[0].data_ptr(), y.data_ptr()
    if pre is not None:
        a.pre_scale, a.pre_shift = pre[0].data_ptr(), pre[1].data_ptr()
    if post is not None:
        a.post_scale, a.post_shift = post[0].data_ptr(), post[1].data_ptr()
    if res1 is not None:
        a.res1, a.ldr1 = res1.data_ptr(), res1.shape[-1]
    a.N, a.H, a.W, a.Cin, a.ldx = n, h, w_, cin, ldx
    a.OH, a.OW, a.Cout, a.ldy = oh, ow, cout, y.shape[-1]
    a.KH, a.KW, a.SH, a.SW, a.PT, a.PL = kh, kw, stride, stride, pt, pl
    a.K, a.Kp, a.Np = kh * kw * cin, w[1], w[2]
    a.pre_relu, a.post_relu, a.w_split = int(pre_relu), int(post_relu), code
    rc = lib.dh_conv2d_f32(C.byref(a), tile_cfg, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


# ---- the model of the extended scope's model tests ---------------------------------------------------------------------------
def spnet_case(res=256, frames=8, seed=13):
    """Pose-only SPNet (growth 96: the entry flow's 3 x 3 convolutions read 48 and 144 channels), two pyramids, `frames` frames
    of one smooth video, heads fitted to one peak per joint (tests/wellcond.py), conditioning asserted on the fp64 oracle.
    -> (model, x, oracle(dtype) -> outputs, read-out(outputs) -> coordinate arrays)"""
    import wellcond
    from deephar_amd import graph, utils, weights
    from deephar_amd.config import ModelConfig
    from deephar_amd.models import spnet
    from oracle import spnet as osp
    graph.reset_naming()
    m = spnet.build(ModelConfig((res, res, 3), utils.pa16j2d, num_actions=[], num_pyramids=2, action_pyramids=[]))
    weights.init_synthetic(m, seed=0)
    ocfg = dict(num_joints=16, dim=2, num_actions=[], num_pyramids=2, action_pyramids=[], num_levels=4, kernel_size=(5, 5),
                growth=96, image_div=8, num_pose_features=0, num_visual_features=0, sam_alpha=1)
    x = wellcond.video_cuts(1, frames, res, seed)
    x = np.ascontiguousarray(x.reshape((frames,) + x.shape[2:]))
    wellcond.fit_spnet_heads(m, ocfg, x, wellcond.scene_positions(1, frames, 16, seed))
    wd = weights.as_dict(m)
    t64 = {}
    osp.forward(wd, x, ocfg, dtype=torch.float64, taps=t64)
    wellcond.assert_well_conditioned(t64, 'extended-scope SPNet')
    return m, x, lambda dt: osp.forward(wd, x, ocfg, dtype=dt), lambda o: [np.asarray(v)[..., :2] for v in o]


def conv_codes(m):
    """[(step, Cin, w_split)] of the bound convolutions of a model's plan."""
    return [(s, s.ins['x'].C, s.attrs.get('w_split', 0)) for s in m.plan.steps if s.kind == 'conv']
