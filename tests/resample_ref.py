"""CPU restatement (torch, fp32 / fp64) of the learned-resampling flavour of SPNet, downsampling_type='conv'
(reference deephar/models/common.py:25-108, deephar/models/spnet.py:151-352, deephar/layers.py:74-89).  TEST INFRASTRUCTURE.

The oracle package restates the max-pooling flavour only; what the 'conv' flavour adds -- SeparableConv2D at a stride,
Conv2DTranspose((2, 2), strides=(2, 2)), the stride-2 residual unit, the BN -> ReLU -> Conv2DTranspose up-scaling unit --
is restated here on top of oracle.ops, and the pose-only forward that returns the heat-map logits with it.
"""
import numpy as np
import torch

from oracle import ops
from oracle.naming import Weights
from oracle.spnet import StopForward, prediction_branch


# ---- ops ---------------------------------------------------------------------------------------------------
def dwconv_strided(x, dw_kernel, strides=(2, 2), pre_scale=None, pre_shift=None, pre_relu=False):
    """relu?(x * scale + shift) -> depthwise conv at a stride, TF-SAME (zero padding AFTER the prologue).
    x [N,H,W,C] torch, dw_kernel [kh,kw,C,1]."""
    if pre_scale is not None:
        x = x * pre_scale + pre_shift
    if pre_relu:
        x = ops.relu(x)
    return ops.depthwise_conv2d(x, dw_kernel, strides, 'same')


def conv_transpose2x2(x, w, pre_scale=None, pre_shift=None, pre_relu=False, res=None, post_relu=False):
    """Conv2DTranspose(filters, (2, 2), strides=(2, 2), padding='same', use_bias=False): x [N,H,W,Cin], w in the Keras layout
    [2,2,Cout,Cin]; y[n, 2i+a, 2j+b, :] = W[a, b] @ x[n, i, j, :] (no kernel flip) = torch's conv_transpose2d with the
    kernel as [Cin, Cout, kh, kw]."""
    if pre_scale is not None:
        x = x * pre_scale + pre_shift
    if pre_relu:
        x = ops.relu(x)
    y = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1).contiguous(), stride=2)
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + res
    return ops.relu(y) if post_relu else y


# ---- units (weights by name, oracle.naming.Weights) --------------------------------------------------------------
def _bn(W, x, name):
    c = x.shape[-1]
    return ops.batchnorm(x, W.get(name, 'beta', (c,)), W.get(name, 'moving_mean', (c,)),
                         W.get(name, 'moving_variance', (c,)), gamma=W.get(name, 'gamma', (c,)))


def _conv(W, x, filters, size, name, strides=(1, 1)):
    return ops.conv2d(x, W.get(name, 'kernel', (size[0], size[1], x.shape[-1], filters)), strides, 'same')


def _sepconv(W, x, filters, size, name, strides=(1, 1)):
    dw = W.get(name, 'depthwise_kernel', (size[0], size[1], x.shape[-1], 1))
    pw = W.get(name, 'pointwise_kernel', (1, 1, x.shape[-1], filters))
    return ops.sepconv2d(x, dw, pw, strides, 'same')


def residual_unit(W, x, kernel_size, name, strides=(1, 1), out_size=None, convtype='depthwise', features_div=2):
    """common.residual_unit (common.py:25-67), any stride."""
    nf = x.shape[-1]
    out_size = nf if out_size is None else out_size
    project = nf != out_size or tuple(strides) != (1, 1)
    normed = _bn(W, x, name + '_bn1')
    shortcut = _conv(W, ops.relu(normed), out_size, (1, 1), name + '_shortcut_conv', strides) if project else x
    y = ops.relu(normed)
    if convtype == 'depthwise':
        y = _sepconv(W, y, out_size, kernel_size, name + '_conv1', strides)
    else:
        y = _conv(W, y, int(out_size / features_div), (1, 1), name + '_conv1')
        y = ops.relu(_bn(W, y, name + '_bn2'))
        y = _conv(W, y, out_size, kernel_size, name + '_conv2', strides)
    return shortcut + y


def downscaling_unit(W, x, kernel_size, name, out_size):
    """common.downscaling_unit, downsampling_type='conv' (common.py:70-86): a stride-2 residual unit."""
    return residual_unit(W, x, kernel_size, name + '_r0', strides=(2, 2), out_size=out_size)


def upscaling_unit(W, x, name, out_size):
    """common.upscaling_unit, downsampling_type='conv' (common.py:103-106): BN -> ReLU -> Conv2DTranspose."""
    w = W.get(name + '_convtrans1', 'kernel', (2, 2, out_size, x.shape[-1]))
    return conv_transpose2x2(ops.relu(_bn(W, x, name + '_bn1')), w)


def mini_pyramid(weights, x, growth=32, kernel_size=(5, 5), levels=3, dtype=torch.float32):
    """Three down-scaling units, then three up-scaling units with lateral adds (the wiring of spnet.py:251-314 without the
    prediction blocks): names 'du<i>' / 'uu<i>'."""
    W = Weights(weights, dtype)
    with torch.no_grad():
        xs = [torch.from_numpy(np.ascontiguousarray(x)).to(dtype)]
        for i in range(1, levels + 1):
            xs.append(downscaling_unit(W, xs[-1], kernel_size, 'du%d' % i, xs[-1].shape[-1] + growth))
        y = xs[-1]
        for i in range(levels - 1, -1, -1):
            y = upscaling_unit(W, y, 'uu%d' % i, y.shape[-1] - growth) + xs[i]
        return y.numpy()


MINI_LAYERS = 9      # GEMM / depthwise layers on the longest path: 3 x (depthwise + pointwise) down, 3 transposed convs up


def build_mini_pyramid():
    """(model with synthetic weights, its weight dict): the graph mini_pyramid above restates, out of the public builders"""
    from deephar_amd import Model, graph, layers as L, utils, weights
    from deephar_amd.config import ModelConfig
    from deephar_amd.models.common import downscaling_unit, upscaling_unit
    graph.reset_naming()
    cfg = ModelConfig((16, 16, 96), utils.pa16j2d, kernel_size=(5, 5), growth=32, downsampling_type='conv')
    x = L.Input((16, 16, 96))
    xs = [x]
    for i in (1, 2, 3):
        xs.append(downscaling_unit(xs[-1], cfg, out_size=xs[-1].shape[-1] + cfg.growth, name='du%d' % i))
    y = xs[-1]
    for i in (2, 1, 0):
        y = L.add([upscaling_unit(y, cfg, out_size=y.shape[-1] - cfg.growth, name='uu%d' % i), xs[i]])
    m = Model(x, y, name='mini_pyramid')
    weights.init_synthetic(m, seed=0)
    return m, weights.as_dict(m)


def entry_flow(W, x, growth=96, image_div=8):
    """spnet.entry_flow (spnet.py:317-352), downsampling_type='conv': stride-2 'normal' residual units instead of pooling."""
    x = _conv(W, x, 64, (7, 7), 'conv1', (2, 2))
    x = residual_unit(W, x, (3, 3), 'res0', out_size=growth, convtype='normal')
    x = ops.maxpool2d(x, (3, 3), (2, 2), 'same')
    x = residual_unit(W, x, (3, 3), 'res1', out_size=2 * growth, convtype='normal')
    x = residual_unit(W, x, (3, 3), 'res2', out_size=2 * growth, convtype='normal')
    nf, cnt, div = 2 * growth, 2, 4
    while div < image_div:
        nf += growth
        x = residual_unit(W, x, (3, 3), 'res%d' % (cnt + 1), strides=(2, 2), out_size=nf, convtype='normal')
        x = residual_unit(W, x, (3, 3), 'res%d' % (cnt + 2), out_size=nf, convtype='normal')
        cnt += 2
        div *= 2
    return x


def spnet_pose_forward(weights, frames, cfg, dtype=torch.float32, taps=None):
    """Pose-only SPNet, downsampling_type='conv' (spnet.build without actions).  cfg: dict(num_joints, dim, num_pyramids,
    num_levels, kernel_size, growth, image_div, sam_alpha).  frames [N, H, W, 3].  Returns the poses [N, J, dim + 1] of
    every prediction block; taps (a dict) receives '<block>/logits' (and '/dlogits' for 3-D); a true 'want_head_inputs' in it
    also records '<block>_heatmaps/in', the tensor the 1x1 heads read, and 'stop_at' ends the pass there (StopForward)."""
    W = Weights(weights, dtype)
    J, dim, ks, growth = cfg['num_joints'], cfg['dim'], cfg['kernel_size'], cfg['growth']
    alpha = cfg.get('sam_alpha', 1)
    poses = []
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(frames)).to(dtype)

        def prediction_block(xp, name, last):
            """spnet.prediction_block (spnet.py:151-248), pose stream"""
            nf = xp.shape[-1]
            xp = residual_unit(W, xp, ks, name + '_r1')
            reinject = [xp]
            xp = ops.relu(_bn(W, xp, name + '_bn1'))
            xp = _sepconv(W, xp, nf, ks, name + '_conv1')
            reinject.append(xp)
            xp = _bn(W, xp, name + '_bn2')
            x1, org_h, _ = prediction_branch(W, xp, J, name + '_heatmaps', pred_activate=True, reinject=not last, taps=taps)
            reinject.append(x1)
            if taps is not None:
                taps[name + '/logits'] = org_h.numpy().copy()
            h = ops.channel_softmax_2d(org_h, alpha)
            p = ops.softargmax2d_from_prob(h)
            c = ops.joints_probability(h)
            if dim == 3:
                x1, org_d, _ = prediction_branch(W, xp, J, name + '_depthmaps', pred_activate=False, forward_maps=False,
                                                 reinject=not last)
                reinject.append(x1)
                if taps is not None:
                    taps[name + '/dlogits'] = org_d.numpy().copy()
                p = torch.cat([p, (torch.sigmoid(org_d) * h).sum(dim=(1, 2)).unsqueeze(-1)], dim=-1)
            poses.append(torch.cat([p, c], dim=-1))
            if last:
                return None
            xp = reinject[0]
            for r in reinject[1:]:
                xp = xp + r
            return xp

        L = cfg['num_levels']
        lp = [None] * L
        lp[0] = entry_flow(W, x, growth, cfg.get('image_div', 8))
        for pyr in range(cfg['num_pyramids']):
            down = pyr % 2 == 0
            name = ('dp%d' if down else 'up%d') % (pyr + 1)
            xp = lp[0] if down else lp[-1]
            levels = list(range(1, L) if down else range(L - 1)[::-1])
            for i in levels:
                if down:
                    xp = downscaling_unit(W, xp, ks, name + '_du%d' % i, xp.shape[-1] + growth)
                else:
                    xp = upscaling_unit(W, xp, name + '_uu%d' % i, xp.shape[-1] - growth)
                if lp[i] is not None:
                    xp = xp + lp[i]
                xp = prediction_block(xp, name + '_pb%d' % i, last=i == levels[-1] and pyr == cfg['num_pyramids'] - 1)
                lp[i] = xp
        return [o.numpy() for o in poses]


def fit_pose_heads(model, cfg, frames, pos):
    """tests/wellcond.py's closed-form "training" of the 1x1 heat-map heads (fit_spnet_heads), on the 'conv' flavour: every
    '<block>_heatmaps_conv1' is fitted, in prediction order, by ridge regression of the tensor it reads (fp32 restatement) onto
    one Gaussian peak per (frame, joint) at `pos` [F, J, 2], then scaled until max S = wellcond.S_TARGET -- read-outs
    conditioned like a trained network's, where fp32 can resolve 1e-3 px.  frames [F, H, W, 3]."""
    import wellcond
    from deephar_amd import weights
    layers = {l.name: l for n in model._nodes for l in n.layers.values()}
    taps = {}
    spnet_pose_forward(weights.as_dict(model), frames, cfg, taps=taps)
    for b in [k[:-len('/logits')] for k in taps if k.endswith('/logits')]:
        taps = {'want_head_inputs': True, 'stop_at': b + '_heatmaps/in'}
        try:
            spnet_pose_forward(weights.as_dict(model), frames, cfg, taps=taps)
        except StopForward:
            pass
        f = taps[b + '_heatmaps/in'].astype(np.float64)
        n, h, w, c = f.shape
        x = f.reshape(-1, c)
        y = wellcond.peak_targets(pos, h, w).reshape(n * h * w, -1)
        g = x.T @ x
        k = np.linalg.solve(g + wellcond.RIDGE * np.trace(g) / c * np.eye(c), x.T @ y)
        k *= wellcond._scale_for((x @ k).reshape(n, h, w, -1), wellcond.S_TARGET)
        p = layers[b + '_heatmaps_conv1'].params[0]
        p.set(k.reshape(p.shape).astype(np.float32))
