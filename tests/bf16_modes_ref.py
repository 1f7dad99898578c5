"""CPU references for the reduced-precision rungs of the split-bf16 GEMM family (Model.gemm_precision = 'bf16x2' / 'bf16',
dh_conv_args.w_split = 3 / 4, csrc/gemm1x1s.hip).  TEST INFRASTRUCTURE: nothing here is used by the package.

The contract both sides share: operands are split by repeated round-to-nearest-even
    x1 = bf16(x),  x2 = bf16(x - x1),  x3 = bf16(x - x1 - x2)
(activations after the optional ReLU prologue, weights on the host), and a mode with P parts computes
    E_P = sum_k sum_{i + j <= P + 1} a_i[k] b_j[k]
with exact products and fp32 accumulation.  Here the split is done with torch.Tensor.bfloat16() (round to nearest even)
and E_P is evaluated in fp64:
    P = 1:  conv(x1, w1)
    P = 2:  conv(x1 + x2, w1 + w2) - conv(x2, w2)
    P = 3:  conv(x, w) - conv(x2, w3) - conv(x3, w2) - conv(x3, w3)            (x = x1 + x2 + x3 exactly)
`emulate(monkeypatch, P)` wraps oracle.ops.conv2d so that every dense convolution the split family could take (pointwise,
or K x K with Cin % 32 == 0) is evaluated as E_P: the fp64 oracle then IS the mode, up to summation order and up to the
layers the engine leaves on fp32 kernels (skinny layers, BN-prologue convolutions, the first layer).  Its distance from
the plain fp64 oracle is what the mode costs by definition -- the bar of tests/test_gpu_bf16_modes.py comes from it."""
import numpy as np
import torch

PARTS = {'bf16x3': 3, 'bf16x2': 2, 'bf16': 1}


def split_parts(x, parts):
    """[x1, .., x_parts] as float32 tensors; x is rounded to float32 first (the kernels' operands are float32)."""
    r = torch.as_tensor(x).to(torch.float32)
    out = []
    for _ in range(parts):
        h = r.bfloat16().to(torch.float32)
        out.append(h)
        r = r - h                      # exact: the residual of a round-to-nearest bf16 fits float32
    return out


def conv_ep(conv, x, kernel, strides, padding, parts):
    """E_P of one convolution, evaluated in x's dtype (float64 for a reference) through `conv` = oracle.ops.conv2d."""
    d = x.dtype
    xs = [p.to(d) for p in split_parts(x, parts)]
    ws = [p.to(d) for p in split_parts(kernel, parts)]
    if parts == 1:
        return conv(xs[0], ws[0], strides, padding)
    if parts == 2:
        return conv(xs[0] + xs[1], ws[0] + ws[1], strides, padding) - conv(xs[1], ws[1], strides, padding)
    full = conv(xs[0] + xs[1] + xs[2], ws[0] + ws[1] + ws[2], strides, padding)
    return full - conv(xs[1], ws[2], strides, padding) - conv(xs[2], ws[1], strides, padding) - \
        conv(xs[2], ws[2], strides, padding)


def emulate(monkeypatch, parts):
    """Patch oracle.ops.conv2d (sepconv2d's pointwise half goes through it too) for the rest of the test."""
    from oracle import ops
    orig = ops.conv2d

    def conv2d(x, kernel, strides=(1, 1), padding='same'):
        kh, kw, cin, _ = kernel.shape
        if (kh == 1 and kw == 1) or cin % 32 == 0:
            return conv_ep(orig, x, kernel, strides, padding, parts)
        return orig(x, kernel, strides, padding)

    monkeypatch.setattr(ops, 'conv2d', conv2d)
    return orig


def px(a, b):
    """Worst distance of two lists of normalised coordinate arrays, in pixels of the 256-px crop."""
    return 256.0 * max(float(np.abs(np.asarray(u, np.float64) - np.asarray(v, np.float64)).max()) for u, v in zip(a, b))


# ---- the four models of tests/test_gpu_bf16x3.py: same builders, seeds and inputs -------------------------------------
def model_case(name):
    """-> (model, x, batch, oracle(dtype) -> outputs, poses(outputs) -> coordinate arrays, actions(outputs) -> score arrays)"""
    from test_gpu_models import _build, _oracle, _merge, _spnet
    if name == 'mpii':
        kw = dict(num_context_per_joint=2, concat_pose_confidence=False)
        m, wd = _build(2, 8, 16, **kw)
        x = np.random.default_rng(0).uniform(-1, 1, (3, 256, 256, 3)).astype(np.float32)
        return (m, x, 3, lambda dt: _oracle(wd, x, 2, 8, 16, dt, **kw)[0],
                lambda o: [v[..., :2] for v in o[::2]], lambda o: [])
    if name == 'h36m':
        m, wd = _build(3, 8, 17, depth_maps=16)
        x = np.random.default_rng(31).uniform(-1, 1, (2, 256, 256, 3)).astype(np.float32)
        return (m, x, 2, lambda dt: _oracle(wd, x, 3, 8, 17, dt, depth_maps=16)[0],
                lambda o: [v[..., :3] for v in o[:8]], lambda o: [])
    if name == 'penn':
        from oracle import action as oact
        T, blocks, nact, joints = 16, 4, 15, 16
        m, wd = _merge(2, T, joints, blocks, pose_net_version='v1', num_actions=nact)
        x = np.random.default_rng(32).uniform(-1, 1, (1, T, 256, 256, 3)).astype(np.float32)
        okw = dict(pose_dim=2, pose_net_version='v1', output_poses=True)
        return (m, x, 1, lambda dt: oact.forward_merge(wd, x, nact, joints, blocks, dtype=dt, **okw),
                lambda o: [o[0][..., :2]], lambda o: list(o[2:]))
    if name == 'ntu':
        from deephar_amd.models import spnet
        from oracle import spnet as osp
        x = np.random.default_rng(11).uniform(-1, 1, (1, 8, 256, 256, 3)).astype(np.float32)
        m, cfg, wd, ocfg = _spnet(8, 'pa17j3d', 60, 2, [1, 2], 192, calibrate=x)
        npose = spnet.get_num_predictions(2, 4)
        return (m, x, 1, lambda dt: osp.forward(wd, x, ocfg, dtype=dt),
                lambda o: [v[..., :3] for v in o[:npose]], lambda o: list(o[npose:]))
    raise KeyError(name)
