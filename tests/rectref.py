"""fp64 NumPy statement of the 2-D soft-argmax read-out on H x W maps with H != W.  TEST INFRASTRUCTURE (a plain module,
imported like tests/slabview.py).

Independent of oracle/ops.py (which the GPU tests compare as well): written from the definition, with explicit pixel
coordinates.  For a map h[H, W] of one frame and channel, with r the row and q the column of a pixel:

    p       = exp(alpha h - max) / max(sum exp(alpha h - max), 1e-7)                    (activations.py:3-13)
    x       = sum_{r,q} p[r, q] * q / (W - 1),    y = sum_{r,q} p[r, q] * r / (H - 1)     (linspace_2d, utils/math.py:6-19)
    conf(m) = the largest sum of m over a 2 x 2 window [r, r+1] x [q, q+1], r + 1 < H, q + 1 < W
    conf_raw = conf(conf_scale * h),  conf_prob = conf(p),  gmax = max h

`swapped=True` evaluates the same formulas with the roles of H and W exchanged the way a kernel would get them wrong: the
flat pixel index px = r W + q is split as r' = px // H, q' = px % H, x is normalised by H - 1 and y by W - 1, and the window
is the four pixels px, px + 1, px + H, px + H + 1 under the guard r' + 1 < W && q' + 1 < H.  tests/test_rect_host.py shows that
on every input of the GPU tests this lands far outside the bars -- with H == W it is the identity.
"""
import numpy as np

EPS = 1e-7            # K.epsilon(): the clip of the soft-max denominator


def softargmax(h, alpha=1.0, conf_scale=1.0, swapped=False):
    """h [F, H, W, C] -> dict(xy [F, C, 2], prob [F, H, W, C], conf_raw [F, C, 1], conf_prob [F, C, 1], gmax [F, C]), fp64"""
    h = np.asarray(h, np.float64)
    F, H, W, C = h.shape
    Hs, Ws = (W, H) if swapped else (H, W)                 # the extents the index arithmetic uses
    flat = h.reshape(F, H * W, C)
    px = np.arange(H * W)
    r, q = px // Ws, px % Ws
    z = alpha * flat
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / np.maximum(e.sum(axis=1, keepdims=True), EPS)
    x = (p * (q / (Ws - 1.0))[None, :, None]).sum(axis=1)
    y = (p * (r / (Hs - 1.0))[None, :, None]).sum(axis=1)
    win = px[(r + 1 < Hs) & (q + 1 < Ws)]                  # top-left pixels of the 2 x 2 windows

    def conf(m):
        return (m[:, win] + m[:, win + 1] + m[:, win + Ws] + m[:, win + Ws + 1]).max(axis=1)[..., None]
    return dict(xy=np.stack([x, y], axis=-1), prob=p.reshape(F, H, W, C), conf_raw=conf(conf_scale * flat),
                conf_prob=conf(p), gmax=flat.max(axis=1))


def context_aggregation(ys, yc, pc, J, nctx, alpha):
    """blocks.build_context_aggregation (blocks.py:217-285): ys [F, J, 2], yc [F, J*nctx, 2], pc [F, J*nctx, 1];
    joint j's contexts are rows j*nctx .. j*nctx + nctx - 1.  y = alpha ys + (1 - alpha) sum_k yc pc / sum_k pc."""
    F = ys.shape[0]
    yc, pc = yc.reshape(F, J, nctx, 2), pc.reshape(F, J, nctx, 1)
    return alpha * ys + (1.0 - alpha) * (yc * pc).sum(axis=2) / pc.sum(axis=2)


def transposed(out):
    """the read-outs of h transposed in (H, W), from the read-outs of h: x and y change places, nothing else moves"""
    t = dict(out)
    t['xy'] = out['xy'][..., ::-1]
    t['prob'] = np.swapaxes(out['prob'], 1, 2)
    return t


# ---- the cases the host test (discrimination) and the GPU tests share ---------------------------------------------------
# (F, H, W, C) -> (channels per work-group, staged in LDS) of softargmax2d_kernel, as the library answers (slabview.sam_variant); every
# shape comes with its transpose
SAM_SHAPES = {
    (3, 12, 20, 17): (4, True), (3, 20, 12, 17): (4, True),
    (2, 48, 96, 5): (4, False), (2, 96, 48, 5): (4, False),                # slab of 74 304 B > 60 KiB
    (1024, 3, 5, 16): (16, True), (512, 6, 4, 17): (16, True),             # the second: a one-channel tail group
    (1024, 40, 56, 3): (16, False), (1024, 56, 40, 3): (16, False),        # slab of 143 744 B > 128 KiB
    (2, 3, 300, 4): (4, True), (2, 300, 3, 4): (4, True),                  # a grid longer than the 256 threads
}
SAM_ALPHAS = (1.0, 2.5)
SAM_CONF_SCALE = 4.0
SAM_VIEW = (3, 12, 20, 17)          # the shape of the slab-view and xy_times_conf cases


def sam_input(shape):
    """N(0, 4^2) maps, as tests/test_gpu_ops.py::test_softargmax2d draws them; one array per shape"""
    return (np.random.default_rng(sum(shape)).standard_normal(shape) * 4.0).astype(np.float32)
