"""NumPy restatement of the crop-and-resize front end (include/deephar_hip.h, "Crop-and-resize front end"): PIL's 8-bit
Image.crop(box).resize(size, BILINEAR) [+ FLIP_LEFT_RIGHT] in four steps, and the loaders' box / affine-map bookkeeping
(reference deephar/utils/transform.py:56-120) composed matrix by matrix.  Pure NumPy: no PIL, no GPU, no library."""
import numpy as np

PRECISION_BITS = 22


def axis_taps(n_in, n_out):
    scale = n_in / n_out
    return int(np.ceil(max(scale, 1.0))) * 2 + 1


def axis_coeffs(n_in, n_out):
    """first[out], count[out], k[out, taps] (int64) of one axis; every float is a C double, operation by operation."""
    scale = np.float64(n_in) / np.float64(n_out)
    fs = max(scale, np.float64(1.0))
    support = fs
    ss = np.float64(1.0) / fs
    taps = axis_taps(n_in, n_out)
    first = np.zeros(n_out, np.int64)
    count = np.zeros(n_out, np.int64)
    k = np.zeros((n_out, taps), np.int64)
    for i in range(n_out):
        center = (np.float64(i) + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))               # int() truncates toward zero like a C cast
        xmax = min(n_in, int(center + support + 0.5))
        n = xmax - xmin
        j = np.arange(n, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j + xmin - center + 0.5) * ss))
        ww = np.float64(0.0)
        for v in w:                                               # the sum in index order, like the C loop
            ww += v
        if ww != 0.0:
            w = w / ww
        first[i], count[i] = xmin, n
        k[i, :n] = (0.5 + w * 4194304.0).astype(np.int64)         # values are positive: truncation
    return first, count, k


def _resample_axis0(a, n_out):
    """a: uint8 [n_in, ...] -> uint8 [n_out, ...] along axis 0."""
    n_in = a.shape[0]
    if n_in == n_out:
        return a
    first, count, k = axis_coeffs(n_in, n_out)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    wide = a.astype(np.int64)
    for i in range(n_out):
        kk = k[i, :count[i]].reshape((-1,) + (1,) * (a.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (kk * wide[first[i]:first[i] + count[i]]).sum(axis=0)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def crop(img, box):
    """Step 1: C[y, x] = S[y0 + y, x0 + x] inside the image, 0 outside."""
    x0, y0, x1, y1 = [int(v) for v in box]
    H, W = img.shape[:2]
    out = np.zeros((y1 - y0, x1 - x0) + img.shape[2:], np.uint8)
    sx0, sx1, sy0, sy1 = max(x0, 0), min(x1, W), max(y0, 0), min(y1, H)
    if sx1 > sx0 and sy1 > sy0:
        out[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = img[sy0:sy1, sx0:sx1]
    return out


def crop_resize(img, box, out_hw, hflip=False):
    """img uint8 [H, W, 3], integer box (x0, y0, x1, y1), out_hw = (OH, OW) -> uint8 [OH, OW, 3]."""
    OH, OW = out_hw
    c = crop(np.asarray(img, np.uint8), box)
    h = np.swapaxes(_resample_axis0(np.swapaxes(c, 0, 1), OW), 0, 1)      # horizontal pass, rounded to uint8 ...
    v = _resample_axis0(np.ascontiguousarray(h), OH)                      # ... before the vertical pass reads it
    return np.ascontiguousarray(v[:, ::-1] if hflip else v)


def crop_box(objpos, winsize):
    """transform.py:110-111: the window as integers, truncated toward zero."""
    cx, cy = float(objpos[0]), float(objpos[1])
    w, h = float(winsize[0]), float(winsize[1])
    return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dtype=int)


def _translate(x, y):
    t = np.eye(3)
    t[0, 2], t[1, 2] = x, y
    return t


def _scale(w, h):
    t = np.eye(3)
    t[0, 0] *= w
    t[1, 1] *= h
    return t


def crop_afmat(box, out_wh, hflip=False):
    """The loaders' affine map image -> normalised crop coordinates, np.dot(t, afmat) step by step."""
    x0, y0, x1, y1 = [int(v) for v in box]
    OW, OH = int(out_wh[0]), int(out_wh[1])
    A = np.eye(3)
    A = np.dot(_translate(-x0, -y0), A)
    A = np.dot(_scale(OW / (x1 - x0), OH / (y1 - y0)), A)
    if hflip:
        A = np.dot(_scale(-1, 1), A)
        A = np.dot(_translate(OW, 0), A)
    A = np.dot(_scale(1 / OW, 1 / OH), A)
    return A


def synthetic_image(seed, H, W):
    """Seeded test image: smooth ramps plus noise, so that both interpolation and rounding matter."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 11) % 256, (xx + yy) * 5 % 256], axis=-1)
    noise = rng.integers(0, 256, (H, W, 3))
    return np.where(rng.random((H, W, 1)) < 0.5, base, noise).astype(np.uint8)
