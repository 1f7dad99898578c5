"""Shared by tests/test_posebox_host.py and tests/test_gpu_posebox.py: the generator of random items, the Python chain they are
held to (evaltools.bbox.get_bbox_from_poses over frontend.crop_afmat), a long-hand numpy restatement of csrc/posebox_index.h,
the ctypes plumbing of dh_pose_boxes_host, and the edge cases both files put through the host twin and the kernel."""
import numpy as np

OUT_WH = (256, 256)
THR = np.float32(0.25)
OK, NO_JOINT, NAN_JOINT, RANGE, WINDOW = range(5)


def job_rows(src, windows, hflip=0):
    """int32 [n, 6] rows (src, x0, y0, x1, y1, hflip)"""
    rows = np.zeros((len(windows), 6), np.int32)
    rows[:, 0] = src
    rows[:, 1:5] = windows
    rows[:, 5] = hflip
    return rows


def random_windows(rng, n):
    """origin in [-300, 900) x [-300, 500), sides in [32, 1400)"""
    x0, y0 = rng.integers(-300, 900, n), rng.integers(-300, 500, n)
    w, h = rng.integers(32, 1400, n), rng.integers(32, 1400, n)
    return np.stack([x0, y0, x0 + w, y0 + h], axis=1).astype(np.int64)


def random_items(rng, n, F):
    """n items of F frames: per item J in 2..20 and D in {3, 4}, coordinates in [-0.2, 1.2], every other channel (the confidence
    among them) uniform in [0, 1].  -> list of float32 [F, J, D], windows int64 [n, 4]"""
    items = []
    for _ in range(n):
        J, D = int(rng.integers(2, 21)), int(rng.integers(3, 5))
        p = rng.uniform(0.0, 1.0, (F, J, D))
        p[..., 0:2] = rng.uniform(-0.2, 1.2, (F, J, 2))
        items.append(p.astype(np.float32))
    return items, random_windows(rng, n)


def python_chain(item, window, scale=1.5):
    """The reference's arithmetic for one item [F, J, D] -> float64 box, or None where get_valid_bbox raises for a frame that
    keeps no joint"""
    from deephar_amd import frontend
    from deephar_amd.evaltools.bbox import get_bbox_from_poses
    try:
        return get_bbox_from_poses(item, frontend.crop_afmat(window, OUT_WH), scale)
    except ValueError as e:
        assert 'all points are invalid' in str(e)
        return None


def longhand(item, window, relsize=1.5, conf_channel=None, hflip=0):
    """posebox_index.h in numpy scalars, statement for statement: float32 span per frame, exact float union, doubles through the
    window.  -> (int32 box [4], float64 box [4], status)"""
    f32, f64 = np.float32, np.float64
    F, J, D = item.shape
    cc = D - 2 if conf_channel is None else conf_channel
    rs = f32(relsize)
    zero = (np.zeros(4, np.int32), np.zeros(4, np.float64))
    spans, nojoint, nan, wild = [], False, False, False
    with np.errstate(all='ignore'):
        for f in range(F):
            keep = item[f, :, cc] > THR
            if not keep.any():
                nojoint = True
                continue
            u, v = item[f, keep, 0], item[f, keep, 1]
            if np.isnan(u).any() or np.isnan(v).any():
                nan = True
                continue
            ulo, uhi, vlo, vhi = f32(u.min()), f32(u.max()), f32(v.min()), f32(v.max())
            cx, cy = f32(f32(ulo + uhi) / f32(2)), f32(f32(vlo + vhi) / f32(2))
            w, h = f32(rs * f32(uhi - ulo)), f32(rs * f32(vhi - vlo))
            s = h if h > w else w
            half = f32(s / f32(2))
            c = [f32(cx - half), f32(cy - half), f32(cx + half), f32(cy + half)]
            if not np.all(np.isfinite(c)):
                wild = True
                continue
            spans.append(c)
        if nojoint:
            return zero + (NO_JOINT,)
        if nan:
            return zero + (NAN_JOINT,)
        x0, y0, x1, y1 = (int(t) for t in window)
        if hflip or not (x1 > x0 and y1 > y0):
            return zero + (WINDOW,)
        if wild:
            return zero + (RANGE,)
        spans = np.array(spans, np.float32)
        u0, v0, u1, v1 = spans[:, 0].min(), spans[:, 1].min(), spans[:, 2].max(), spans[:, 3].max()
        cw, ch = f64(x1) - f64(x0), f64(y1) - f64(y0)
        ax, ay = f64(x0) + f64(u0) * cw, f64(y0) + f64(v0) * ch
        bx, by = f64(x0) + f64(u1) * cw, f64(y0) + f64(v1) * ch
        box = np.array([min(ax, bx), min(ay, by), max(ax, bx), max(ay, by)], np.float64)
        if not np.all(np.abs(box) < 2147483648.0):
            return zero + (RANGE,)
        return box.astype(np.int32), box, OK


# ---- the twin through ctypes (host memory) ------------------------------------------------------------------------------------
def host_pose_boxes(lib, poses, jobs, relsize=1.5, conf_channel=None, strides=None, F=None, J=None, job_stride=1, n=None, rc=0):
    """dh_pose_boxes_host on a float32 array [n, F, J, D] (or a flat buffer with explicit (item, frame, joint) strides)
    -> (boxes int32 [n, 4], boxes float64 [n, 4], status int32 [n]), written between guard rows that must survive"""
    poses = np.ascontiguousarray(poses, np.float32)
    jobs = np.ascontiguousarray(jobs, np.int32)
    if strides is None:
        n, F, J, D = poses.shape
        strides = (F * J * D, J * D, D)
        if conf_channel is None:
            conf_channel = D - 2
    box = np.full((n + 2, 4), -7777, np.int32)
    boxf = np.full((n + 2, 4), -777.125, np.float64)
    status = np.full((n + 2,), 77, np.int32)
    got = lib.dh_pose_boxes_host(poses.ctypes.data, strides[0], strides[1], strides[2], F, J, conf_channel, jobs.ctypes.data,
                                 job_stride, n, relsize, box[1:].ctypes.data, boxf[1:].ctypes.data, status[1:].ctypes.data)
    assert got == rc, got
    for a, g in ((box, -7777), (boxf, -777.125), (status, 77)):
        assert np.all(a[0] == g) and np.all(a[-1] == g), 'a guard row was written'
    return box[1:-1], boxf[1:-1], status[1:-1]


def strided_items(rng, n, F, J, D, pad_joint=0, pad_frame=0, coff=0, pad_item=3):
    """A flat float32 buffer full of 9e9 with n items [F, J, D] laid into it at a channel offset, a joint stride of D + pad_joint,
    a frame stride above J joints and an item stride above F frames: what a view of a wider arena buffer looks like.
    -> (flat, element offset of item 0, (item, frame, joint) strides, the dense items [n, F, J, D])"""
    js = D + pad_joint
    fs = J * js + pad_frame
    its = F * fs + pad_item
    flat = np.full(coff + n * its + 8, 9e9, np.float32)
    dense = rng.uniform(0.0, 1.0, (n, F, J, D))
    dense[..., 0:2] = rng.uniform(-0.2, 1.2, (n, F, J, 2))
    dense = dense.astype(np.float32)
    for i in range(n):
        for f in range(F):
            for j in range(J):
                o = coff + i * its + f * fs + j * js
                flat[o:o + D] = dense[i, f, j]
    return flat, coff, (its, fs, js), dense


# ---- edge cases: (name, poses [n, F, J, D], job rows [n, 6], relsize, the status to expect per item) -----------------------------
def edge_cases():
    rng = np.random.default_rng(5)
    win = np.array([[100, 80, 400, 380]])

    def good(n=1, F=1, J=16, D=3):
        # every channel in [0.3, 0.9]: whichever is the confidence (D - 2: channel 1, y, when D = 3), every joint is kept
        return rng.uniform(0.3, 0.9, (n, F, J, D)).astype(np.float32)

    cases = [('ok', good(), job_rows(0, win), 1.5, [OK])]
    none = good(F=2)
    none[0, 1, :, 1] = 0.25                                                  # frame 1: no confidence ABOVE the threshold
    cases.append(('keeps_no_joint', none, job_rows(0, win), 1.5, [NO_JOINT]))
    nanc = good()
    nanc[0, 0, :, 1] = np.nan                                                # a NaN confidence keeps nothing
    cases.append(('nan_confidence', nanc, job_rows(0, win), 1.5, [NO_JOINT]))
    nanj = good()
    nanj[0, 0, 7, 0] = np.nan
    cases.append(('nan_joint', nanj, job_rows(0, win), 1.5, [NAN_JOINT]))
    dropped = good()
    dropped[0, 0, 7] = [np.nan, np.nan, 0.1]                                 # NaN > 0.25 is false: not kept, so no harm
    cases.append(('nan_joint_not_kept', dropped, job_rows(0, win), 1.5, [OK]))
    both = good(F=2)
    both[0, 0, 3, 0] = np.nan
    both[0, 1, :, 1] = 0.0
    cases.append(('no_joint_beats_nan', both, job_rows(0, win), 1.5, [NO_JOINT]))
    far = good()
    far[0, 0, 2, 0] = 1e8                                                    # 1e8 * 300 px >= 2^31
    cases.append(('corner_beyond_int32', far, job_rows(0, win), 1.5, [RANGE]))
    inf = good()
    inf[0, 0, 2, 1] = np.inf
    cases.append(('infinite_joint', inf, job_rows(0, win), 1.5, [RANGE]))
    huge = good()
    huge[0, 0, 2, 0], huge[0, 0, 3, 0] = 3e38, -3e38                         # xmax - xmin overflows float32
    cases.append(('float_overflow', huge, job_rows(0, win), 1.5, [RANGE]))
    cases.append(('flipped_window', good(), job_rows(3, win, hflip=1), 1.5, [WINDOW]))
    cases.append(('empty_window', good(), job_rows(2, np.array([[100, 80, 100, 380]])), 1.5, [WINDOW]))
    cases.append(('reversed_window', good(), job_rows(2, np.array([[100, 380, 400, 80]])), 1.5, [WINDOW]))
    cases.append(('J_1', good(J=1), job_rows(0, win), 1.5, [OK]))
    zeros = good(F=2, D=4)                                                   # (D = 4: the confidence is channel 2)
    zeros[0, :, :, 0] = np.array([0.0, -0.0] * 8, np.float32)                # zeros of both signs: the +-0 paragraph
    zeros[0, :, :, 1] = np.array([-0.0, 0.0] * 8, np.float32)
    cases.append(('signed_zeros', zeros, job_rows(0, np.array([[0, 0, 300, 300]])), 1.5, [OK]))
    mixed = good(n=5, F=2)
    mixed[1, 1, :, 1] = 0.2                                                  # kept nothing, between good items
    mixed[3, 0, 5, 0] = np.nan                                           # a NaN joint, between good items
    cases.append(('mixed', mixed, job_rows(np.arange(5), np.repeat(win, 5, axis=0)), 1.2, [OK, NO_JOINT, OK, NAN_JOINT, OK]))
    return cases


def check_case(case, box, boxf, status):
    """the statuses of an edge case as pinned; zero boxes behind a non-zero status; the long-hand restatement bit for bit"""
    name, poses, jobs, relsize, expect = case
    assert status.tolist() == expect, (name, status.tolist())
    for i, st in enumerate(expect):
        wb, wf, ws = longhand(poses[i], jobs[i, 1:5], relsize, hflip=int(jobs[i, 5]))
        assert ws == st, (name, i, ws)
        assert np.array_equal(box[i], wb) and np.array_equal(boxf[i].view(np.uint64), wf.view(np.uint64)), (name, i)
        if st != OK:
            assert not box[i].any() and not boxf[i].view(np.uint64).any(), (name, i)
