"""Shared by tests/test_refine_host.py and tests/test_gpu_refine.py: the body of evaltools.refine_pred_frames' Python loop lifted
out of the model (synthetic poses stand for the network), the ctypes plumbing of the dh_refine_* / dh_jobs_from_boxes_* twins,
and the edge cases both files put through the host twin and the kernel."""
import ctypes as C

import numpy as np

OUT_HW = (256, 256)
EMPTY = (0, 0, 0, 0, 0)                                   # (x0, y0, x1, y1, hflip) of the empty job


def python_loop(bbox0, poses, winsize_scale=1.5, momentum=0.8, out_hw=OUT_HW):
    """refine_pred_frames' arithmetic, statement for statement, with poses[t] ([N, J, >= 2], crop-normalised) in the place of
    iteration t's prediction.  -> (windows int64 [T + 1, N, 4], boxes float64 [T + 1, N, 4], pre-truncation corners [T + 1, N, 4])
    for T = len(poses) refinement steps."""
    from deephar_amd import frontend
    from deephar_amd.utils import bbox_to_objposwin, objposwin_to_bbox, transform_pose_sequence
    OH, OW = out_hw
    current = np.array(bbox0, dtype=np.float64).copy()
    windows, boxes, corners = [], [], []

    def note(cur):
        windows.append(np.stack([frontend.crop_box(*bbox_to_objposwin(b)) for b in cur]))
        boxes.append(cur.copy())
        c = []
        for b in cur:
            (cx, cy), (w, h) = bbox_to_objposwin(b)
            cx, cy, w, h = float(cx), float(cy), float(w), float(h)
            c.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
        corners.append(np.array(c))

    note(current)
    for t in range(len(poses)):
        A = np.stack([frontend.crop_afmat(w, (OW, OH), False) for w in windows[-1]])
        pred = transform_pose_sequence(A.copy(), poses[t].astype(np.float32), inverse=True)
        refined = current.copy()
        lo, hi = pred[:, :, 0:2].min(axis=1), pred[:, :, 0:2].max(axis=1)
        for i in range(len(pred)):
            centre_p = np.array([(lo[i, 0] + hi[i, 0]) / 2, (lo[i, 1] + hi[i, 1]) / 2])
            side = winsize_scale * max(hi[i, 0] - lo[i, 0], hi[i, 1] - lo[i, 1])
            centre_t, _ = bbox_to_objposwin(current[i])
            refined[i, :] = objposwin_to_bbox(momentum * centre_t + (1 - momentum) * centre_p, (side, side))
        current = refined
        note(current)
    return np.stack(windows).astype(np.int64), np.stack(boxes), np.stack(corners)


def preconditions(windows, corners, out_hw=OUT_HW, near=1e-7):
    """What makes equality of integer windows a fair demand: no corner within `near` of an integer before it is truncated,
    every window non-empty and under the 16x scale cap.  -> (distance of the nearest corner to an integer, the largest scale)"""
    dist = float(np.abs(corners - np.round(corners)).min())
    cw, ch = windows[..., 2] - windows[..., 0], windows[..., 3] - windows[..., 1]
    scale = max(float(cw.max()) / out_hw[1], float(ch.max()) / out_hw[0])
    assert dist > near, 'a corner lies %.3e from an integer' % dist
    assert cw.min() > 0 and ch.min() > 0, 'an empty window'
    assert scale <= 16, 'a window beyond the scale cap'
    return dist, scale


# ---- the twins through ctypes (host memory) -------------------------------------------------------------------------------
def job_rows(src, windows, hflip=0):
    """int32 [n, 6] rows (src, x0, y0, x1, y1, hflip)"""
    n = len(windows)
    rows = np.zeros((n, 6), np.int32)
    rows[:, 0] = src
    rows[:, 1:5] = windows
    rows[:, 5] = hflip
    return rows


def host_jobs_from_boxes(lib, boxes, src):
    boxes = np.ascontiguousarray(boxes, np.float64)
    src = np.ascontiguousarray(src, np.int32)
    jobs = np.full((len(boxes), 6), -7, np.int32)
    assert lib.dh_jobs_from_boxes_host(boxes.ctypes.data, src.ctypes.data, len(boxes), jobs.ctypes.data) == 0
    return jobs


def host_refine(lib, poses, jobs, boxes, ws=1.5, mom=0.8, sample_stride=None, joint_stride=None, J=None, inplace=False, rc=0):
    """dh_refine_boxes_host on a float32 array [n, J, D] (or a flat buffer with explicit strides) -> (boxes, jobs)"""
    poses = np.ascontiguousarray(poses, np.float32)
    jobs = np.ascontiguousarray(jobs, np.int32).copy()
    boxes = np.ascontiguousarray(boxes, np.float64).copy()
    n = len(boxes)
    if J is None:
        J, D = poses.shape[1], poses.shape[2]
        sample_stride, joint_stride = J * D, D
    nb, nj = (boxes, jobs) if inplace else (np.full_like(boxes, -1.25), np.full_like(jobs, -7))
    got = lib.dh_refine_boxes_host(poses.ctypes.data, sample_stride, joint_stride, J, jobs.ctypes.data, boxes.ctypes.data, n,
                                   ws, mom, nb.ctypes.data, nj.ctypes.data)
    assert got == rc, got
    return nb, nj


# ---- edge cases: (name, poses [n, J, D], job rows [n, 6], boxes [n, 4], what to expect per sample) ---------------------------------
def edge_cases():
    """-> list of (name, poses, jobs, boxes, expect) with expect[i] in {'empty', 'nan', 'pass', 'ok'}: the new job is empty (and the
    box what the arithmetic gives), the box is NaN and the job empty, the box passes through and the job is empty, a good job."""
    rng = np.random.RandomState(5)
    box = np.array([[100.5, 80.25, 400.5, 380.25]])
    win = np.array([[100, 80, 400, 380]])
    good = rng.uniform(0.1, 0.9, (1, 16, 3)).astype(np.float32)
    cases = []
    point = np.full((1, 16, 3), 0.5, np.float32)
    cases.append(('one_point', point, job_rows(0, win), box, ['empty']))
    nanj = good.copy()
    nanj[0, 7, 1] = np.nan
    cases.append(('nan_joint', nanj, job_rows(0, win), box, ['nan']))
    far = np.array([[3e9, 80.25, 3e9 + 300, 380.25]])                                      # the new corners lie near 2.4e9 >= 2^31
    cases.append(('corner_3e9', good, job_rows(0, win), far, ['empty']))
    cases.append(('flipped_job', good, job_rows(3, win, hflip=1), box, ['pass']))
    cases.append(('empty_job', good, job_rows(2, np.array([[100, 80, 100, 380]])), box, ['pass']))
    cases.append(('n_1', good, job_rows(0, win), box, ['ok']))
    cases.append(('J_1', good[:, :1], job_rows(0, win), box, ['empty']))                 # one joint is one point
    many = rng.uniform(0.1, 0.9, (5, 16, 3)).astype(np.float32)
    many[1, 0, 0] = np.nan
    rows = job_rows(np.arange(5), np.repeat(win, 5, axis=0))
    rows[3, 5] = 1
    cases.append(('mixed', many, rows, np.repeat(box, 5, axis=0), ['ok', 'nan', 'ok', 'pass', 'ok']))
    return cases


def check_expectation(name, expect, jobs_in, boxes_in, nb, nj):
    qnan = np.uint64(0x7ff8000000000000)
    for i, what in enumerate(expect):
        if what == 'ok':
            assert nj[i, 0] == jobs_in[i, 0] and nj[i, 3] > nj[i, 1] and nj[i, 4] > nj[i, 2] and nj[i, 5] == 0, (name, i)
            continue
        if name == 'one_point' or name == 'J_1':                                           # side 0: a window of no extent
            assert nj[i, 0] == jobs_in[i, 0] and nj[i, 1] == nj[i, 3] and nj[i, 2] == nj[i, 4] and nj[i, 5] == 0, (name, i)
            assert nb[i, 0] == nb[i, 2] and nb[i, 1] == nb[i, 3], (name, i)
            continue
        assert tuple(nj[i]) == (jobs_in[i, 0],) + EMPTY, (name, i, nj[i])
        if what == 'nan':
            assert np.all(nb[i].view(np.uint64) == qnan), (name, i)
        if what == 'pass':
            assert np.array_equal(nb[i].view(np.uint64), np.asarray(boxes_in[i], np.float64).view(np.uint64)), (name, i)


def synthetic(n=4096, J=16, steps=3, seed=0):
    """The distribution of the issue: centres in [100, 1180] x [100, 620], sides in [120.3, 700.7], poses in [0.1, 0.9]^2"""
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(100, 1180, n), rng.uniform(100, 620, n)
    side = rng.uniform(120.3, 700.7, n)
    bbox0 = np.stack([cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2], axis=1)
    poses = rng.uniform(0.1, 0.9, (steps, n, J, 2)).astype(np.float32)
    return bbox0, poses


def strided_poses(rng, n, J, D, pad_joint=0, pad_sample=0, coff=0):
    """A flat float32 buffer full of 9e9 with n poses [J, D >= 2] laid into it at a channel offset, a joint stride of D + pad_joint
    and a sample stride above J joints -> (flat, element offset of pose 0, sample_stride, joint_stride, the dense poses [n, J, 2])"""
    js = D + pad_joint
    ss = J * js + pad_sample
    flat = np.full(coff + n * ss + 8, 9e9, np.float32)
    dense = rng.uniform(0.05, 0.95, (n, J, 2)).astype(np.float32)
    for i in range(n):
        for j in range(J):
            flat[coff + i * ss + j * js: coff + i * ss + j * js + 2] = dense[i, j]
    return flat, coff, ss, js, dense


def c_ptr(a):
    return C.c_void_p(a.ctypes.data)
