"""Box refinement on the GPU: dh_refine_boxes_f64 / dh_jobs_from_boxes_f64 against their host twins bit for bit (boxes as uint64,
jobs as int32) on strided pose views, in place and out of place, between sentinels; refine_pred_frames(loop='device') against
loop='host' on one- and two-stream models; the status path; dh_refine_frames_host through ctypes and from a gcc-compiled host
(tools/c_host/refine_frames.c).  No PIL, no reference checkout."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refinecases as rc  # noqa: E402
from test_gpu_crop import _frames_and_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTIDX = 2
SENT_F, SENT_I = -777.125, -7777


def _device_refine(cuda, flat, off, ss, js, J, jobs, boxes, ws, mom, inplace):
    """dh_refine_boxes_f64 between sentinels: -> (boxes, jobs) as numpy, after checking the guard rows around both"""
    from deephar_amd import _lib
    lib = _lib.load()
    n = len(boxes)
    f = torch.from_numpy(np.ascontiguousarray(flat, np.float32)).to(cuda)
    bin_ = torch.full((n + 2, 4), SENT_F, dtype=torch.float64, device=cuda)
    jin = torch.full((n + 2, 6), SENT_I, dtype=torch.int32, device=cuda)
    bin_[1:n + 1] = torch.from_numpy(np.ascontiguousarray(boxes, np.float64)).to(cuda)
    jin[1:n + 1] = torch.from_numpy(np.ascontiguousarray(jobs, np.int32)).to(cuda)
    if inplace:
        bout, jout = bin_, jin
    else:
        bout = torch.full((n + 2, 4), SENT_F, dtype=torch.float64, device=cuda)
        jout = torch.full((n + 2, 6), SENT_I, dtype=torch.int32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.dh_refine_boxes_f64(f.data_ptr() + 4 * off, ss, js, J, jin[1].data_ptr(), bin_[1].data_ptr(), n, ws, mom,
                                   bout[1].data_ptr(), jout[1].data_ptr(), st) == 0
    torch.cuda.synchronize()
    b, j = bout.cpu().numpy(), jout.cpu().numpy()
    assert np.all(b[0] == SENT_F) and np.all(b[-1] == SENT_F) and np.all(j[0] == SENT_I) and np.all(j[-1] == SENT_I)
    if not inplace:                                                          # the inputs were only read
        assert np.array_equal(bin_.cpu().numpy()[1:-1].view(np.uint64), np.ascontiguousarray(boxes, np.float64).view(np.uint64))
        assert np.array_equal(jin.cpu().numpy()[1:-1], np.ascontiguousarray(jobs, np.int32))
    return b[1:-1], j[1:-1]


def _boxes_for(rng, n):
    cx, cy, side = rng.uniform(100, 1180, n), rng.uniform(100, 620, n), rng.uniform(120.3, 700.7, n)
    return np.stack([cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2], axis=1)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 257])
@pytest.mark.parametrize('J,D,pad_joint,pad_sample,coff', [(1, 2, 0, 0, 0), (16, 4, 0, 5, 3), (17, 2, 1, 0, 1), (65, 4, 2, 9, 2),
                                                           (16, 2, 0, 0, 0)])
def test_refine_boxes_device_equals_host_twin(n, J, D, pad_joint, pad_sample, coff, cuda, hip_lib):
    rng = np.random.RandomState(1000 * n + J)
    flat, off, ss, js, _ = rc.strided_poses(rng, n, J, D, pad_joint, pad_sample, coff)
    boxes = _boxes_for(rng, n)
    jobs = rc.host_jobs_from_boxes(hip_lib, boxes, np.arange(n))
    if n >= 3:                                                               # a flipped and an empty job among the good ones
        jobs[1, 5] = 1
        jobs[2, 3] = jobs[2, 1]
    if n >= 5:
        flat[off + 4 * ss + (J - 1) * js + 1] = np.nan                       # a NaN in the last joint of sample 4
    want_b, want_j = rc.host_refine(hip_lib, flat[off:], jobs, boxes, 1.5, 0.8, sample_stride=ss, joint_stride=js, J=J)
    for inplace in (False, True):
        got_b, got_j = _device_refine(cuda, flat, off, ss, js, J, jobs, boxes, 1.5, 0.8, inplace)
        assert np.array_equal(got_b.view(np.uint64), want_b.view(np.uint64)), ('boxes', inplace)
        assert np.array_equal(got_j, want_j), ('jobs', inplace)


def test_refine_boxes_three_steps_equal_host_twin(cuda, hip_lib):
    """The issue's distribution, 1024 samples, three steps chained on the device (in place) and on the host."""
    from deephar_amd import functional as F
    bbox0, poses = rc.synthetic(n=1024)
    src = np.arange(1024, dtype=np.int32)
    boxes_d = torch.from_numpy(bbox0).to(cuda)
    jobs_d = F.jobs_from_boxes(boxes_d, torch.from_numpy(src).to(cuda))
    jobs_h, cur = rc.host_jobs_from_boxes(hip_lib, bbox0, src), bbox0
    assert np.array_equal(jobs_d.cpu().numpy(), jobs_h)
    for t in range(3):
        F.refine_boxes(torch.from_numpy(poses[t]).to(cuda), jobs_d, boxes_d, out_boxes=boxes_d, out_jobs=jobs_d)
        cur, jobs_h = rc.host_refine(hip_lib, poses[t], jobs_h, cur)
        assert np.array_equal(boxes_d.cpu().numpy().view(np.uint64), cur.view(np.uint64)), t
        assert np.array_equal(jobs_d.cpu().numpy(), jobs_h), t


@pytest.mark.parametrize('case', rc.edge_cases(), ids=lambda c: c[0])
def test_edge_cases_on_device(case, cuda, hip_lib):
    name, poses, jobs, boxes, expect = case
    n, J, D = poses.shape
    want_b, want_j = rc.host_refine(hip_lib, poses, jobs, boxes)
    for inplace in (False, True):
        got_b, got_j = _device_refine(cuda, poses.reshape(-1), 0, J * D, D, J, jobs, boxes, 1.5, 0.8, inplace)
        rc.check_expectation(name, expect, jobs, boxes, got_b, got_j)
        assert np.array_equal(got_b.view(np.uint64), want_b.view(np.uint64)) and np.array_equal(got_j, want_j)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_jobs_from_boxes_device_equals_host_twin(n, cuda, hip_lib):
    rng = np.random.RandomState(n)
    boxes = rng.uniform(-900.0, 1500.0, (n, 4))
    special = np.array([[0, 0, 3e9, 10], [-3e9, 0, 5, 10], [0, 0, np.nan, 10], [0, -np.inf, 5, 10], [0, 0, 2147483648.0, 10],
                        [-0.5, -0.75, 0.5, 0.75], [-10.99, -3.01, -2.5, -1.2]])
    boxes[:min(n, len(special))] = special[:min(n, len(special))]
    src = rng.randint(0, 50, n).astype(np.int32)
    want = rc.host_jobs_from_boxes(hip_lib, boxes, src)
    bd, sd = torch.from_numpy(boxes).to(cuda), torch.from_numpy(src).to(cuda)
    out = torch.full((n + 2, 6), SENT_I, dtype=torch.int32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert hip_lib.dh_jobs_from_boxes_f64(bd.data_ptr(), sd.data_ptr(), n, out[1].data_ptr(), st) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[0] == SENT_I) and np.all(got[-1] == SENT_I) and np.array_equal(got[1:-1], want)


# ---- whole models ----------------------------------------------------------------------------------------------------------
def _model(streams=1):
    from test_gpu_models import _build
    model, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)
    if streams > 1:
        model.num_streams = streams
    return model


@pytest.fixture(scope='module')
def small_model(cuda, hip_lib):
    return _model()


@pytest.fixture(scope='module')
def six(small_model):
    """six frames, float boxes, and the host loop's poses at num_iter = 2 and batch 4: computed once"""
    from deephar_amd.evaltools import mpii_tools
    images, boxes, _ = _frames_and_boxes(6, 11)
    bbox0 = boxes.astype(np.float64) + np.array([0.25, 0.5, 0.75, 0.125])                 # fractional corners, as datasets have
    want = mpii_tools.refine_pred_frames(small_model, images, bbox0, OUTIDX, num_iter=2, batch_size=4)
    for w in want:
        w.setflags(write=False)
    return images, bbox0, want


def _host_loop_windows(bbox0, preds, ws=1.5, mom=0.8):
    """The windows the host loop cropped, from the image-space poses it returned: its own statements again.
    -> (windows [len(preds), N, 4], pre-truncation corners)"""
    from deephar_amd import frontend
    from deephar_amd.utils import bbox_to_objposwin, objposwin_to_bbox
    current = np.array(bbox0, np.float64).copy()
    windows, corners = [], []
    for t, pred in enumerate(preds):
        windows.append(np.stack([frontend.crop_box(*bbox_to_objposwin(b)) for b in current]))
        c = []
        for b in current:
            (cx, cy), (w, h) = bbox_to_objposwin(b)
            c.append([float(cx) - float(w) / 2, float(cy) - float(h) / 2, float(cx) + float(w) / 2, float(cy) + float(h) / 2])
        corners.append(np.array(c))
        refined = current.copy()
        lo, hi = pred[:, :, 0:2].min(axis=1), pred[:, :, 0:2].max(axis=1)
        for i in range(len(pred)):
            centre_p = np.array([(lo[i, 0] + hi[i, 0]) / 2, (lo[i, 1] + hi[i, 1]) / 2])
            side = ws * max(hi[i, 0] - lo[i, 0], hi[i, 1] - lo[i, 1])
            centre_t, _ = bbox_to_objposwin(current[i])
            refined[i, :] = objposwin_to_bbox(mom * centre_t + (1 - mom) * centre_p, (side, side))
        current = refined
    return np.stack(windows).astype(np.int64), np.stack(corners)


@pytest.mark.parametrize('streams,batch', [(1, 4), (1, 8), (2, 4), (2, 8)])
def test_refine_pred_frames_loop_device_equals_host(streams, batch, cuda, hip_lib, small_model, six):
    from deephar_amd.evaltools import mpii_tools
    images, bbox0, want = six
    windows, corners = _host_loop_windows(bbox0, want)
    rc.preconditions(windows, corners)                                       # equality of windows is a fair demand
    model = small_model if streams == 1 else _model(streams)
    if streams > 1:
        model.executor.tune_table = small_model.executor.tune_table         # (tilings never move a bit; this spares the timing)
    got = mpii_tools.refine_pred_frames(model, images, bbox0, OUTIDX, num_iter=2, batch_size=batch, loop='device')
    assert len(got) == len(want) == 2
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), t
    with pytest.raises(ValueError):
        mpii_tools.refine_pred_frames(model, images, bbox0, OUTIDX, loop='gpu')


def test_three_iterations_when_the_host_loop_keeps_them_valid(cuda, hip_lib, small_model, six):
    """With the synthetic weights a third window may be empty; the case runs when the host loop shows that it is not."""
    from deephar_amd.evaltools import mpii_tools
    images, bbox0, _ = six
    try:
        want = mpii_tools.refine_pred_frames(small_model, images, bbox0, OUTIDX, num_iter=3, batch_size=4)
    except (ValueError, ZeroDivisionError) as e:                             # the host loop refuses a window: so must the device loop
        print('host loop at three iterations:', repr(e))
        with pytest.raises(ValueError):
            mpii_tools.refine_pred_frames(small_model, images, bbox0, OUTIDX, num_iter=3, batch_size=4, loop='device')
        return
    windows, corners = _host_loop_windows(bbox0, want)
    rc.preconditions(windows, corners)
    got = mpii_tools.refine_pred_frames(small_model, images, bbox0, OUTIDX, num_iter=3, batch_size=4, loop='device')
    for t, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), t


def test_status_path_raises_after_a_clean_drain(cuda, hip_lib, small_model, six):
    from deephar_amd.evaltools import mpii_tools
    images, bbox0, _ = six
    x = np.random.default_rng(3).integers(0, 256, (3, 256, 256, 3), dtype=np.uint8)
    before = [np.array(o) for o in small_model.predict(x, batch_size=4)]
    bad = bbox0.copy()
    bad[4] = [80.0, 60.0, 50.0, 200.0]                                       # one empty box (x1 < x0)
    with pytest.raises(ValueError):
        mpii_tools.refine_pred_frames(small_model, images, bad, OUTIDX, num_iter=2, batch_size=4)
    with pytest.raises(ValueError, match='iteration 0, sample 4'):
        mpii_tools.refine_pred_frames(small_model, images, bad, OUTIDX, num_iter=2, batch_size=4, loop='device')
    after = small_model.predict(x, batch_size=4)
    for a, b in zip(after, before):
        assert np.array_equal(a, b)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def four_device(small_model, six):
    """frontend.refine_from_frames of the first four frames at batch 4: raw outputs, windows"""
    from deephar_amd import frontend
    images, bbox0, _ = six
    raws, windows, _ = frontend.refine_from_frames(small_model, images[:4], np.arange(4), bbox0[:4], OUTIDX, num_iter=2, batch_size=4)
    return raws, windows


@pytest.mark.parametrize('streams', [1, 2])
def test_dh_refine_frames_host_equals_python_loop(streams, cuda, hip_lib, small_model, six, four_device, tmp_path):
    from deephar_amd import _lib
    lib = hip_lib
    images, bbox0, _ = six
    raws, windows = four_device
    model = small_model
    if streams > 1:
        model = _model(streams)
        model.stream_policy = 'list'
        model.executor.tune_table = small_model.executor.tune_table
    path = str(tmp_path / 'm_u8.dhplan')
    model.export_plan(path, 4, uint8=True, multi_stream=streams > 1)
    blob = open(path, 'rb').read()
    plan, frames = C.c_void_p(), C.c_void_p()
    assert lib.dh_plan_create(blob, len(blob), C.byref(plan)) == 0
    ims = [np.ascontiguousarray(im) for im in images[:4]]
    table = (_lib.CropSrc * 4)(*[_lib.CropSrc(im.ctypes.data, 3 * im.shape[1], im.shape[0], im.shape[1]) for im in ims])
    assert lib.dh_frames_create(table, 4, C.byref(frames)) == 0
    try:
        assert lib.dh_plan_num_streams(plan) == streams and lib.dh_plan_output_channels(plan, OUTIDX) == raws[0].shape[2]
        for n in (4, 3):                                                     # a full batch, then a ragged one
            src = np.arange(n, dtype=np.int32)
            b0 = np.ascontiguousarray(bbox0[:n])
            poses = np.full((2, n) + raws[0].shape[1:], np.nan, np.float32)
            jobs = np.full((2, n, 6), -7, np.int32)
            status = np.full((2, n), 77, np.int32)
            assert lib.dh_refine_frames_host(plan, frames, src.ctypes.data, b0.ctypes.data, n, 256, 256, OUTIDX, 2, 1.5, 0.8,
                                             poses.ctypes.data, jobs.ctypes.data, status.ctypes.data) == 0
            assert not status.any()
            assert np.array_equal(jobs[:, :, 1:5], windows[:, :n]) and np.array_equal(jobs[:, :, 0], np.stack([src, src]))
            for t in range(2):
                assert np.array_equal(poses[t], raws[t][:n]), (n, t)
        # refusals on a real plan
        a = (src.ctypes.data, b0.ctypes.data)
        tail = (poses.ctypes.data, jobs.ctypes.data, status.ctypes.data)
        assert lib.dh_refine_frames_host(plan, frames, *a, 5, 256, 256, OUTIDX, 2, 1.5, 0.8, *tail) == -1
        assert lib.dh_refine_frames_host(plan, frames, *a, 3, 256, 255, OUTIDX, 2, 1.5, 0.8, *tail) == -1
        assert lib.dh_refine_frames_host(plan, frames, *a, 3, 256, 256, lib.dh_plan_num_outputs(plan), 2, 1.5, 0.8, *tail) == -1
        assert lib.dh_refine_frames_host(plan, frames, *a, 3, 256, 256, OUTIDX, 0, 1.5, 0.8, *tail) == -1
        assert lib.dh_refine_frames_host(plan, frames, None, b0.ctypes.data, 3, 256, 256, OUTIDX, 2, 1.5, 0.8, *tail) == -1
    finally:
        torch.cuda.synchronize()
        assert lib.dh_plan_destroy(plan) == 0
        assert lib.dh_frames_destroy(frames) == 0


def test_pure_c_host_refines_frames(hip_lib, cuda, small_model, six, four_device, tmp_path):
    """gcc-compiled host (no Python, no HIP headers): plan file + raw frames + float boxes in; the same windows printed, the
    same raw poses written."""
    images, bbox0, _ = six
    raws, windows = four_device
    small_model.export_plan(str(tmp_path / 'm.dhplan'), 4, uint8=True)
    np.stack(images[:4]).tofile(str(tmp_path / 'frames.u8'))
    np.ascontiguousarray(bbox0[:4]).tofile(str(tmp_path / 'boxes.f64'))
    H, W = images[0].shape[:2]
    exe = str(tmp_path / 'refine_frames')
    libdir = os.path.join(ROOT, 'deephar_amd', 'csrc')
    r = subprocess.run(['gcc', '-O2', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tools', 'c_host', 'refine_frames.c'),
                        '-L' + libdir, '-ldeephar_hip', '-Wl,-rpath,' + libdir, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / 'm.dhplan'), str(tmp_path / 'frames.u8'), str(H), str(W), str(tmp_path / 'boxes.f64'),
                        '256', '256', str(OUTIDX), '2', '1.5', '0.8', str(tmp_path / 'out')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    printed = [[int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith('window ')]
    want = [[t, i] + [int(v) for v in windows[t, i]] + [0] for t in range(2) for i in range(4)]
    assert printed == want
    got = np.fromfile(str(tmp_path / 'out.poses.f32'), np.float32).reshape((2,) + raws[0].shape)
    for t in range(2):
        assert np.array_equal(got[t], raws[t])
