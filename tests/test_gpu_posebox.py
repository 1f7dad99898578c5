"""Person boxes from predicted poses on the GPU: dh_pose_boxes_f64 against its host twin bit for bit (int32 boxes, float64 boxes as
uint64, statuses) on strided pose views between sentinels; the edge cases; predict_frame_bboxes_frames(loop='device') against
loop='host' on one- and two-stream models; a clip-shaped tensor through functional.pose_boxes; the status path;
dh_frame_boxes_host through ctypes and from a gcc-compiled host (tools/c_host/frame_boxes.c).  No PIL, no reference checkout."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropref  # noqa: E402
import poseboxcases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTIDX = 2                                                # the second block's pose [16, 2] of the small model
SENT_F, SENT_I = -777.125, -7777
NEAR = 1e-9


def _device_pose_boxes(cuda, lib, flat, off, strides, F, J, cc, jobs, job_stride, n, relsize=1.5):
    """dh_pose_boxes_f64 between sentinels -> (boxes, float boxes, status) as numpy, after checking the guard rows"""
    f = torch.from_numpy(np.ascontiguousarray(flat, np.float32)).to(cuda)
    jd = torch.from_numpy(np.ascontiguousarray(jobs, np.int32)).to(cuda)
    box = torch.full((n + 2, 4), SENT_I, dtype=torch.int32, device=cuda)
    boxf = torch.full((n + 2, 4), SENT_F, dtype=torch.float64, device=cuda)
    status = torch.full((n + 2,), SENT_I, dtype=torch.int32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.dh_pose_boxes_f64(f.data_ptr() + 4 * off, strides[0], strides[1], strides[2], F, J, cc, jd.data_ptr(), job_stride, n,
                                 relsize, box[1].data_ptr(), boxf[1].data_ptr(), status[1:].data_ptr(), st) == 0
    torch.cuda.synchronize()
    b, q, s = box.cpu().numpy(), boxf.cpu().numpy(), status.cpu().numpy()
    for a, g in ((b, SENT_I), (q, SENT_F), (s, SENT_I)):
        assert np.all(a[0] == g) and np.all(a[-1] == g), 'a guard row was written'
    assert np.array_equal(jd.cpu().numpy(), np.ascontiguousarray(jobs, np.int32))           # the jobs were only read
    return b[1:-1], q[1:-1], s[1:-1]


def _same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)) and
            np.array_equal(got[2], want[2]))


@pytest.mark.parametrize('n', [1, 3, 4, 5, 257])
@pytest.mark.parametrize('F,J,D,pad_joint,pad_frame,coff', [(1, 2, 3, 0, 0, 0), (1, 16, 4, 0, 5, 3), (3, 17, 3, 1, 0, 1),
                                                            (2, 65, 4, 2, 9, 2), (1, 64, 2, 0, 0, 0)])
def test_pose_boxes_device_equals_host_twin(n, F, J, D, pad_joint, pad_frame, coff, cuda, hip_lib):
    rng = np.random.default_rng(1000 * n + 10 * J + F)
    flat, off, strides, _ = pc.strided_items(rng, n, F, J, D, pad_joint, pad_frame, coff)
    windows = pc.random_windows(rng, n)
    table = np.full((n, 2, 6), 7, np.int32)                                  # two jobs per item: the first one is the item's
    table[:, 0] = pc.job_rows(np.arange(n), windows)
    if n >= 5:
        table[2, 0, 5] = 1                                                   # a flipped window among the good ones
        flat[off + 4 * strides[0] + (F - 1) * strides[1] + (J - 1) * strides[2]] = np.nan   # x of the last joint of item 4
    want = pc.host_pose_boxes(hip_lib, flat[off:], table, 1.5, D - 2, strides, F, J, 2, n)
    got = _device_pose_boxes(cuda, hip_lib, flat, off, strides, F, J, D - 2, table, 2, n)
    assert _same(got, want), (got[2].tolist(), want[2].tolist())
    assert (want[2] == pc.OK).any() or n == 1


@pytest.mark.parametrize('case', pc.edge_cases(), ids=lambda c: c[0])
def test_edge_cases_on_device(case, cuda, hip_lib):
    name, poses, jobs, relsize, expect = case
    n, F, J, D = poses.shape
    want = pc.host_pose_boxes(hip_lib, poses, jobs, relsize)
    got = _device_pose_boxes(cuda, hip_lib, poses.reshape(-1), 0, (F * J * D, J * D, D), F, J, D - 2, jobs, 1, n, relsize)
    pc.check_case(case, *got)
    assert _same(got, want)


def test_bad_items_do_not_move_their_neighbours(cuda, hip_lib):
    """a kept-nothing item and a NaN item between good items in one launch: the good items' results are those of a launch
    without the bad ones"""
    rng = np.random.default_rng(9)
    n, F, J, D = 9, 2, 17, 3
    poses = rng.uniform(0.3, 0.9, (n, F, J, D)).astype(np.float32)
    jobs = pc.job_rows(np.arange(n), pc.random_windows(rng, n))
    strides = (F * J * D, J * D, D)
    clean = _device_pose_boxes(cuda, hip_lib, poses.reshape(-1), 0, strides, F, J, D - 2, jobs, 1, n)
    assert not clean[2].any()
    bad = poses.copy()
    bad[3, 1, :, 1] = 0.1                                                    # item 3: frame 1 keeps nothing
    bad[4, 0, 2, 0] = np.nan                                                 # item 4: a kept NaN joint (same work-group as 5..7)
    got = _device_pose_boxes(cuda, hip_lib, bad.reshape(-1), 0, strides, F, J, D - 2, jobs, 1, n)
    assert got[2].tolist() == [0, 0, 0, pc.NO_JOINT, pc.NAN_JOINT, 0, 0, 0, 0]
    keep = np.array([0, 1, 2, 5, 6, 7, 8])
    assert _same(tuple(a[keep] for a in got), tuple(a[keep] for a in clean))
    assert not got[0][3:5].any() and not got[1][3:5].view(np.uint64).any()


def test_functional_pose_boxes_on_a_clip_shaped_tensor(cuda, hip_lib):
    """[N, T, J, D] on the device, dense and as a strided view of a wider tensor; [N, J, D] as well"""
    from deephar_amd import functional as Fn
    rng = np.random.default_rng(11)
    n, T, J, D = 6, 4, 16, 3
    poses = rng.uniform(0.0, 1.0, (n, T, J, D)).astype(np.float32)
    poses[..., 0:2] = rng.uniform(-0.2, 1.2, (n, T, J, 2)).astype(np.float32)
    poses[..., 1] = np.maximum(poses[..., 1], 0.26)                          # (D - 2 = 1: y is the confidence) every joint kept
    windows = pc.random_windows(rng, n)
    want = pc.host_pose_boxes(hip_lib, poses, pc.job_rows(0, windows), 1.5)
    assert not want[2].any()
    for i in range(n):                                                       # and the Python chain, clip by clip
        ref = pc.python_chain(poses[i], windows[i])
        assert np.abs(ref - np.round(ref)).min() > NEAR and np.array_equal(ref.astype(int), want[0][i])
    dense = torch.from_numpy(poses).to(cuda)
    wide = torch.full((n, T, J + 3, D + 5), 9e9, dtype=torch.float32, device=cuda)
    wide[:, :, 1:J + 1, 2:D + 2] = dense
    for t in (dense, wide[:, :, 1:J + 1, 2:D + 2]):
        got = tuple(a.cpu().numpy() for a in Fn.pose_boxes(t, windows, 1.5))
        assert _same(got, want)
    got = tuple(a.cpu().numpy() for a in Fn.pose_boxes(dense[:, 0], torch.from_numpy(windows.astype(np.int32)).to(cuda)))
    assert _same(got, pc.host_pose_boxes(hip_lib, poses[:, :1], pc.job_rows(0, windows), 1.5))
    with pytest.raises(ValueError):
        Fn.pose_boxes(dense[..., :1], windows)
    with pytest.raises(ValueError):
        Fn.pose_boxes(dense, windows[:-1])


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


WINDOWS = np.array([[200, 100, 700, 600], [-40, -30, 360, 370], [600, 200, 1100, 650], [900, 300, 1330, 730],
                    [100, 50, 1000, 700], [333, 111, 777, 666]])


@pytest.fixture(scope='module')
def six(small_model):
    """six 720 x 1280 frames, their windows and keys; the host loop's dictionary at batch 4 and the float boxes of the Python
    chain: computed once"""
    from deephar_amd import frontend
    from deephar_amd.evaltools.bbox import get_bbox_from_poses, predict_frame_bboxes_frames
    images = [cropref.synthetic_image(700 + i, 720, 1280) for i in range(6)]
    keys = ['%d.%d' % (i // 3, i % 3) for i in range(6)]
    index = np.arange(6)
    want = predict_frame_bboxes_frames(small_model, images, index, WINDOWS, keys, batch_size=4, outidx=OUTIDX)   # raises for none
    res = frontend.predict_from_frames(small_model, images, index, WINDOWS, batch_size=4)
    corners = np.stack([get_bbox_from_poses(res[OUTIDX][i:i + 1], res[-1][i], 1.5) for i in range(6)])
    assert np.abs(corners - np.round(corners)).min() > NEAR, 'a host corner lies within 1e-9 of an integer'
    assert [want[k] for k in keys] == corners.astype(int).tolist()
    return images, index, keys, want, corners


@pytest.mark.parametrize('streams,batch', [(1, 4), (1, 8), (2, 4), (2, 8)])
def test_predict_frame_bboxes_frames_loop_device_equals_host(streams, batch, cuda, hip_lib, small_model, six):
    from deephar_amd.evaltools.bbox import predict_frame_bboxes_frames
    images, index, keys, want, _ = six
    model = small_model if streams == 1 else _model(streams)
    if streams > 1:
        model.executor.tune_table = small_model.executor.tune_table         # (tilings never move a bit; this spares the timing)
    got = predict_frame_bboxes_frames(model, images, index, WINDOWS, keys, batch_size=batch, loop='device', outidx=OUTIDX)
    assert got == want
    assert all(isinstance(v, int) for b in got.values() for v in b)
    with pytest.raises(ValueError):
        predict_frame_bboxes_frames(model, images, index, WINDOWS, keys, loop='gpu', outidx=OUTIDX)


def test_frame_boxes_from_frames_float_boxes_and_refusals(cuda, hip_lib, small_model, six):
    from deephar_amd import frontend
    images, index, keys, want, corners = six
    boxes, boxes_f64, status = frontend.frame_boxes_from_frames(small_model, images, index, WINDOWS, outidx=OUTIDX, batch_size=4)
    assert boxes.dtype == np.int64 and not status.any()
    assert boxes.tolist() == [want[k] for k in keys]
    assert np.abs(boxes_f64 - corners).max() <= 4 * 4.55e-13                 # (the bound of tests/test_posebox_host.py)
    with pytest.raises(ValueError):                                          # the last output is [16, 1]: no pose output
        frontend.frame_boxes_from_frames(small_model, images, index, WINDOWS, outidx=-1)
    with pytest.raises(ValueError):
        frontend.frame_boxes_from_frames(small_model, images, index, WINDOWS.astype(np.float64), outidx=OUTIDX)
    with pytest.raises(ValueError):
        frontend.frame_boxes_from_frames(small_model, images, index + 1, WINDOWS, outidx=OUTIDX)


def test_clip_model_loop_device_equals_host(cuda, hip_lib):
    """a clip model (input [T = 4, 256, 256, 3], pose output [4, 16, 2]): index [N, T], one window per item broadcast over its
    frames, the union over the item's frames; three items at batch 2, so the second chunk is ragged"""
    from test_gpu_models import _merge
    from deephar_amd import frontend
    from deephar_amd.evaltools.bbox import get_bbox_from_poses, predict_frame_bboxes_frames
    model, _ = _merge(2, 4, 16, 2, num_actions=15)
    images = [cropref.synthetic_image(800 + i, 360, 480) for i in range(12)]
    index = np.arange(12).reshape(3, 4)
    windows = np.array([[40, 20, 400, 340], [-30, -20, 300, 310], [100, 50, 470, 355]])
    keys = ['a', 'b', 'c']
    want = predict_frame_bboxes_frames(model, images, index, windows, keys, batch_size=2, outidx=0)       # raises for none
    res = frontend.predict_from_frames(model, images, index, windows, batch_size=2)
    assert res[0].shape == (3, 4, 16, 2) and res[-1].shape == (3, 4, 3, 3)
    corners = np.stack([get_bbox_from_poses(res[0][i:i + 1], res[-1][i, 0], 1.5) for i in range(3)])
    assert np.abs(corners - np.round(corners)).min() > NEAR, 'a host corner lies within 1e-9 of an integer'
    assert [want[k] for k in keys] == corners.astype(int).tolist()
    got = predict_frame_bboxes_frames(model, images, index, windows, keys, batch_size=2, loop='device', outidx=0)
    assert got == want
    boxes, boxes_f64, status = frontend.frame_boxes_from_frames(model, images, index, windows, outidx=0, batch_size=2)
    assert not status.any() and np.abs(boxes_f64 - corners).max() <= 4 * 4.55e-13
    with pytest.raises(ValueError):
        frontend.frame_boxes_from_frames(model, images, np.arange(12), windows, outidx=0)   # a clip model needs [N, T] indices
    with pytest.raises(ValueError):
        frontend.frame_boxes_from_frames(model, images, index, windows, outidx=2)           # [15] is no pose output


def test_status_path_raises_after_a_clean_drain(cuda, hip_lib, small_model, six, monkeypatch):
    """A sample that keeps no joint raises the reference's ValueError under both loops, after a clean drain.  The small model's
    poses are whatever its synthetic weights give, so the sample is made with a stubbed pose tensor: output OUTIDX of sample 4
    is overwritten where the forward leaves it (loop='device' reads it in the arena, loop='host' gets it copied out)."""
    from deephar_amd import functional as Fn
    from deephar_amd.evaltools.bbox import predict_frame_bboxes_frames
    images, index, keys, want, _ = six
    x = np.random.default_rng(3).integers(0, 256, (3, 256, 256, 3), dtype=np.uint8)
    before = [np.array(o) for o in small_model.predict(x, batch_size=4)]
    # the op on the stub alone
    stub = torch.full((3, 16, 2), 0.5, dtype=torch.float32, device=cuda)
    stub[1, :, 0] = 0.2                                                      # (D = 2: x is the confidence) nothing above 0.25
    _, _, status = Fn.pose_boxes(stub, WINDOWS[:3])
    assert status.cpu().tolist() == [0, pc.NO_JOINT, 0]
    # the whole pass, both loops: the forward of this executor zeroes the x of sample 4 of every chunk that has one
    ex = small_model.executor
    forward = ex.forward

    def stubbed(bp):
        forward(bp)
        if bp.n > 4:
            with torch.cuda.stream(ex.stream):
                bp.tensor(ex.plan.outputs[OUTIDX])[4, :, 0] = 0.0
    monkeypatch.setattr(ex, 'forward', stubbed)
    for loop in ('host', 'device'):
        with pytest.raises(ValueError, match=r'get_valid_bbox: all points are invalid! \(sample 4'):
            predict_frame_bboxes_frames(small_model, images, index, WINDOWS, keys, batch_size=8, loop=loop, outidx=OUTIDX)
    monkeypatch.undo()
    assert predict_frame_bboxes_frames(small_model, images, index, WINDOWS, keys, batch_size=8, loop='device', outidx=OUTIDX) == want
    after = small_model.predict(x, batch_size=4)
    for a, b in zip(after, before):
        assert np.array_equal(a, b)
    # a window the program builder refuses: the error of the host path, after the drain
    bad = WINDOWS.copy()
    bad[2] = [80, 60, 50, 200]
    for loop in ('host', 'device'):
        with pytest.raises(ValueError, match='empty crop box'):
            predict_frame_bboxes_frames(small_model, images, index, bad, keys, batch_size=4, loop=loop, outidx=OUTIDX)
    after = small_model.predict(x, batch_size=4)
    for a, b in zip(after, before):
        assert np.array_equal(a, b)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def four_device(small_model, six):
    from deephar_amd import frontend
    images, index, _, _, _ = six
    return frontend.frame_boxes_from_frames(small_model, images[:4], index[:4], WINDOWS[:4], outidx=OUTIDX, batch_size=4)


@pytest.mark.parametrize('streams', [1, 2])
def test_dh_frame_boxes_host_equals_frame_boxes_from_frames(streams, cuda, hip_lib, small_model, six, four_device, tmp_path):
    from deephar_amd import _lib
    lib = hip_lib
    images = six[0]
    boxes, boxes_f64, status = four_device
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
        assert lib.dh_plan_num_streams(plan) == streams
        for n in (4, 3):                                                     # a full batch, then a ragged one
            src = np.arange(n, dtype=np.int32)
            win = np.ascontiguousarray(WINDOWS[:n], np.int32)
            b = np.full((n, 4), -7, np.int32)
            q = np.full((n, 4), np.nan)
            s = np.full((n,), 77, np.int32)
            assert lib.dh_frame_boxes_host(plan, frames, src.ctypes.data, win.ctypes.data, n, 256, 256, OUTIDX, 1.5, b.ctypes.data,
                                           q.ctypes.data, s.ctypes.data) == 0
            assert not s.any() and np.array_equal(b, boxes[:n])
            assert np.array_equal(q.view(np.uint64), boxes_f64[:n].view(np.uint64))
        # refusals on a real plan
        a = (src.ctypes.data, win.ctypes.data)
        tail = (b.ctypes.data, q.ctypes.data, s.ctypes.data)
        assert lib.dh_frame_boxes_host(plan, frames, *a, 5, 256, 256, OUTIDX, 1.5, *tail) == -1
        assert lib.dh_frame_boxes_host(plan, frames, *a, 3, 256, 255, OUTIDX, 1.5, *tail) == -1
        assert lib.dh_frame_boxes_host(plan, frames, *a, 3, 256, 256, lib.dh_plan_num_outputs(plan), 1.5, *tail) == -1
        assert lib.dh_frame_boxes_host(plan, frames, *a, 3, 256, 256, 1, 1.5, *tail) == -1           # output 1 is [16, 1]
        assert lib.dh_frame_boxes_host(plan, frames, None, win.ctypes.data, 3, 256, 256, OUTIDX, 1.5, *tail) == -1
        empty = win.copy()
        empty[1, 2] = empty[1, 0]
        assert lib.dh_frame_boxes_host(plan, frames, src.ctypes.data, empty.ctypes.data, 3, 256, 256, OUTIDX, 1.5, *tail) == -1
    finally:
        torch.cuda.synchronize()
        assert lib.dh_plan_destroy(plan) == 0
        assert lib.dh_frames_destroy(frames) == 0


def test_pure_c_host_boxes_frames(hip_lib, cuda, small_model, six, four_device, tmp_path):
    """gcc-compiled host (no Python, no HIP headers): plan file + raw frames + windows in; the same boxes printed and written"""
    images = six[0]
    boxes, boxes_f64, status = four_device
    small_model.export_plan(str(tmp_path / 'm.dhplan'), 4, uint8=True)
    np.stack(images[:4]).tofile(str(tmp_path / 'frames.u8'))
    np.ascontiguousarray(WINDOWS[:4], np.int32).tofile(str(tmp_path / 'windows.i32'))
    H, W = images[0].shape[:2]
    exe = str(tmp_path / 'frame_boxes')
    libdir = os.path.join(ROOT, 'deephar_amd', 'csrc')
    r = subprocess.run(['gcc', '-O2', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tools', 'c_host', 'frame_boxes.c'),
                        '-L' + libdir, '-ldeephar_hip', '-Wl,-rpath,' + libdir, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / 'm.dhplan'), str(tmp_path / 'frames.u8'), str(H), str(W), str(tmp_path / 'windows.i32'),
                        '256', '256', str(OUTIDX), '1.5', str(tmp_path / 'out')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    printed = [[int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith('box ')]
    assert printed == [[i] + [int(v) for v in boxes[i]] + [0] for i in range(4)]
    assert np.array_equal(np.fromfile(str(tmp_path / 'out.boxes.i32'), np.int32).reshape(4, 4), boxes)
    assert np.array_equal(np.fromfile(str(tmp_path / 'out.boxes.f64'), np.uint64).reshape(4, 4), boxes_f64.view(np.uint64))
    assert not np.fromfile(str(tmp_path / 'out.status.i32'), np.int32).any()
