"""The crop program built on the GPU (dh_crop_program_build_dev) against the host builder, byte for byte, in buffers with
sentinel bytes behind the program; a table with refused jobs in it; functional.crop_resize / predict_from_frames /
refine_pred_frames under program='device' against program='host' and tests/cropref.py; dh_frames_* and dh_forward_frames
through ctypes and from a gcc-compiled host (tools/c_host/predict_frames.c).  No PIL, no reference checkout."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropref  # noqa: E402
from test_gpu_crop import OP_CASES, _as_list, _frames_and_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DH_EINVAL, DH_EUNSUPPORTED = -1, -2
GUARD = 64


def _sources(cuda, images, pitches=None):
    """-> (the device tensors, CropSrc table with DEVICE pointers)"""
    from deephar_amd import _lib
    keep = []
    srcs = (_lib.CropSrc * len(images))()
    for i, im in enumerate(images):
        H, W = im.shape[:2]
        pitch = pitches[i] if pitches else 3 * W
        wide = np.full((H, pitch), 0xAB, np.uint8)
        wide[:, :3 * W] = im.reshape(H, 3 * W)
        t = torch.from_numpy(wide).to(cuda)
        keep.append(t)
        srcs[i] = _lib.CropSrc(t.data_ptr(), pitch, H, W)
    return keep, srcs


def _job_table(jobs):
    from deephar_amd import _lib
    return (_lib.CropJob * len(jobs))(*[_lib.CropJob(int(s), int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(f)) for s, b, f in jobs])


def _upload(cuda, table):
    return torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(cuda)


def build_dev(lib, cuda, srcs, jobs, OH, OW):
    """The device builder into a 0xCD-filled buffer of max_bytes + GUARD -> (program buffer as np.uint8, status, capacity)."""
    cj = _job_table(jobs)
    cap = C.c_size_t(0)
    assert lib.dh_crop_program_max_bytes(len(jobs), len(srcs), OH, OW, C.byref(cap)) == 0
    buf = torch.full((cap.value + GUARD,), 0xCD, dtype=torch.uint8, device=cuda)
    status = torch.full((len(jobs),), 77, dtype=torch.int32, device=cuda)
    sd, jd = _upload(cuda, srcs), _upload(cuda, cj)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.dh_crop_program_build_dev(sd.data_ptr(), len(srcs), jd.data_ptr(), len(jobs), OH, OW, buf.data_ptr(), cap.value,
                                         status.data_ptr(), st) == 0
    torch.cuda.synchronize()
    return buf, status.cpu().numpy(), cap.value


def build_host(lib, srcs, jobs, OH, OW):
    cj = _job_table(jobs)
    n = C.c_size_t(0)
    assert lib.dh_crop_program_bytes(cj, len(jobs), len(srcs), OH, OW, C.byref(n)) == 0
    prog = np.zeros(n.value // 8 + 1, np.uint64)
    assert lib.dh_crop_program_build_host(srcs, len(srcs), cj, len(jobs), OH, OW, prog.ctypes.data, n.value) == 0
    return prog.view(np.uint8)[:n.value]


def same_program(lib, cuda, srcs, jobs, OH, OW):
    buf, status, cap = build_dev(lib, cuda, srcs, jobs, OH, OW)
    dev = buf.cpu().numpy()
    want = build_host(lib, srcs, jobs, OH, OW)
    nbytes = int(dev[28:32].view(np.uint32)[0])                                  # CropHeader.bytes
    assert nbytes == want.size <= cap, (nbytes, want.size, cap)
    assert np.all(status == 0), status
    if not np.array_equal(dev[:nbytes], want):
        at = int(np.flatnonzero(dev[:nbytes] != want)[0])
        raise AssertionError('programs differ from byte %d of %d on (%d differ)' % (at, nbytes, int((dev[:nbytes] != want).sum())))
    assert np.all(dev[nbytes:] == 0xCD), 'bytes at or behind header.bytes were written'
    return buf, nbytes


@pytest.mark.parametrize('name', sorted(OP_CASES))
def test_device_program_equals_host_program(name, cuda, hip_lib):
    shapes, jobs, OH, OW, pitches = OP_CASES[name]
    images = [cropref.synthetic_image(i, h, w) for i, (h, w) in enumerate(shapes)]
    keep, srcs = _sources(cuda, images, pitches)
    same_program(hip_lib, cuda, srcs, jobs, OH, OW)


def test_device_program_720x1280_to_256(cuda, hip_lib):
    keep, srcs = _sources(cuda, [np.zeros((720, 1280, 3), np.uint8)])
    same_program(hip_lib, cuda, srcs, [(0, (300, 60, 900, 660), 0), (0, (800, 300, 1400, 900), 1)], 256, 256)


@pytest.mark.parametrize('OH,OW', [(4, 4), (5, 7)])
def test_device_program_axis_sweep(OH, OW, cuda, hip_lib):
    """128 jobs whose windows run through every width and height 1 ... 64 (64 / 4 is the scale cap): every division and
    rounding of a small axis, odd and even output extents (the padded and the unpadded table), taps 3 ... 33."""
    keep, srcs = _sources(cuda, [np.zeros((70, 70, 3), np.uint8)])
    jobs = [(0, (i % 5 - 2, i % 3, i % 5 - 2 + i + 1, i % 3 + 64 - i), i % 2) for i in range(64)]          # w = i + 1, h = 64 - i
    jobs += [(0, (3, -1, 3 + i + 1, -1 + i + 1), 0) for i in range(64)]                                    # w = h = i + 1
    assert {b[2] - b[0] for _, b, _ in jobs} == {b[3] - b[1] for _, b, _ in jobs} == set(range(1, 65))
    buf, nbytes = same_program(hip_lib, cuda, srcs, jobs, OH, OW)
    prog = buf.cpu().numpy()
    job_off = int(prog[24:28].view(np.uint32)[0])
    taps = prog[job_off:job_off + 48 * 128].view(np.int32).reshape(128, 12)[:, 6:8]
    if (OH, OW) == (4, 4):
        assert set(taps[:, 0].tolist()) == set(taps[:, 1].tolist()) == set(range(3, 34, 2))


def test_device_program_layout_scan_crosses_its_chunk(cuda, hip_lib):
    """300 jobs: the layout launch scans 256 jobs at a time and carries the running offset into the second chunk."""
    keep, srcs = _sources(cuda, [np.zeros((70, 70, 3), np.uint8), np.zeros((9, 9, 3), np.uint8)])
    jobs = [(j % 2, (j % 7 - 3, j % 4, j % 7 - 3 + 1 + (j * 7) % 64, j % 4 + 1 + (j * 13) % 64), j % 2) for j in range(300)]
    same_program(hip_lib, cuda, srcs, jobs, 4, 4)


def test_mixed_table_refuses_jobs_in_place(cuda, hip_lib):
    """Good jobs with an empty box, a source index out of range and a window beyond the scale cap among them: their status says
    so, their records are skipped by the crop launch (items left as they were), the good jobs run."""
    lib = hip_lib
    images = [cropref.synthetic_image(7, 70, 90), cropref.synthetic_image(8, 40, 30)]
    keep, srcs = _sources(cuda, images)
    OH, OW = 8, 8
    jobs = [(0, (3, 2, 36, 50), 0), (0, (5, 5, 5, 9), 0), (1, (-4, -4, 20, 30), 1), (2, (0, 0, 8, 8), 0), (1, (0, 0, 30, 40), 0),
            (0, (0, 0, 129, 64), 0), (0, (10, 10, 74, 60), 1)]
    want_status = [0, DH_EINVAL, 0, DH_EINVAL, 0, DH_EUNSUPPORTED, 0]
    buf, status, cap = build_dev(lib, cuda, srcs, jobs, OH, OW)
    assert status.tolist() == want_status
    prog = buf.cpu().numpy()
    nbytes = int(prog[28:32].view(np.uint32)[0])
    # the good jobs alone make a program of exactly the same size: a refused job takes a record and no table bytes
    good = [j for j, s in zip(jobs, want_status) if s == 0]
    assert nbytes == build_host(lib, srcs, good, OH, OW).size + 48 * 3
    assert np.all(prog[nbytes:] == 0xCD)
    item = OH * OW * 3
    pitch = item + GUARD
    out = torch.full((GUARD + len(jobs) * pitch,), 0xEE, dtype=torch.uint8, device=cuda)
    assert lib.dh_crop_resize_u8(buf.data_ptr(), len(jobs), OH, OW, out.data_ptr() + GUARD, pitch,
                                 torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.all(host[:GUARD] == 0xEE)
    body = host[GUARD:].reshape(len(jobs), pitch)
    assert np.all(body[:, item:] == 0xEE), 'guard bytes behind an item were overwritten'
    for j, ((s, box, flip), code) in enumerate(zip(jobs, want_status)):
        if code == 0:
            assert np.array_equal(body[j, :item].reshape(OH, OW, 3), cropref.crop_resize(images[s], box, (OH, OW), bool(flip))), j
        else:
            assert np.all(body[j, :item] == 0xEE), ('a refused job wrote its item', j)


# ---- the op ----------------------------------------------------------------------------------------------------------------
def _op(cuda, shapes, jobs, OH, OW, pitches=None, seed=0, guard=GUARD):
    """functional.crop_resize(program='device') into a sentinel-filled buffer, against cropref."""
    from deephar_amd import functional as F
    images = [cropref.synthetic_image(seed + i, h, w) for i, (h, w) in enumerate(shapes)]
    srcs = []
    for i, im in enumerate(images):
        H, W = im.shape[:2]
        pitch = pitches[i] if pitches else 3 * W
        wide = np.full((H, pitch), 0xAB, np.uint8)
        wide[:, :3 * W] = im.reshape(H, 3 * W)
        srcs.append(torch.as_strided(torch.from_numpy(wide).to(cuda), (H, W, 3), (pitch, 3, 1)))
    item = OH * OW * 3
    pitch_out = item + guard
    buf = torch.full((guard + len(jobs) * pitch_out,), 0xCD, dtype=torch.uint8, device=cuda)
    F.crop_resize(srcs, jobs, (OH, OW), out=buf[guard:], item_pitch=pitch_out, program='device')
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:guard] == 0xCD)
    body = host[guard:].reshape(len(jobs), pitch_out)
    assert np.all(body[:, item:] == 0xCD)
    for j, (s, box, flip) in enumerate(jobs):
        assert np.array_equal(body[j, :item].reshape(OH, OW, 3), cropref.crop_resize(images[s], box, (OH, OW), bool(flip))), j


@pytest.mark.parametrize('name', ['three_sources_five_jobs', 'flip_on_and_off'])
def test_crop_resize_program_device_equals_cropref(name, cuda, hip_lib):
    shapes, jobs, OH, OW, pitches = OP_CASES[name]
    _op(cuda, shapes, jobs, OH, OW, pitches, seed=sum(map(ord, name)))


def test_crop_resize_program_device_misaligned_destination(cuda, hip_lib):
    _op(cuda, [(37, 53)], [(0, (3, 2, 36, 50), 0), (0, (10, 10, 30, 31), 1)], 16, 16, seed=5, guard=7)


def test_crop_resize_program_device_refuses_like_the_host_path(cuda, hip_lib):
    from deephar_amd import functional as F
    src = torch.zeros((70, 70, 3), dtype=torch.uint8, device=cuda)
    out = torch.full((4 * 4 * 3,), 0xCD, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        F.crop_resize([src], [(0, (0, 0, 65, 64), 0)], (4, 4), out=out, item_pitch=48, program='device')
    with pytest.raises(ValueError):
        F.crop_resize([src], [(0, (5, 5, 5, 9), 0)], (4, 4), out=out, item_pitch=48, program='device')
    with pytest.raises(ValueError):
        F.crop_resize([src], [(0, (0, 0, 8, 8), 0)], (4, 4), program='gpu')
    torch.cuda.synchronize()
    assert bool((out == 0xCD).all())


# ---- whole models ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_model(cuda, hip_lib):
    from test_gpu_models import _build
    model, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)
    return model


@pytest.fixture(scope='module')
def six_frames(small_model):
    """images, boxes, flips and predict_from_frames(program='host') of them at batch 4 (4 + a ragged 2): computed once"""
    from deephar_amd import frontend
    images, boxes, flips = _frames_and_boxes(6, 3)
    ref = frontend.predict_from_frames(small_model, images, np.arange(6), boxes, hflip=flips, batch_size=4)
    for r in ref:
        r.setflags(write=False)
    return images, boxes, flips, ref


@pytest.mark.parametrize('streams', [1, 2])
def test_predict_from_frames_program_device_equals_host(streams, cuda, hip_lib, small_model, six_frames):
    from test_gpu_models import _build
    from deephar_amd import frontend
    images, boxes, flips, ref = six_frames
    model = small_model
    if streams > 1:
        model, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)      # the same synthetic weights
        model.num_streams = streams
    got = frontend.predict_from_frames(model, images, np.arange(6), boxes, hflip=flips, batch_size=4, program='device')
    assert len(got) == len(ref)
    for g, w in zip(got, ref):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    # a store uploaded once, frames shared between jobs, both programs
    store = frontend.FrameStore(images, cuda)
    idx = np.array([5, 0, 0, 3])
    a = frontend.predict_from_frames(model, store, idx, boxes[:4], batch_size=4, program='host')
    b = frontend.predict_from_frames(model, store, idx, boxes[:4], batch_size=4, program='device')
    for g, w in zip(b, a):
        assert np.array_equal(g, w)
    with pytest.raises(ValueError):                                            # beyond the scale cap: refused before anything runs
        big = [np.zeros((16, 5000, 3), np.uint8)]
        frontend.predict_from_frames(model, big, np.array([0]), np.array([[0, 0, 4200, 10]]), program='device')
    with pytest.raises(ValueError):
        frontend.predict_from_frames(model, store, idx, boxes[:4], program='both')


def test_predict_from_frames_program_device_clip_model(cuda, hip_lib):
    from test_gpu_models import _merge
    from deephar_amd import frontend
    model, _ = _merge(2, 4, 16, 2, num_actions=15)                              # input [T = 4, 256, 256, 3]
    images, boxes, _ = _frames_and_boxes(8, 7)
    index = np.arange(8).reshape(2, 4)
    want = frontend.predict_from_frames(model, images, index, boxes[:2], batch_size=2)
    got = frontend.predict_from_frames(model, images, index, boxes[:2], batch_size=2, program='device')
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_refine_pred_frames_program_device_equals_host(cuda, hip_lib, small_model):
    from deephar_amd.evaltools import mpii_tools
    images, boxes, _ = _frames_and_boxes(6, 11)
    want = mpii_tools.refine_pred_frames(small_model, images, boxes.astype(np.float64), 2, num_iter=2, batch_size=4)
    got = mpii_tools.refine_pred_frames(small_model, images, boxes.astype(np.float64), 2, num_iter=2, batch_size=4, program='device')
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def _frames_handle(lib, images):
    from deephar_amd import _lib
    table = (_lib.CropSrc * len(images))(*[_lib.CropSrc(im.ctypes.data, 3 * im.shape[1], im.shape[0], im.shape[1]) for im in images])
    h = C.c_void_p()
    assert lib.dh_frames_create(table, len(images), C.byref(h)) == 0
    assert lib.dh_frames_count(h) == len(images) and lib.dh_frames_table_dev(h)
    return h


@pytest.mark.parametrize('streams', [1, 2])
def test_dh_forward_frames_equals_predict_from_frames(streams, cuda, hip_lib, small_model, six_frames, tmp_path):
    from test_gpu_models import _build
    lib = hip_lib
    images, boxes, flips, ref = six_frames
    images = [np.ascontiguousarray(im) for im in images]
    model = small_model
    if streams > 1:
        model, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)
        model.num_streams, model.stream_policy = streams, 'list'
        model.executor.tune_table = small_model.executor.tune_table             # (tilings never move a bit; this spares the timing)
    path = str(tmp_path / 'm_u8.dhplan')
    model.export_plan(path, 4, uint8=True, multi_stream=streams > 1)
    blob = open(path, 'rb').read()
    plan = C.c_void_p()
    assert lib.dh_plan_create(blob, len(blob), C.byref(plan)) == 0
    frames = _frames_handle(lib, images)
    try:
        assert lib.dh_plan_num_streams(plan) == streams and lib.dh_plan_input_is_u8(plan, 0) == 1
        jobs = [(i, boxes[i], flips[i]) for i in range(6)]
        jd = _upload(cuda, _job_table(jobs))
        st = torch.cuda.current_stream().cuda_stream
        for start, m in [(0, 4), (4, 2)]:                                        # m = batch, then a ragged m
            outs = [torch.full((m,) + r.shape[1:], float('nan'), device=cuda) for r in ref[:-1]]
            outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            assert lib.dh_forward_frames(plan, frames, jd.data_ptr() + 24 * start, m, 256, 256, outs_p, st) == 0
            torch.cuda.synchronize()
            for k, (o, r) in enumerate(zip(outs, ref[:-1])):
                assert np.array_equal(o.cpu().numpy(), r[start:start + m]), ('device pointers', start, k)
            host = [np.full((m,) + r.shape[1:], np.nan, np.float32) for r in ref[:-1]]
            outs_h = (C.c_void_p * len(host))(*[h.ctypes.data for h in host])
            assert lib.dh_forward_frames_host(plan, frames, _job_table(jobs[start:start + m]), m, 256, 256, outs_h) == 0
            for k, (h, r) in enumerate(zip(host, ref[:-1])):
                assert np.array_equal(h, r[start:start + m]), ('host pointers', start, k)
        # refusals on a real plan: a job count above the batch, a crop size the input is no stack of, a bad table (host form)
        assert lib.dh_forward_frames(plan, frames, jd.data_ptr(), 5, 256, 256, outs_p, st) == DH_EINVAL
        assert lib.dh_forward_frames(plan, frames, jd.data_ptr(), 4, 256, 255, outs_p, st) == DH_EINVAL
        assert lib.dh_forward_frames(plan, frames, None, 4, 256, 256, outs_p, st) == DH_EINVAL
        bad = _job_table([(0, (0, 0, 256 * 16 + 1, 300), 0), (9, (0, 0, 30, 30), 0)])
        assert lib.dh_forward_frames_host(plan, frames, bad, 1, 256, 256, outs_h) == DH_EUNSUPPORTED
        assert lib.dh_forward_frames_host(plan, frames, _job_table([(9, (0, 0, 30, 30), 0)]), 1, 256, 256, outs_h) == DH_EINVAL
        if streams == 1:                                                         # a plan with a float input says so
            model.export_plan(path, 4)
            fblob = open(path, 'rb').read()
            fplan = C.c_void_p()
            assert lib.dh_plan_create(fblob, len(fblob), C.byref(fplan)) == 0
            assert lib.dh_forward_frames(fplan, frames, jd.data_ptr(), 4, 256, 256, outs_p, st) == DH_EINVAL
            assert lib.dh_plan_destroy(fplan) == 0
    finally:
        torch.cuda.synchronize()
        assert lib.dh_plan_destroy(plan) == 0
        assert lib.dh_frames_destroy(frames) == 0


def test_pure_c_host_predicts_from_frames(hip_lib, cuda, small_model, six_frames, tmp_path):
    """gcc-compiled host (no Python, no HIP headers): plan file + raw frames + job table in, raw outputs out, equal bits."""
    images, boxes, flips, ref = six_frames
    small_model.export_plan(str(tmp_path / 'm.dhplan'), 4, uint8=True)
    np.stack(images).tofile(str(tmp_path / 'frames.u8'))
    H, W = images[0].shape[:2]
    table = np.array([[i] + [int(v) for v in boxes[i]] + [int(flips[i])] for i in range(4)], np.int32)
    table.tofile(str(tmp_path / 'jobs.i32'))
    exe = str(tmp_path / 'predict_frames')
    libdir = os.path.join(ROOT, 'deephar_amd', 'csrc')
    r = subprocess.run(['gcc', '-O2', '-I' + os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tools', 'c_host', 'predict_frames.c'), '-L' + libdir, '-ldeephar_hip',
                        '-Wl,-rpath,' + libdir, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / 'm.dhplan'), str(tmp_path / 'frames.u8'), str(H), str(W), str(tmp_path / 'jobs.i32'),
                        '256', '256', str(tmp_path / 'out')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    for k, want in enumerate(ref[:-1]):
        got = np.fromfile(str(tmp_path / ('out.%d.f32' % k)), np.float32).reshape(want[:4].shape)
        assert np.array_equal(got, want[:4]), k
