"""The box-refinement index module (csrc/refine_index.h) through its host twins, without a GPU: dh_refine_boxes_host against the
Python loop of evaltools.refine_pred_frames lifted out of the model, dh_jobs_from_boxes_host against frontend.crop_box, the edge
cases, every refusal, dh_refine_frames_shape, and tools/refine_sweep.cpp built with the host sanitizers and run."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refinecases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DH_EINVAL = -1
FAKE = 0x10000                                            # a non-NULL, 8-byte aligned address no refusal may touch


def test_host_twin_equals_python_loop(hip_lib):
    """4096 samples, J = 16, three refinement steps (four window tables).  Every integer window equal; float boxes within
    1e-9 px of the loop's, which go through np.linalg.inv and einsum.  Measured here: the twin's boxes differ from the
    loop's by at most 4.55e-13 px; the nearest pre-truncation corner lies 8.49e-06 from an integer; the largest window is
    4.47 x 256."""
    bbox0, poses = rc.synthetic()
    windows, boxes, corners = rc.python_loop(bbox0, poses)
    dist, scale = rc.preconditions(windows, corners)
    n = len(bbox0)
    src = np.arange(n, dtype=np.int32)
    jobs = rc.host_jobs_from_boxes(hip_lib, bbox0, src)
    assert np.array_equal(jobs[:, 1:5], windows[0]) and np.array_equal(jobs[:, 0], src) and not jobs[:, 5].any()
    cur, worst = bbox0.copy(), 0.0
    for t in range(len(poses)):
        cur, jobs = rc.host_refine(hip_lib, poses[t], jobs, cur)
        worst = max(worst, float(np.abs(cur - boxes[t + 1]).max()))
        assert np.array_equal(jobs[:, 1:5], windows[t + 1]), ('windows of iteration', t + 1)
        assert np.array_equal(jobs[:, 0], src) and not jobs[:, 5].any()
    print('twin vs loop: %.3e px; nearest corner to an integer %.3e; largest scale %.2f' % (worst, dist, scale))
    assert worst <= 1e-9


def test_jobs_from_boxes_equals_crop_box(hip_lib):
    from deephar_amd import frontend
    from deephar_amd.utils import bbox_to_objposwin
    rng = np.random.RandomState(1)
    boxes = np.concatenate([rng.uniform(-900.0, 1500.0, (500, 4)),                        # negative corners, reversed boxes too
                            np.array([[-0.5, -0.75, 0.5, 0.75], [-10.99, -3.01, -2.5, -1.2], [0.0, 0.0, 256.0, 256.0],
                                      [-1e-9, 5.9999999, 7.0000001, 9.5]])])
    src = np.arange(len(boxes), dtype=np.int32)[::-1].copy()
    jobs = rc.host_jobs_from_boxes(hip_lib, boxes, src)
    want = np.stack([frontend.crop_box(*bbox_to_objposwin(b)) for b in boxes])
    assert (want < 0).any() and np.array_equal(jobs[:, 1:5], want)
    assert np.array_equal(jobs[:, 0], src) and not jobs[:, 5].any()
    # corners that do not fit int32, or are not finite: the empty job
    bad = np.array([[0, 0, 3e9, 10], [-3e9, 0, 5, 10], [0, 0, np.nan, 10], [0, -np.inf, 5, 10], [0, 0, 2147483648.0, 10]])
    jobs = rc.host_jobs_from_boxes(hip_lib, bad, np.arange(5))
    assert np.array_equal(jobs, rc.job_rows(np.arange(5), np.zeros((5, 4), int)))


@pytest.mark.parametrize('case', rc.edge_cases(), ids=lambda c: c[0])
def test_edge_cases(hip_lib, case):
    name, poses, jobs, boxes, expect = case
    nb, nj = rc.host_refine(hip_lib, poses, jobs, boxes)
    rc.check_expectation(name, expect, jobs, boxes, nb, nj)
    ib, ij = rc.host_refine(hip_lib, poses, jobs, boxes, inplace=True)                    # aliased in / out pointers
    assert np.array_equal(ib.view(np.uint64), nb.view(np.uint64)) and np.array_equal(ij, nj)


def test_strides_and_channel_offset(hip_lib):
    """poses read in place from a wider buffer: joint stride above D, sample stride above J joints, a channel offset"""
    rng = np.random.RandomState(2)
    for n, J, D, pj, ps, coff in [(3, 16, 3, 0, 0, 0), (5, 17, 2, 3, 11, 5), (1, 65, 4, 1, 7, 2), (4, 1, 2, 0, 0, 1)]:
        flat, off, ss, js, dense = rc.strided_poses(rng, n, J, D, pj, ps, coff)
        boxes = np.repeat(np.array([[30.25, 40.5, 330.25, 300.5]]), n, axis=0)
        jobs = rc.host_jobs_from_boxes(hip_lib, boxes, np.arange(n))
        want_b, want_j = rc.host_refine(hip_lib, dense, jobs, boxes)
        got_b, got_j = rc.host_refine(hip_lib, flat[off:], jobs, boxes, sample_stride=ss, joint_stride=js, J=J)
        assert np.array_equal(got_b.view(np.uint64), want_b.view(np.uint64)) and np.array_equal(got_j, want_j)


def test_refusals(hip_lib):
    lib = hip_lib
    for args in [(None, FAKE, 2, FAKE), (FAKE, None, 2, FAKE), (FAKE, FAKE, 2, None), (FAKE, FAKE, 0, FAKE), (FAKE, FAKE, -1, FAKE)]:
        assert lib.dh_jobs_from_boxes_host(*args) == DH_EINVAL
        assert lib.dh_jobs_from_boxes_f64(*args, None) == DH_EINVAL                      # refused before anything is enqueued

    def refine(poses=FAKE, ss=48, js=3, J=16, jin=FAKE, bin_=FAKE, n=2, bout=FAKE, jout=FAKE):
        a = (poses, ss, js, J, jin, bin_, n, 1.5, 0.8, bout, jout)
        host, dev = lib.dh_refine_boxes_host(*a), lib.dh_refine_boxes_f64(*a, None)
        assert host == dev
        return host

    for kw in [dict(poses=None), dict(jin=None), dict(bin_=None), dict(bout=None), dict(jout=None), dict(n=0), dict(n=-3), dict(J=0),
               dict(js=1), dict(js=0), dict(ss=46), dict(ss=-48), dict(J=17)]:            # (16 joints of stride 3 span 47 floats)
        assert refine(**kw) == DH_EINVAL, kw
    assert lib.dh_refine_boxes_f64(FAKE + 2, 48, 3, 16, FAKE, FAKE, 2, 1.5, 0.8, FAKE, FAKE, None) == DH_EINVAL   # misaligned poses
    assert lib.dh_refine_boxes_f64(FAKE, 48, 3, 16, FAKE, FAKE + 4, 2, 1.5, 0.8, FAKE, FAKE, None) == DH_EINVAL   # misaligned boxes


def test_refine_frames_shape(hip_lib):
    lib = hip_lib
    J = C.c_int(0)
    good = dict(num_inputs=1, u8=1, items=256 * 256 * 3, batch=4, n=4, OH=256, OW=256, nout=3, outidx=2, out_items=48, ch=3, it=2)

    def shape(**kw):
        a = dict(good, **kw)
        return lib.dh_refine_frames_shape(a['num_inputs'], a['u8'], a['items'], a['batch'], a['n'], a['OH'], a['OW'], a['nout'],
                                          a['outidx'], a['out_items'], a['ch'], a['it'], C.byref(J))

    assert shape() == 0 and J.value == 16
    assert shape(n=1) == 0 and shape(it=1) == 0 and shape(ch=2, out_items=32) == 0
    for kw in [dict(num_inputs=2), dict(u8=0), dict(items=4 * 256 * 256 * 3), dict(items=256 * 256 * 3 - 1), dict(n=5), dict(n=0),
               dict(outidx=3), dict(outidx=-1), dict(ch=1, out_items=16), dict(ch=0), dict(it=0), dict(OW=255), dict(OH=0),
               dict(out_items=47), dict(batch=0)]:
        assert shape(**kw) == DH_EINVAL, kw
    assert lib.dh_refine_frames_host(None, None, None, None, 1, 256, 256, 0, 2, 1.5, 0.8, None, None, None) == DH_EINVAL


def test_refine_sweep_builds_and_passes(tmp_path):
    """tools/refine_sweep.cpp, the stand-alone sweep of the header (its own main(), nothing loaded into Python), built plainly
    and run: windows, steps and refusals in heap blocks of exactly their length.  Its sanitizer build (the command in the
    file's head) is run by hand on a CPU host; this keeps the sweep compiling and passing."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'refine_sweep')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'deephar_amd', 'csrc'),
                        os.path.join(ROOT, 'tools', 'refine_sweep.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'refine_sweep: ok' in r.stdout, r.stdout + r.stderr
