"""The person-box index module (csrc/posebox_index.h) through its host twin, without a GPU: dh_pose_boxes_host against the Python
chain evaltools.bbox.get_bbox_from_poses over frontend.crop_afmat, against a long-hand numpy restatement bit for bit, every
status on a hand-made case, strided views, every refusal, dh_frame_boxes_shape, the C-ABI surface, and tools/posebox_sweep.cpp
built plainly and run."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseboxcases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DH_EINVAL = -1
FAKE = 0x10000                                            # a non-NULL, 8-byte aligned address no refusal may touch
NEAR = 1e-9                                               # an item may sit out the integer comparison only this near an integer
# float64 boxes against the Python chain: measured on the CPU 4.55e-13 px for F = 1 and for F = 3 (default_rng(1)); a factor 4
# over that, because np.linalg.inv goes through LAPACK and its last bits may differ between builds
BOUND = 4 * 4.55e-13


@pytest.mark.parametrize('F', [1, 3])
def test_host_twin_equals_python_chain(hip_lib, F):
    """4096 random items.  Measured here with default_rng(1): F = 1: 4073 items compared, F = 3: 4036 (the others have a frame
    that keeps no joint); none within 1e-9 of an integer; every integer box equal; float boxes within 4.55e-13 px."""
    rng = np.random.default_rng(1)
    items, windows = pc.random_items(rng, 4096, F)
    compared = near = 0
    worst = 0.0
    for item, w in zip(items, windows):
        want = pc.python_chain(item, w)
        box, boxf, status = pc.host_pose_boxes(hip_lib, item[None], pc.job_rows(0, w[None]))
        if want is None:                                  # get_valid_bbox raised: the twin says so too
            assert status[0] == pc.NO_JOINT
            continue
        assert status[0] == pc.OK
        worst = max(worst, float(np.abs(want - boxf[0]).max()))
        if np.abs(want - np.round(want)).min() < NEAR:
            near += 1
            continue
        compared += 1
        assert np.array_equal(want.astype(int), box[0]), (want, box[0])
    print('F = %d: %d items compared, %d near an integer, float boxes within %.3e px' % (F, compared, near, worst))
    assert near == 0 and compared > 3900
    assert worst <= BOUND


def test_host_twin_equals_longhand_bit_for_bit(hip_lib):
    """the numpy restatement of the header: J = 1, J = 65, D = 2 (confidence channel 0), a relsize float32 does not hold"""
    rng = np.random.default_rng(2)
    seen = set()
    for F, J, D, relsize in [(1, 1, 3, 1.5), (1, 65, 4, 1.2), (3, 17, 2, 1.2), (2, 16, 2, 1.5), (4, 20, 3, 1.2), (1, 2, 2, 0.1)]:
        n = 64
        p = rng.uniform(0.0, 1.0, (n, F, J, D))
        p[..., 0:2] = rng.uniform(-0.2, 1.2, (n, F, J, 2))
        p = p.astype(np.float32)
        windows = pc.random_windows(rng, n)
        box, boxf, status = pc.host_pose_boxes(hip_lib, p, pc.job_rows(np.arange(n), windows), relsize)
        for i in range(n):
            wb, wf, ws = pc.longhand(p[i], windows[i], relsize)
            assert status[i] == ws, (F, J, D, i)
            assert np.array_equal(boxf[i], wf) and np.array_equal(boxf[i].view(np.uint64), wf.view(np.uint64)), (F, J, D, i)
            assert np.array_equal(box[i], wb), (F, J, D, i)
            seen.add(int(ws))
    assert seen == {pc.OK, pc.NO_JOINT}


@pytest.mark.parametrize('case', pc.edge_cases(), ids=lambda c: c[0])
def test_edge_cases(hip_lib, case):
    box, boxf, status = pc.host_pose_boxes(hip_lib, case[1], case[2], case[3])
    pc.check_case(case, box, boxf, status)


def test_every_status_is_pinned(hip_lib):
    got = set()
    for case in pc.edge_cases():
        got.update(pc.host_pose_boxes(hip_lib, case[1], case[2], case[3])[2].tolist())
    assert got == {pc.OK, pc.NO_JOINT, pc.NAN_JOINT, pc.RANGE, pc.WINDOW}


def test_strides_channel_offset_and_job_stride(hip_lib):
    """poses read in place from a wider buffer; the item's window read from a job table of job_stride jobs per item"""
    rng = np.random.default_rng(3)
    for n, F, J, D, pj, pf, coff in [(3, 1, 16, 3, 0, 0, 0), (5, 3, 17, 3, 1, 0, 1), (2, 2, 65, 4, 2, 9, 2), (4, 1, 1, 2, 0, 5, 3)]:
        flat, off, strides, dense = pc.strided_items(rng, n, F, J, D, pj, pf, coff)
        windows = pc.random_windows(rng, n)
        want = pc.host_pose_boxes(hip_lib, dense, pc.job_rows(0, windows), 1.5)
        got = pc.host_pose_boxes(hip_lib, flat[off:], pc.job_rows(0, windows), 1.5, D - 2, strides, F, J, 1, n)
        table = np.full((n, 3, 6), 7, np.int32)                             # three jobs per item: the first one is the item's
        table[:, 0] = pc.job_rows(0, windows)
        wide = pc.host_pose_boxes(hip_lib, flat[off:], table, 1.5, D - 2, strides, F, J, 3, n)
        for g in (got, wide):
            assert np.array_equal(g[0], want[0]) and np.array_equal(g[1].view(np.uint64), want[1].view(np.uint64))
            assert np.array_equal(g[2], want[2])


def test_refusals(hip_lib):
    lib = hip_lib

    def boxes(poses=FAKE, its=96, fs=48, js=3, F=2, J=16, cc=1, jobs=FAKE, jstride=2, n=2, box=FAKE, boxf=FAKE, status=FAKE):
        a = (poses, its, fs, js, F, J, cc, jobs, jstride, n, 1.5, box, boxf, status)
        host, dev = lib.dh_pose_boxes_host(*a), lib.dh_pose_boxes_f64(*a, None)
        assert host == dev                                                   # refused before anything is read or enqueued
        return host

    big = (1 << 40) + 1
    for kw in [dict(poses=None), dict(jobs=None), dict(box=None), dict(boxf=None), dict(status=None), dict(n=0), dict(n=-3),
               dict(F=0), dict(F=-1), dict(J=0), dict(J=-2), dict(cc=-1), dict(jstride=0), dict(jstride=-1), dict(jstride=big),
               dict(js=1), dict(js=0), dict(js=-3), dict(cc=3),             # (channel 3 does not lie within a joint stride of 3)
               dict(fs=46), dict(fs=-48), dict(J=17),                       # (16 joints of stride 3 span 47 floats)
               dict(its=94), dict(its=-96), dict(F=3),                      # (2 frames of stride 48 span 95 floats)
               dict(F=1, its=46), dict(F=1, its=2), dict(F=1, its=10),      # (one frame spans 47 floats: no division hides it)
               dict(js=big, fs=big, its=big), dict(fs=big, its=big), dict(its=big),
               dict(n=0x7fffffff, its=1 << 40), dict(n=0x7fffffff, jstride=1 << 40)]:   # (n - 1) * stride above 2^58
        assert boxes(**kw) == DH_EINVAL, kw
    a = (48, 48, 3, 1, 16, 1, FAKE, 1, 2, 1.5)
    assert lib.dh_pose_boxes_f64(FAKE + 2, *a, FAKE, FAKE, FAKE, None) == DH_EINVAL       # misaligned poses
    assert lib.dh_pose_boxes_f64(FAKE, *a, FAKE, FAKE + 4, FAKE, None) == DH_EINVAL       # misaligned float64 boxes
    assert lib.dh_pose_boxes_f64(FAKE, *a, FAKE + 1, FAKE, FAKE, None) == DH_EINVAL       # misaligned int32 boxes


def test_frame_boxes_shape(hip_lib):
    lib = hip_lib
    J = C.c_int(0)
    good = dict(num_inputs=1, u8=1, items=256 * 256 * 3, batch=4, n=4, OH=256, OW=256, nout=3, outidx=2, out_items=48, ch=3)

    def shape(**kw):
        a = dict(good, **kw)
        return lib.dh_frame_boxes_shape(a['num_inputs'], a['u8'], a['items'], a['batch'], a['n'], a['OH'], a['OW'], a['nout'],
                                        a['outidx'], a['out_items'], a['ch'], C.byref(J))

    assert shape() == 0 and J.value == 16
    assert shape(n=1) == 0 and shape(ch=2, out_items=32) == 0 and shape(outidx=0) == 0
    for kw in [dict(num_inputs=2), dict(u8=0), dict(items=4 * 256 * 256 * 3), dict(items=256 * 256 * 3 - 1), dict(n=5), dict(n=0),
               dict(outidx=3), dict(outidx=-1), dict(ch=1, out_items=16), dict(ch=0), dict(OW=255), dict(OH=0), dict(out_items=47),
               dict(batch=0)]:
        assert shape(**kw) == DH_EINVAL, kw
    assert lib.dh_frame_boxes_host(None, None, None, None, 1, 256, 256, 0, 1.5, None, None, None) == DH_EINVAL


def test_c_abi_lists_the_new_symbols(hip_lib):
    from deephar_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deephar_hip.h')).read()
    for name in ('dh_pose_boxes_f64', 'dh_pose_boxes_host', 'dh_frame_boxes_shape', 'dh_frame_boxes_host'):
        assert name in _lib.SIGNATURES and 'int %s(' % name in header, name
        assert getattr(hip_lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES['dh_pose_boxes_f64'][1]) == len(_lib.SIGNATURES['dh_pose_boxes_host'][1]) + 1     # the stream


def test_posebox_sweep_builds_and_passes(tmp_path):
    """tools/posebox_sweep.cpp, the stand-alone sweep of the header (its own main(), nothing loaded into Python), built plainly
    and run: items, statuses and refusals in heap blocks of exactly their length.  Its sanitizer build (the command in the
    file's head) is run by hand on a CPU host; this keeps the sweep compiling and passing."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'posebox_sweep')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'deephar_amd', 'csrc'),
                        os.path.join(ROOT, 'tools', 'posebox_sweep.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'posebox_sweep: ok' in r.stdout, r.stdout + r.stderr
