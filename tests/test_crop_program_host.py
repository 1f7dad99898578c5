"""The device crop-program builder and the frames C-ABI, as far as they go without a GPU: the capacity query against the size
query, every refusal that is answered on the host before anything is enqueued, the GPU-free shape test dh_forward_frames runs,
and what frontend.CropFeed stages per chunk under program='device'."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_crop_host import SWEEP  # noqa: E402

DH_EINVAL, DH_EUNSUPPORTED = -1, -2
FAKE = 0x10000                                            # a non-NULL, 8-byte aligned address no refusal may touch


def _jobs(jobs):
    from deephar_amd import _lib
    return (_lib.CropJob * len(jobs))(*[_lib.CropJob(s, b[0], b[1], b[2], b[3], int(f)) for s, b, f in jobs])


def _max_bytes(lib, njobs, nsrc, OH, OW):
    n = C.c_size_t(0)
    rc = lib.dh_crop_program_max_bytes(njobs, nsrc, OH, OW, C.byref(n))
    return rc, n.value


def _bytes(lib, jobs, nsrc, OH, OW):
    n = C.c_size_t(0)
    rc = lib.dh_crop_program_bytes(_jobs(jobs), len(jobs), nsrc, OH, OW, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize('case', range(len(SWEEP)))
def test_capacity_covers_every_sweep_table(hip_lib, case):
    shapes, jobs, OH, OW, _ = SWEEP[case]
    rc, exact = _bytes(hip_lib, jobs, len(shapes), OH, OW)
    assert rc == 0
    rc, cap = _max_bytes(hip_lib, len(jobs), len(shapes), OH, OW)
    assert rc == 0 and cap >= exact and cap % 8 == 0
    # header + sources + records + per job both tables at 33 taps, rounded to 8 bytes per table
    tab = lambda out: (out * (2 + 33) * 4 + 7) & ~7
    assert cap == 32 + 24 * len(shapes) + len(jobs) * (48 + tab(OW) + tab(OH))


def test_capacity_is_exact_at_the_scale_cap(hip_lib):
    """Every job at scale exactly 16 on both axes has 33 taps: the capacity is the program, to the byte."""
    jobs = [(0, (0, 0, 64, 64), 0), (0, (-8, 8, 56, 72), 1), (0, (3, 3, 83, 115), 0)]
    for OH, OW, js in [(4, 4, jobs[:2]), (7, 5, jobs[2:])]:
        rc, exact = _bytes(hip_lib, js, 1, OH, OW)
        assert rc == 0
        assert _max_bytes(hip_lib, len(js), 1, OH, OW) == (0, exact)


def test_capacity_refusals(hip_lib):
    lib = hip_lib
    n = C.c_size_t(0)
    assert lib.dh_crop_program_max_bytes(1, 1, 8, 8, None) == DH_EINVAL
    for args in [(0, 1, 8, 8), (-3, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (1, 1, (1 << 20) + 1, 8), (1, 1, 8, (1 << 20) + 1)]:
        assert lib.dh_crop_program_max_bytes(*args, C.byref(n)) == DH_EINVAL, args
    assert n.value == 0
    assert lib.dh_crop_program_max_bytes(1 << 20, 1, 256, 256, C.byref(n)) == DH_EUNSUPPORTED          # above 2^31 - 1 bytes
    assert lib.dh_crop_program_max_bytes(64, 8, 256, 256, C.byref(n)) == 0 and n.value == 32 + 8 * 24 + 64 * (48 + 2 * 35840)


def test_device_builder_refuses_on_the_host(hip_lib):
    """Nothing here reaches a device: the pointers are made up, and every call is refused before a launch."""
    build = hip_lib.dh_crop_program_build_dev
    rc, cap = _max_bytes(hip_lib, 3, 2, 8, 8)
    assert rc == 0
    ok = dict(srcs=FAKE, nsrc=2, jobs=FAKE + 0x1000, njobs=3, OH=8, OW=8, prog=FAKE + 0x2000, cap=cap, status=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return build(a['srcs'], a['nsrc'], a['jobs'], a['njobs'], a['OH'], a['OW'], a['prog'], a['cap'], a['status'], a['stream'])

    assert call(cap=cap - 1) == DH_EINVAL                                        # one byte short
    assert call(cap=0) == DH_EINVAL
    assert call(prog=FAKE + 0x2004) == DH_EINVAL                                 # misaligned program
    assert call(prog=None) == DH_EINVAL
    assert call(srcs=None) == DH_EINVAL
    assert call(jobs=None) == DH_EINVAL
    assert call(srcs=FAKE + 4) == DH_EINVAL
    assert call(jobs=FAKE + 2) == DH_EINVAL
    assert call(status=FAKE + 0x3001) == DH_EINVAL
    assert call(njobs=0) == DH_EINVAL
    assert call(nsrc=0) == DH_EINVAL
    assert call(OH=0) == DH_EINVAL and call(OW=0) == DH_EINVAL
    assert call(OW=(1 << 20) + 1, cap=1 << 40) == DH_EINVAL
    # 33 rows of the output width must fit LDS: the pitch of OW = 661 is 1984 bytes (65 472), of OW = 662 it is 2000
    assert call(OW=662, cap=_max_bytes(hip_lib, 3, 2, 8, 662)[1]) == DH_EUNSUPPORTED
    assert call(OW=662, cap=_max_bytes(hip_lib, 3, 2, 8, 662)[1] - 1) == DH_EINVAL


def test_frames_and_forward_frames_refuse_on_the_host(hip_lib):
    from deephar_amd import _lib
    lib = hip_lib
    img = np.zeros((6, 7, 3), np.uint8)
    good = _lib.CropSrc(img.ctypes.data, 21, 6, 7)
    h = C.c_void_p()
    assert lib.dh_frames_create(None, 1, C.byref(h)) == DH_EINVAL
    assert lib.dh_frames_create((_lib.CropSrc * 1)(good), 1, None) == DH_EINVAL
    assert lib.dh_frames_create((_lib.CropSrc * 1)(good), 0, C.byref(h)) == DH_EINVAL
    for bad in [_lib.CropSrc(None, 21, 6, 7), _lib.CropSrc(img.ctypes.data, 20, 6, 7), _lib.CropSrc(img.ctypes.data, 21, 0, 7),
                _lib.CropSrc(img.ctypes.data, 21, 6, 0)]:
        assert lib.dh_frames_create((_lib.CropSrc * 2)(good, bad), 2, C.byref(h)) == DH_EINVAL
    assert h.value is None
    assert lib.dh_frames_destroy(None) == 0 and lib.dh_frames_count(None) == 0 and lib.dh_frames_table_dev(None) is None
    outs = (C.c_void_p * 1)(FAKE)
    job = _jobs([(0, (0, 0, 4, 4), 0)])
    assert lib.dh_forward_frames(None, FAKE, FAKE, 1, 4, 4, outs, None) == DH_EINVAL
    assert lib.dh_forward_frames_host(None, FAKE, job, 1, 4, 4, outs) == DH_EINVAL
    # what dh_forward_frames asks of its plan and of the job count (the same function, GPU-free)
    shape = lib.dh_forward_frames_shape
    m, per = C.c_int(-1), C.c_int(-1)
    item = 256 * 256 * 3
    assert shape(1, 1, item, 4, 4, 256, 256, C.byref(m), C.byref(per)) == 0 and (m.value, per.value) == (4, 1)
    assert shape(1, 1, item, 4, 3, 256, 256, C.byref(m), C.byref(per)) == 0 and (m.value, per.value) == (3, 1)      # a ragged m
    assert shape(1, 1, 4 * item, 2, 8, 256, 256, C.byref(m), C.byref(per)) == 0 and (m.value, per.value) == (2, 4)  # clips of 4
    assert shape(1, 1, 4 * item, 2, 4, 256, 256, C.byref(m), None) == 0 and m.value == 1
    assert shape(1, 0, item, 4, 4, 256, 256, C.byref(m), C.byref(per)) == DH_EINVAL        # a plan with a float input
    assert shape(2, 1, item, 4, 4, 256, 256, C.byref(m), C.byref(per)) == DH_EINVAL        # two inputs
    assert shape(1, 1, 4 * item, 2, 6, 256, 256, C.byref(m), C.byref(per)) == DH_EINVAL    # 6 jobs do not fill clips of 4
    assert shape(1, 1, item, 4, 5, 256, 256, C.byref(m), C.byref(per)) == DH_EINVAL        # more items than the plan holds
    assert shape(1, 1, item, 4, 0, 256, 256, C.byref(m), C.byref(per)) == DH_EINVAL
    assert shape(1, 1, item, 4, 4, 256, 255, C.byref(m), C.byref(per)) == DH_EINVAL        # the input is no stack of such crops
    assert shape(1, 1, item, 4, 4, 0, 256, C.byref(m), C.byref(per)) == DH_EINVAL


class _Store:
    """What CropFeed needs of a FrameStore, without a device."""

    def __init__(self, shapes):
        from deephar_amd import _lib
        self.srcs = (_lib.CropSrc * len(shapes))(*[_lib.CropSrc(FAKE, 3 * w, h, w) for h, w in shapes])
        self.n = len(shapes)

    def __len__(self):
        return self.n


def test_cropfeed_stages_24_bytes_per_job_under_program_device(hip_lib):
    import torch
    from deephar_amd import frontend
    store = _Store([(300, 340)] * 3)
    rng = np.random.default_rng(4)
    index = rng.integers(0, 3, (5, 4))                                           # 5 clips of 4 frames
    x0, y0 = rng.integers(-20, 200, (5, 4)), rng.integers(-20, 200, (5, 4))
    boxes = np.stack([x0, y0, x0 + rng.integers(1, 300, (5, 4)), y0 + rng.integers(1, 300, (5, 4))], axis=-1)
    flips = rng.integers(0, 2, (5, 4)).astype(bool)
    feed = frontend.CropFeed(store, index, boxes, flips, (64, 48), program='device')
    assert feed.program == 'device' and feed.per_item == 4
    for start, m in [(0, 2), (2, 2), (4, 1)]:
        out = torch.full((24 * 2 * 4 + 16,), 0xCD, dtype=torch.uint8)
        n = feed.stage(start, m, out)
        assert n == 24 * m * 4
        got = out.numpy()
        assert np.all(got[n:] == 0xCD)
        table = got[:n].view(np.int32).reshape(m * 4, 6)
        want = np.concatenate([index[start:start + m].reshape(-1, 1), boxes[start:start + m].reshape(-1, 4),
                               flips[start:start + m].reshape(-1, 1)], axis=1)
        assert np.array_equal(table, want)
        assert feed.max_bytes(m) == _max_bytes(hip_lib, m * 4, 3, 64, 48)[1] >= feed.program_bytes(start, m)
    with pytest.raises(ValueError):
        feed.stage(0, 2, torch.zeros(24 * 8 - 1, dtype=torch.uint8))
    with pytest.raises(ValueError):
        frontend.CropFeed(store, index, boxes, flips, (64, 48), program='gpu')
    assert frontend.CropFeed(store, index, boxes, flips, (64, 48)).program == 'host'
