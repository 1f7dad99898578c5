"""The crop-and-resize front end without a GPU: tests/cropref.py against the reference's own PIL path (fixtures) and against
PIL where it imports; the library's coefficient tables, crop program builder and host twin (csrc/crop_index.h) against
cropref, exactly; every refusal; refine_pred_frames against refine_pred."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'crop_reference.npz')
DH_EINVAL, DH_EUNSUPPORTED = -1, -2


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    cases = []
    for i in range(int(g['num_cases'])):
        H, W = [int(v) for v in g['shape_%d' % i]]
        cases.append(dict(img=cropref.synthetic_image(int(g['seed_%d' % i]), H, W), objpos=g['objpos_%d' % i],
                          winsize=g['winsize_%d' % i], size=tuple(int(v) for v in g['size_%d' % i]), hflip=int(g['hflip_%d' % i]),
                          frame=g['frame_%d' % i], afmat=g['afmat_%d' % i], box=g['box_%d' % i]))
    return str(g['pillow_version']), cases


def test_cropref_equals_the_reference_fixtures(golden):
    version, cases = golden
    assert version and len(cases) >= 12
    kinds = set()
    for c in cases:
        box = cropref.crop_box(c['objpos'], c['winsize'])
        assert np.array_equal(box, c['box'])
        OW, OH = c['size']
        got = cropref.crop_resize(c['img'], box, (OH, OW), hflip=bool(c['hflip']))
        assert got.dtype == np.uint8 and np.array_equal(got, c['frame'])
        assert np.array_equal(cropref.crop_afmat(box, c['size'], bool(c['hflip'])), c['afmat'])
        H, W = c['img'].shape[:2]
        cw, ch = box[2] - box[0], box[3] - box[1]
        kinds |= {'neg'} if box[0] < 0 or box[1] < 0 else set()
        kinds |= {'beyond'} if box[2] > W and box[3] > H else set()
        kinds |= {'nonsquare'} if cw != ch and c['winsize'][0] == c['winsize'][1] else set()
        kinds |= {'up'} if cw < OW and ch < OH else set()
        kinds |= {'down4'} if cw / OW > 4 and cw % OW else set()
        kinds |= {'flip%d' % c['hflip']}
    assert kinds == {'neg', 'beyond', 'nonsquare', 'up', 'down4', 'flip0', 'flip1'}


def test_cropref_equals_pil_on_random_cases():
    PIL = pytest.importorskip('PIL')
    from PIL import Image
    rng = np.random.default_rng(5)
    for _ in range(40):
        H, W = int(rng.integers(8, 120)), int(rng.integers(8, 120))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        x0, y0 = int(rng.integers(-20, W - 1)), int(rng.integers(-20, H - 1))
        x1, y1 = x0 + int(rng.integers(1, W + 20)), y0 + int(rng.integers(1, H + 20))
        OW, OH = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        want = np.asarray(Image.fromarray(img).crop((x0, y0, x1, y1)).resize((OW, OH), Image.BILINEAR))
        assert np.array_equal(cropref.crop_resize(img, (x0, y0, x1, y1), (OH, OW)), want), (PIL.__version__, H, W, x0, y0, x1, y1)


def _lib_coeffs(lib, n_in, n_out):
    taps = lib.dh_crop_axis_taps(n_in, n_out)
    first, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    k = np.full((n_out, taps), -7, np.int32)
    i32p = C.POINTER(C.c_int32)
    rc = lib.dh_crop_axis_coeffs_host(n_in, n_out, taps, first.ctypes.data_as(i32p), count.ctypes.data_as(i32p),
                                      k.ctypes.data_as(i32p))
    return rc, taps, first, count, k


def test_library_coefficient_tables_equal_cropref(hip_lib):
    checked = 0
    for n_out in (1, 3, 8, 32, 64, 256):
        for n_in in range(1, 701):                                            # (the scale cap of 16 belongs to the launch, not here)
            rc, taps, first, count, k = _lib_coeffs(hip_lib, n_in, n_out)
            assert rc == 0 and taps == cropref.axis_taps(n_in, n_out)
            rf, rcnt, rk = cropref.axis_coeffs(n_in, n_out)
            assert np.array_equal(first, rf) and np.array_equal(count, rcnt) and np.array_equal(k, rk), (n_in, n_out)
            checked += 1
    assert checked == 6 * 700
    i32p = C.POINTER(C.c_int32)
    buf = np.zeros(64, np.int32).ctypes.data_as(i32p)
    assert hip_lib.dh_crop_axis_coeffs_host(9, 3, 6, buf, buf, buf) == DH_EINVAL          # fewer taps than the axis needs
    assert hip_lib.dh_crop_axis_coeffs_host(0, 3, 7, buf, buf, buf) == DH_EINVAL
    assert hip_lib.dh_crop_axis_coeffs_host(9, 3, 7, None, buf, buf) == DH_EINVAL


# ---- crop programs ---------------------------------------------------------------------------------------------------------
def build_program(lib, images, jobs, OH, OW, pitches=None):
    """images: uint8 [H, W, 3] arrays; jobs: (src, (x0, y0, x1, y1), hflip) -> (rc, program bytes as np.uint8, keep-alive)."""
    from deephar_amd import _lib
    keep = []
    srcs = (_lib.CropSrc * len(images))()
    for i, im in enumerate(images):
        H, W = im.shape[:2]
        pitch = (pitches[i] if pitches else 3 * W)
        buf = np.full((H, pitch), 0xAB, np.uint8)
        buf[:, :3 * W] = im.reshape(H, 3 * W)
        keep.append(buf)
        srcs[i] = _lib.CropSrc(buf.ctypes.data, pitch, H, W)
    cj = (_lib.CropJob * len(jobs))(*[_lib.CropJob(s, b[0], b[1], b[2], b[3], int(f)) for s, b, f in jobs])
    nbytes = C.c_size_t(0)
    rc = lib.dh_crop_program_bytes(cj, len(jobs), len(images), OH, OW, C.byref(nbytes))
    if rc != 0:
        return rc, None, keep
    prog = np.zeros(nbytes.value // 8 + 1, np.uint64)                          # 8-byte aligned
    rc = lib.dh_crop_program_build_host(srcs, len(images), cj, len(jobs), OH, OW, prog.ctypes.data, nbytes.value)
    return rc, prog.view(np.uint8)[:nbytes.value], keep + [prog]


def run_host(lib, prog, njobs, OH, OW, pad=0):
    item = OH * OW * 3 + pad
    y = np.full(njobs * item + 64, 0xCD, np.uint8)
    rc = lib.dh_crop_resize_host(prog.ctypes.data, prog.size, njobs, OH, OW, y[32:].ctypes.data, item)
    assert np.all(y[:32] == 0xCD) and np.all(y[32 + njobs * item:] == 0xCD)
    body = y[32:32 + njobs * item].reshape(njobs, item)
    if rc == 0:
        assert np.all(body[:, OH * OW * 3:] == 0xCD)
    return rc, body[:, :OH * OW * 3].reshape(njobs, OH, OW, 3), body


def test_host_twin_equals_cropref_on_the_fixtures(hip_lib, golden):
    for c in golden[1]:
        OW, OH = c['size']
        rc, prog, keep = build_program(hip_lib, [c['img']], [(0, c['box'], c['hflip'])], OH, OW)
        assert rc == 0
        rc, out, _ = run_host(hip_lib, prog, 1, OH, OW)
        assert rc == 0 and np.array_equal(out[0], c['frame'])


SWEEP = [  # (image shapes, jobs, OH, OW, pitches)
    ([(20, 30)], [(0, (40, 5, 60, 15), 0), (0, (-30, -30, -2, -1), 1)], 8, 8, None),          # entirely outside: zeros
    ([(20, 30)], [(0, (7, 3, 8, 19), 0), (0, (29, -4, 30, 30), 1)], 8, 5, None),              # one pixel wide
    ([(40, 32)], [(0, (0, 3, 32, 33), 0), (0, (-5, 0, 27, 40), 1)], 16, 32, None),            # cw == OW: no horizontal pass
    ([(64, 64)], [(0, (0, 0, 64, 64), 0), (0, (-8, 8, 56, 72), 1)], 4, 4, None),              # scale exactly 16
    ([(37, 53)], [(0, (3, 2, 36, 50), 0)], 8, 8, [3 * 53 + 13]),                              # a row pitch above 3 W
    ([(37, 53)], [(0, (3, 2, 36, 50), 0), (0, (10, 10, 30, 31), 1)], 8, 8, None),             # two jobs on one source
    ([(16, 16), (37, 53), (9, 70)], [(2, (0, 0, 70, 9), 0), (0, (-2, -2, 18, 18), 1), (1, (0, 0, 53, 37), 0),
                                     (2, (60, 2, 90, 12), 1), (1, (5, 5, 6, 6), 0)], 12, 10, [48, 200, 211]),   # mixed sources
]


@pytest.mark.parametrize('case', range(len(SWEEP)))
def test_host_twin_equals_cropref_on_the_sweep(hip_lib, case):
    shapes, jobs, OH, OW, pitches = SWEEP[case]
    images = [cropref.synthetic_image(100 + case * 7 + i, h, w) for i, (h, w) in enumerate(shapes)]
    rc, prog, keep = build_program(hip_lib, images, jobs, OH, OW, pitches)
    assert rc == 0
    rc, out, _ = run_host(hip_lib, prog, len(jobs), OH, OW, pad=5)
    assert rc == 0
    for j, (s, box, flip) in enumerate(jobs):
        want = cropref.crop_resize(images[s], box, (OH, OW), bool(flip))
        assert np.array_equal(out[j], want), (case, j)
        H, W = images[s].shape[:2]
        if box[0] >= W or box[2] <= 0 or box[1] >= H or box[3] <= 0:
            assert not out[j].any()


def test_host_twin_random_sweep(hip_lib):
    rng = np.random.default_rng(11)
    for _ in range(30):
        H, W = int(rng.integers(4, 60)), int(rng.integers(4, 60))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        OH, OW = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        jobs = []
        for _ in range(3):
            cw, ch = int(rng.integers(1, min(16 * OW, W + 20) + 1)), int(rng.integers(1, min(16 * OH, H + 20) + 1))
            x0, y0 = int(rng.integers(-15, W)), int(rng.integers(-15, H))
            jobs.append((0, (x0, y0, x0 + cw, y0 + ch), int(rng.integers(0, 2))))
        rc, prog, keep = build_program(hip_lib, [img], jobs, OH, OW)
        assert rc == 0
        rc, out, _ = run_host(hip_lib, prog, 3, OH, OW)
        assert rc == 0
        for j, (s, box, flip) in enumerate(jobs):
            assert np.array_equal(out[j], cropref.crop_resize(img, box, (OH, OW), bool(flip))), (H, W, OH, OW, box, flip)


def test_refusals(hip_lib):
    from deephar_amd import _lib
    lib = hip_lib
    img = cropref.synthetic_image(3, 70, 70)
    # scale just above 16 on either axis: DH_EUNSUPPORTED from the size query and the builder, nothing written
    for box in [(0, 0, 65, 64), (0, 0, 64, 65)]:
        rc, prog, _ = build_program(lib, [img], [(0, box, 0)], 4, 4)
        assert rc == DH_EUNSUPPORTED and prog is None
    # ... and from the host twin when a program claims such a window: built at scale 16, then the job's x1 is patched
    rc, prog, keep = build_program(lib, [img], [(0, (0, 0, 64, 64), 0)], 4, 4)
    assert rc == 0
    bad = prog.copy()
    job_off = int(bad[24:28].view(np.uint32)[0])
    bad[job_off + 12:job_off + 16].view(np.int32)[0] = 65
    prog8 = np.zeros(bad.size // 8 + 1, np.uint64)
    prog8.view(np.uint8)[:bad.size] = bad
    rc, _, body = run_host(lib, prog8.view(np.uint8)[:bad.size], 1, 4, 4)
    assert rc == DH_EUNSUPPORTED and np.all(body == 0xCD)
    # builder: NULL pointers, empty boxes, pitch < 3 W, bad source index, short buffer
    srcbuf = np.ascontiguousarray(img)
    ok_src = (_lib.CropSrc * 1)(_lib.CropSrc(srcbuf.ctypes.data, 210, 70, 70))
    ok_job = (_lib.CropJob * 1)(_lib.CropJob(0, 0, 0, 32, 32, 0))
    n = C.c_size_t(0)
    assert lib.dh_crop_program_bytes(ok_job, 1, 1, 8, 8, C.byref(n)) == 0 and n.value > 0
    out = np.zeros(n.value // 8 + 1, np.uint64)
    assert lib.dh_crop_program_bytes(None, 1, 1, 8, 8, C.byref(n)) == DH_EINVAL
    assert lib.dh_crop_program_bytes(ok_job, 1, 1, 8, 8, None) == DH_EINVAL
    assert lib.dh_crop_program_bytes(ok_job, 0, 1, 8, 8, C.byref(n)) == DH_EINVAL
    assert lib.dh_crop_program_bytes(ok_job, 1, 1, 0, 8, C.byref(n)) == DH_EINVAL
    for jb in [(0, 5, 0, 5, 9, 0), (0, 0, 9, 4, 9, 0), (0, 8, 0, 2, 4, 0), (1, 0, 0, 4, 4, 0), (-1, 0, 0, 4, 4, 0)]:
        assert lib.dh_crop_program_bytes((_lib.CropJob * 1)(_lib.CropJob(*jb)), 1, 1, 8, 8, C.byref(n)) == DH_EINVAL, jb
    assert lib.dh_crop_program_bytes(ok_job, 1, 1, 8, 8, C.byref(n)) == 0
    args = (1, ok_job, 1, 8, 8)
    assert lib.dh_crop_program_build_host(None, *args, out.ctypes.data, n.value) == DH_EINVAL
    assert lib.dh_crop_program_build_host(ok_src, *args, None, n.value) == DH_EINVAL
    assert lib.dh_crop_program_build_host(ok_src, *args, out.ctypes.data, n.value - 8) == DH_EINVAL
    for s in [_lib.CropSrc(None, 210, 70, 70), _lib.CropSrc(srcbuf.ctypes.data, 209, 70, 70), _lib.CropSrc(srcbuf.ctypes.data, 210, 0, 70)]:
        assert lib.dh_crop_program_build_host((_lib.CropSrc * 1)(s), *args, out.ctypes.data, n.value) == DH_EINVAL
    assert not out.any()                                                          # nothing was written by any refusal
    assert lib.dh_crop_program_build_host(ok_src, *args, out.ctypes.data, n.value) == 0
    prog = out.view(np.uint8)[:n.value]
    # host twin: NULL pointers, a short item pitch, a truncated / foreign / mismatched program
    y = np.full(8 * 8 * 3, 0xCD, np.uint8)
    twin = lib.dh_crop_resize_host
    assert twin(None, prog.size, 1, 8, 8, y.ctypes.data, 192) == DH_EINVAL
    assert twin(prog.ctypes.data, prog.size, 1, 8, 8, None, 192) == DH_EINVAL
    assert twin(prog.ctypes.data, prog.size, 1, 8, 8, y.ctypes.data, 191) == DH_EINVAL
    assert twin(prog.ctypes.data, prog.size - 8, 1, 8, 8, y.ctypes.data, 192) == DH_EINVAL
    assert twin(prog.ctypes.data, prog.size, 2, 8, 8, y.ctypes.data, 192) == DH_EINVAL         # more jobs than the program has
    assert twin(prog.ctypes.data, prog.size, 1, 8, 4, y.ctypes.data, 192) == DH_EINVAL         # another output size
    for off, val in [(0, 0), (4, 0), (job_off_of(prog) + 32, 0), (job_off_of(prog) + 36, 1 << 30)]:   # magic, nsrc, band, x table
        bad = np.zeros(prog.size // 8 + 1, np.uint64)
        b8 = bad.view(np.uint8)[:prog.size]
        b8[:] = prog
        b8[off:off + 4].view(np.uint32)[0] = val
        assert twin(b8.ctypes.data, b8.size, 1, 8, 8, y.ctypes.data, 192) == DH_EINVAL, off
    assert np.all(y == 0xCD)
    assert twin(prog.ctypes.data, prog.size, 1, 8, 8, y.ctypes.data, 192) == 0
    assert np.array_equal(y.reshape(8, 8, 3), cropref.crop_resize(img, (0, 0, 32, 32), (8, 8)))
    # the launch refuses bad arguments before it touches the GPU
    launch = lib.dh_crop_resize_u8
    assert launch(None, 1, 8, 8, 4096, 192, None) == DH_EINVAL
    assert launch(4096, 1, 8, 8, None, 192, None) == DH_EINVAL
    assert launch(4096, 0, 8, 8, 4096, 192, None) == DH_EINVAL
    assert launch(4096, 1, 8, 8, 4096, 191, None) == DH_EINVAL
    assert launch(4096, 1, 2, 20000, 8192, 2 * 20000 * 3, None) == DH_EUNSUPPORTED            # two LDS rows of 60 000 bytes


def job_off_of(prog):
    return int(prog[24:28].view(np.uint32)[0])


# ---- the Python bookkeeping ------------------------------------------------------------------------------------------------
def test_frontend_box_and_matrix_equal_cropref(golden):
    from deephar_amd import frontend
    for c in golden[1]:
        box = frontend.crop_box(c['objpos'], c['winsize'])
        assert box.dtype.kind == 'i' and np.array_equal(box, c['box'])
        assert np.array_equal(frontend.crop_afmat(box, c['size'], bool(c['hflip'])), c['afmat'])
    rng = np.random.default_rng(2)
    for _ in range(50):
        objpos, win = rng.uniform(-50, 400, 2), rng.uniform(1, 500, 2)
        box = frontend.crop_box(objpos, win)
        assert np.array_equal(box, cropref.crop_box(objpos, win))
        if box[2] > box[0] and box[3] > box[1]:
            for flip in (False, True):
                assert np.array_equal(frontend.crop_afmat(box, (48, 64), flip), cropref.crop_afmat(box, (48, 64), flip))


class CropDataset:
    """MPII-shaped stub over full frames: frames / afmat / bbox are live views that re-crop (with cropref) when custom boxes
    are set, like the reference's loader does with PIL."""

    def __init__(self, images, boxes, out_hw):
        self.images, self.box0, self.out_hw = images, np.array(boxes, np.float64), out_hw
        self.custom = []

    def set_custom_bboxes(self, mode, boxes):
        self.custom = [] if len(boxes) == 0 else np.array(boxes, np.float64).copy()

    def clear_custom_bboxes(self, mode):
        self.custom = []

    def boxes(self):
        return self.box0 if len(self.custom) == 0 else self.custom

    def int_boxes(self):
        from deephar_amd.utils import bbox_to_objposwin
        return [cropref.crop_box(*bbox_to_objposwin(b)) for b in self.boxes()]

    class _View:
        def __init__(self, fn):
            self.fn = fn

        def __getitem__(self, k):
            return self.fn()[k]

        def __len__(self):
            return len(self.fn())

        def __array__(self, dtype=None, copy=None):
            a = self.fn()
            return a if dtype is None else a.astype(dtype)

    def frames(self):
        return self._View(lambda: np.stack([cropref.crop_resize(im, b, self.out_hw) for im, b in zip(self.images, self.int_boxes())]))

    def afmat(self):
        OH, OW = self.out_hw
        return self._View(lambda: np.stack([cropref.crop_afmat(b, (OW, OH)) for b in self.int_boxes()]))

    def bbox(self):
        return self._View(lambda: self.boxes().copy())


class FrameStubModel:
    """predict() of tests/evalstubs.StubModel, plus the predict_from_frames protocol refine_pred_frames drives: it crops on
    the host with cropref, where the real front end crops on the GPU."""

    def __init__(self, out_hw, specs):
        from evalstubs import StubModel
        self.inner = StubModel(out_hw + (3,), specs)
        self.out_hw = out_hw

    def predict(self, x, batch_size=None, verbose=0):
        return self.inner.predict(np.asarray(x), batch_size=batch_size)


def test_refine_pred_frames_equals_refine_pred(monkeypatch):
    from deephar_amd import frontend
    from deephar_amd.evaltools import bbox as bbtools
    rng = np.random.default_rng(9)
    images = [cropref.synthetic_image(40 + i, 60 + 3 * i, 80 - 2 * i) for i in range(5)]
    boxes = np.concatenate([rng.uniform(-10, 20, (5, 2)), rng.uniform(40, 75, (5, 2))], axis=1)
    out_hw = (16, 16)
    ds = CropDataset(images, boxes, out_hw)
    model = FrameStubModel(out_hw, [('pose', 16, 3), ('pose', 16, 3)])
    want = bbtools.refine_pred(model, ds.frames(), ds.afmat(), ds.bbox(), ds, 2, 1, num_iter=3)

    def host_predict_from_frames(m, frames, index, bxs, hflip=None, batch_size=32):      # the GPU front end, on the host
        crops = np.stack([cropref.crop_resize(frames[i], b, out_hw) for i, b in zip(index, bxs)])
        A = np.stack([frontend.crop_afmat(b, (out_hw[1], out_hw[0]), False) for b in bxs])
        return list(m.predict(crops, batch_size=batch_size)) + [A]

    monkeypatch.setattr(frontend, 'predict_from_frames', host_predict_from_frames)
    got = bbtools.refine_pred_frames(FrameStubModel(out_hw, [('pose', 16, 3), ('pose', 16, 3)]), images, boxes, 1, num_iter=3)
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
