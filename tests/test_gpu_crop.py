"""The crop-and-resize front end on the GPU: dh_crop_resize_u8 against tests/cropref.py, exactly, with sentinel bytes around
every item; predict_from_frames against model.predict on cropref's crops, bit for bit; refine_pred_frames against
refine_pred over a dataset stub that crops with cropref.  No PIL, no reference checkout."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64                                                # sentinel bytes in front of and behind every item (keeps 16-byte alignment)


def run_op(cuda, images, jobs, OH, OW, pitches=None, guard=GUARD):
    """Every job in ONE launch into a sentinel-filled buffer; returns uint8 [njobs, OH, OW, 3] after checking the sentinels."""
    from deephar_amd import functional as F
    srcs = []
    for i, im in enumerate(images):
        H, W = im.shape[:2]
        pitch = pitches[i] if pitches else 3 * W
        wide = np.full((H, pitch), 0xAB, np.uint8)
        wide[:, :3 * W] = im.reshape(H, 3 * W)
        t = torch.from_numpy(wide).to(cuda)
        srcs.append(torch.as_strided(t, (H, W, 3), (pitch, 3, 1)))
    item = OH * OW * 3
    pitch_out = item + guard
    buf = torch.full((guard + len(jobs) * pitch_out,), 0xCD, dtype=torch.uint8, device=cuda)
    F.crop_resize(srcs, jobs, (OH, OW), out=buf[guard:], item_pitch=pitch_out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:guard] == 0xCD)
    body = host[guard:].reshape(len(jobs), pitch_out)
    assert np.all(body[:, item:] == 0xCD), 'bytes behind an item were overwritten'
    return body[:, :item].reshape(len(jobs), OH, OW, 3)


def check(cuda, shapes, jobs, OH, OW, pitches=None, seed=0, guard=GUARD):
    images = [cropref.synthetic_image(seed + i, h, w) for i, (h, w) in enumerate(shapes)]
    got = run_op(cuda, images, jobs, OH, OW, pitches, guard)
    for j, (s, box, flip) in enumerate(jobs):
        want = cropref.crop_resize(images[s], box, (OH, OW), bool(flip))
        assert np.array_equal(got[j], want), (j, box, flip, int(np.abs(got[j].astype(int) - want).max()))
    return got


OP_CASES = {
    'identity_8x8': ([(8, 8)], [(0, (0, 0, 8, 8), 0)], 8, 8, None),
    'up_5x7_to_16x16': ([(5, 7)], [(0, (0, 0, 7, 5), 0)], 16, 16, None),
    'odd_37x53_to_8x8': ([(37, 53)], [(0, (3, 2, 36, 50), 0)], 8, 8, None),
    'scale16_64_to_4': ([(64, 64)], [(0, (0, 0, 64, 64), 0)], 4, 4, None),
    'overhang_each_edge': ([(30, 40)], [(0, (-9, 4, 21, 24), 0), (0, (25, 4, 55, 24), 0), (0, (5, -7, 35, 13), 0),
                                        (0, (5, 20, 35, 41), 0)], 8, 8, None),
    'fully_outside': ([(30, 40)], [(0, (50, 50, 70, 70), 0), (0, (-40, 2, -1, 20), 1)], 8, 8, None),
    'width_1': ([(30, 40)], [(0, (7, 3, 8, 19), 0), (0, (39, -4, 40, 30), 1)], 8, 8, None),
    'bands_64x48': ([(100, 90)], [(0, (-5, 3, 80, 99), 0), (0, (10, 10, 42, 34), 1)], 64, 48, None),
    'bands_48x64': ([(100, 90)], [(0, (-5, 3, 80, 99), 1), (0, (10, 10, 42, 34), 0)], 48, 64, None),
    'width_5_elementwise': ([(37, 53)], [(0, (3, 2, 36, 50), 0), (0, (0, 0, 53, 37), 1)], 6, 5, None),
    'flip_on_and_off': ([(37, 53)], [(0, (3, 2, 36, 50), 0), (0, (3, 2, 36, 50), 1)], 16, 16, None),
    'three_sources_five_jobs': ([(16, 16), (37, 53), (9, 70)], [(2, (0, 0, 70, 9), 0), (0, (-2, -2, 18, 18), 1),
                                                                (1, (0, 0, 53, 37), 0), (2, (60, 2, 90, 12), 1),
                                                                (1, (5, 5, 6, 6), 0)], 16, 16, [48, 200, 211]),
}


@pytest.mark.parametrize('name', sorted(OP_CASES))
def test_crop_resize_equals_cropref(name, cuda, hip_lib):
    shapes, jobs, OH, OW, pitches = OP_CASES[name]
    got = check(cuda, shapes, jobs, OH, OW, pitches, seed=sum(map(ord, name)))
    if name == 'fully_outside':
        assert not got.any()
    if name == 'flip_on_and_off':
        assert np.array_equal(got[0], got[1][:, ::-1]) and not np.array_equal(got[0], got[1])
    if name == 'identity_8x8':
        assert np.array_equal(got[0], cropref.synthetic_image(sum(map(ord, name)), 8, 8))


def test_crop_resize_misaligned_destination_takes_the_bytewise_path(cuda, hip_lib):
    """A 16 x 16 output (48-byte rows) whose items do not start on 16-byte boundaries: same bits, sentinels intact."""
    check(cuda, [(37, 53)], [(0, (3, 2, 36, 50), 0), (0, (10, 10, 30, 31), 1)], 16, 16, seed=5, guard=7)


def test_crop_resize_real_row_720x1280_to_256(cuda, hip_lib):
    check(cuda, [(720, 1280)], [(0, (300, 60, 900, 660), 0), (0, (800, 300, 1400, 900), 1)], 256, 256, seed=21)


def test_crop_resize_refuses_beyond_the_scale_cap(cuda, hip_lib):
    from deephar_amd import functional as F
    src = torch.zeros((70, 70, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        F.crop_resize([src], [(0, (0, 0, 65, 64), 0)], (4, 4))
    with pytest.raises(ValueError):
        F.crop_resize([src], [(0, (5, 5, 5, 9), 0)], (4, 4))


# ---- whole models ------------------------------------------------------------------------------------------------------------
def _frames_and_boxes(n, seed, H=300, W=340):
    rng = np.random.default_rng(seed)
    images = [cropref.synthetic_image(seed * 100 + i, H, W) for i in range(n)]
    boxes = []
    for i in range(n):
        side_w, side_h = int(rng.integers(120, 400)), int(rng.integers(120, 400))
        x0, y0 = int(rng.integers(-60, W - 80)), int(rng.integers(-60, H - 80))
        boxes.append((x0, y0, x0 + side_w, y0 + side_h))
    flips = [bool(i % 2) for i in range(n)]
    return images, np.array(boxes, dtype=int), flips


def _as_list(r):
    return r if isinstance(r, list) else [r]


@pytest.mark.parametrize('streams', [1, 2])
def test_predict_from_frames_equals_predict_on_cropref_crops(streams, cuda, hip_lib):
    from test_gpu_models import _build
    from deephar_amd import frontend
    model, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)
    if streams > 1:
        model.num_streams = streams
    images, boxes, flips = _frames_and_boxes(6, 3)
    crops = np.stack([cropref.crop_resize(images[i], boxes[i], (256, 256), flips[i]) for i in range(6)])
    want = _as_list(model.predict(crops, batch_size=4))
    got = frontend.predict_from_frames(model, images, np.arange(6), boxes, hflip=flips, batch_size=4)     # 4 + a ragged 2
    assert len(got) == len(want) + 1
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(g, w), [bool(np.array_equal(a, b)) for a, b in zip(g, w)]
    A = got[-1]
    assert A.shape == (6, 3, 3) and A.dtype == np.float64
    for i in range(6):
        assert np.array_equal(A[i], cropref.crop_afmat(boxes[i], (256, 256), flips[i]))
    # frames shared between jobs, in another order, from a store uploaded once
    store = frontend.FrameStore(images, cuda)
    idx = np.array([5, 0, 0, 3])
    got2 = frontend.predict_from_frames(model, store, idx, boxes[:4], batch_size=4)
    crops2 = np.stack([cropref.crop_resize(images[i], b, (256, 256)) for i, b in zip(idx, boxes[:4])])
    for g, w in zip(got2, _as_list(model.predict(crops2, batch_size=4))):
        assert np.array_equal(g, w)
    with pytest.raises(ValueError):                                            # beyond the scale cap: refused before anything runs
        big = [np.zeros((16, 5000, 3), np.uint8)]
        frontend.predict_from_frames(model, big, np.array([0]), np.array([[0, 0, 4200, 10]]))


def test_predict_from_frames_clip_model_with_clip_level_box(cuda, hip_lib):
    from test_gpu_models import _merge
    from deephar_amd import frontend
    model, _ = _merge(2, 4, 16, 2, num_actions=15)                              # input [T = 4, 256, 256, 3]
    images, boxes, _ = _frames_and_boxes(8, 7)
    index = np.arange(8).reshape(2, 4)
    clip_boxes = boxes[:2]
    crops = np.stack([np.stack([cropref.crop_resize(images[index[n, t]], clip_boxes[n], (256, 256)) for t in range(4)])
                      for n in range(2)])
    want = _as_list(model.predict(crops, batch_size=2))
    got = frontend.predict_from_frames(model, images, index, clip_boxes, batch_size=2)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert got[-1].shape == (2, 4, 3, 3)
    for n in range(2):
        for t in range(4):
            assert np.array_equal(got[-1][n, t], cropref.crop_afmat(clip_boxes[n], (256, 256), False))
    with pytest.raises(ValueError):
        frontend.predict_from_frames(model, images, np.arange(8), boxes)        # a clip model needs [N, T] indices


def test_refine_pred_frames_equals_refine_pred(cuda, hip_lib):
    from test_crop_host import CropDataset
    from test_gpu_models import _build
    from deephar_amd.evaltools import mpii_tools
    model, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)
    images, boxes, _ = _frames_and_boxes(6, 11)
    ds = CropDataset(images, boxes.astype(np.float64), (256, 256))
    outidx = 2                                                                  # outputs: pose 1, visibility 1, pose 2, visibility 2
    want = mpii_tools.refine_pred(model, ds.frames(), ds.afmat(), ds.bbox(), ds, 2, outidx, num_iter=2, batch_size=4)
    got = mpii_tools.refine_pred_frames(model, images, boxes.astype(np.float64), outidx, num_iter=2, batch_size=4)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
