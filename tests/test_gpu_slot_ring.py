"""The executor's chunk loops when a slot of the output ring is RECLAIMED while the loop is still enqueuing: five frames at
batch 2 on a ring of two slots (chunks of 2, 2 and a ragged 1: the third waits for slot 0 and takes it over) against the same
entry point run as ONE chunk of five, which reclaims nothing -- bit for bit.  Then the ring grows on the same bound plan.
Model.predict on uint8 crops, predict_from_frames under both programs, refine_pred_frames(loop='device').  No PIL, no
reference checkout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropref  # noqa: E402
from test_gpu_crop import _as_list, _frames_and_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
N = 5                                                                           # of the six fixture frames


@pytest.fixture(scope='module')
def small_model(cuda, hip_lib):
    """ONE model for every test of this file: its executor's tune table and bound plans (batch 2 and 5) are shared."""
    from test_gpu_models import _build
    model, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)
    return model


@pytest.fixture(scope='module')
def five():
    images, boxes, flips = _frames_and_boxes(6, 3)
    return images[:N], boxes[:N], flips[:N]


def _recycled_equals_one_chunk(monkeypatch, run):
    """run(batch_size) -> list of arrays.  One chunk; three chunks on two slots; three chunks on three slots (the ring of the
    batch-2 plan grows from 2)."""
    want = run(N)
    for w in want:
        w.setflags(write=False)
    monkeypatch.setenv('DEEPHAR_PREDICT_DEPTH', '2')
    tight = run(2)
    monkeypatch.delenv('DEEPHAR_PREDICT_DEPTH')
    grown = run(2)
    for name, got in (('two slots', tight), ('grown ring', grown)):
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, k)


def test_predict_reclaims_a_slot_while_enqueuing(monkeypatch, cuda, hip_lib, small_model, five):
    images, boxes, flips = five
    crops = np.stack([cropref.crop_resize(images[i], boxes[i], (256, 256), flips[i]) for i in range(N)])
    _recycled_equals_one_chunk(monkeypatch, lambda bs: _as_list(small_model.predict(crops, batch_size=bs)))


@pytest.mark.parametrize('program', ['host', 'device'])
def test_predict_from_frames_reclaims_a_slot_while_enqueuing(program, monkeypatch, cuda, hip_lib, small_model, five):
    from deephar_amd import frontend
    images, boxes, flips = five
    store = frontend.FrameStore(images, cuda)
    _recycled_equals_one_chunk(monkeypatch, lambda bs: frontend.predict_from_frames(
        small_model, store, np.arange(N), boxes, hflip=flips, batch_size=bs, program=program))


def test_refine_device_loop_reclaims_slots_while_enqueuing(monkeypatch, cuda, hip_lib, small_model, five):
    """num_iter = 2 over three chunks: six chunk-steps on two slots, four of them reclaim one."""
    from deephar_amd import frontend
    from deephar_amd.evaltools import mpii_tools
    images, boxes, _ = five
    store = frontend.FrameStore(images, cuda)
    _recycled_equals_one_chunk(monkeypatch, lambda bs: mpii_tools.refine_pred_frames(
        small_model, store, boxes.astype(np.float64), 2, num_iter=2, batch_size=bs, loop='device'))
