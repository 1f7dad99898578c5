"""The multi-clip action vote on the GPU: dh_vote_products_f64 against its host twin bit for bit (products, labels, scores) on
dense and strided sources inside NaN-filled slabs with the outputs between canaries; the edge items (subnormal products
included); split launches; more than one launch's worth of sources; a source row beyond 2^32 bytes; functional.vote_products;
multiclip_votes_frames(loop='device') against loop='host' on a small merge clip model with one and two streams; the refusals of
frontend.votes_from_frames; and loop='host' against Model.predict on the loader-path crops.  No PIL, no reference checkout."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cropref  # noqa: E402
import votecases as vc  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY_F64, CANARY_F32, CANARY_I = -777.125, -555.5, -7777
GUARD = 70                                                # canary elements in front of and behind every output


def _device_vote(cuda, lib, preds, seq, nseq, acc0=None, keep_scores=True, stride_pad=0, off=0):
    """dh_vote_products_f64 -> (acc, label, scores) as numpy.  Source b lies in a NaN-filled slab of its own, rows
    C + stride_pad * (b + 1) floats apart, the first one `off` + b floats in; acc, label and scores lie between GUARD canaries,
    which are checked, and the sources and seq are checked to have been only read."""
    from deephar_amd import _lib
    nb, (n, C) = len(preds), preds[0].shape
    slabs, views = [], []
    for b, p in enumerate(preds):
        stride, o = C + stride_pad * (b + 1), (off + b if off else 0)
        slab = torch.full((o + n * stride + 5,), float('nan'), dtype=torch.float32, device=cuda)
        view = torch.as_strided(slab, (n, C), (stride, 1), o)
        view.copy_(torch.from_numpy(p))
        slabs.append((slab, slab.clone()))
        views.append((view, stride))
    srcs = (_lib.VoteSrc * nb)(*[_lib.VoteSrc(v.data_ptr(), s) for v, s in views])
    sd = torch.from_numpy(np.ascontiguousarray(seq, np.int32)).to(cuda)
    na, nl, ns = nb * nseq * C, nb * n, nb * n * C
    acc = torch.full((na + 2 * GUARD,), CANARY_F64, dtype=torch.float64, device=cuda)
    acc[GUARD:GUARD + na] = torch.from_numpy(np.ones(na) if acc0 is None else acc0.reshape(-1)).to(cuda)
    label = torch.full((nl + 2 * GUARD,), CANARY_I, dtype=torch.int32, device=cuda)
    scores = torch.full((ns + 2 * GUARD,), CANARY_F32, dtype=torch.float32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.dh_vote_products_f64(srcs, nb, C, sd.data_ptr(), n, nseq, acc[GUARD:].data_ptr(), label[GUARD:].data_ptr(),
                                    scores[GUARD:].data_ptr() if keep_scores else None, st) == 0
    torch.cuda.synchronize()
    a, l, s = acc.cpu().numpy(), label.cpu().numpy(), scores.cpu().numpy()
    for t, g, m in ((a, CANARY_F64, na), (l, CANARY_I, nl), (s, CANARY_F32, ns if keep_scores else 0)):
        assert np.all(t[:GUARD] == g) and np.all(t[GUARD + m:] == g), 'a canary was written'
    for slab, before in slabs:                                               # bit for bit: the NaN filling included
        assert torch.equal(slab.view(torch.int32), before.view(torch.int32))
    assert np.array_equal(sd.cpu().numpy(), np.ascontiguousarray(seq, np.int32))
    return (a[GUARD:GUARD + na].reshape(nb, nseq, C), l[GUARD:GUARD + nl].reshape(nb, n),
            s[GUARD:GUARD + ns].reshape(nb, n, C) if keep_scores else None)


def _same(got, want):
    return vc.same_f64(got[0], want[0]) and np.array_equal(got[1], want[1]) and \
        (want[2] is None and got[2] is None or vc.same_f32(got[2], want[2]))


@pytest.mark.parametrize('C', [1, 15, 60, 64, 65, 130])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65])
def test_vote_device_equals_host_twin(n, C, cuda, hip_lib):
    """nb = 1, 3 and 33 (a second launch for the 33rd source), dense and strided sources; unsorted sequences, one of which no
    item names; acc starts from random values, so a lost or doubled multiplication shows"""
    for nb in (1, 3, 33):
        rng = np.random.default_rng(10000 * n + 10 * C + nb)
        nseq = 5
        preds = vc.random_preds(rng, nb, n, C)
        seq = rng.integers(0, nseq - 1, n).astype(np.int32)                  # sequence 4 is never named
        acc0 = rng.uniform(0.5, 2.0, (nb, nseq, C))
        want = vc.host_vote(hip_lib, preds, seq, nseq, acc0.copy())
        assert np.array_equal(want[0][:, 4], acc0[:, 4])
        assert _same(_device_vote(cuda, hip_lib, preds, seq, nseq, acc0), want), ('dense', nb)
        assert _same(_device_vote(cuda, hip_lib, preds, seq, nseq, acc0, stride_pad=3, off=1), want), ('strided', nb)


@pytest.mark.parametrize('case', vc.edge_cases(), ids=lambda c: c[0])
def test_edge_cases_on_device(case, cuda, hip_lib):
    name, rows, seq, nseq, by_hand = case
    want = vc.host_vote(hip_lib, [rows], seq, nseq)
    got = _device_vote(cuda, hip_lib, [rows], seq, nseq)
    assert got[1][0].tolist() == by_hand
    assert _same(got, want)
    if name == 'subnormal_then_zero':                                        # double denormals survive on the device
        run = _device_vote(cuda, hip_lib, [rows[:9]], seq[:9], nseq)[0]
        assert np.all(run > 0) and np.all(run < np.finfo(np.float64).tiny)
        assert vc.same_f64(run, vc.host_vote(hip_lib, [rows[:9]], seq[:9], nseq)[0])


def test_two_launches_over_a_split_equal_one_and_no_scores(cuda, hip_lib):
    rng = np.random.default_rng(21)
    nb, C, n, nseq = 3, 15, 13, 4
    preds = vc.random_preds(rng, nb, n, C)
    preds[2][5, 7] = np.nan
    seq = rng.integers(0, nseq, n).astype(np.int32)
    want = vc.host_vote(hip_lib, preds, seq, nseq)
    for n1 in (1, 6, 12):
        a1, l1, s1 = _device_vote(cuda, hip_lib, [p[:n1] for p in preds], seq[:n1], nseq)
        a2, l2, s2 = _device_vote(cuda, hip_lib, [p[n1:] for p in preds], seq[n1:], nseq, a1)
        assert _same((a2, np.concatenate([l1, l2], axis=1), np.concatenate([s1, s2], axis=1)), want), n1
    got = _device_vote(cuda, hip_lib, preds, seq, nseq, keep_scores=False)
    assert got[2] is None and _same(got, (want[0], want[1], None))


def test_an_item_out_of_range_is_skipped(cuda, hip_lib):
    rng = np.random.default_rng(22)
    nb, C, n, nseq = 2, 65, 6, 2
    preds = vc.random_preds(rng, nb, n, C)
    for bad_value in (-1, nseq, 0x7fffffff):
        seq = np.array([0, 1, bad_value, 1, 1, 0], np.int32)
        want = vc.host_vote(hip_lib, preds, seq, nseq)
        got = _device_vote(cuda, hip_lib, preds, seq, nseq)
        assert np.all(got[1][:, 2] == -1) and np.all(got[2][:, 2] == np.float32(CANARY_F32))
        keep = np.array([0, 1, 3, 4, 5])
        assert vc.same_f64(got[0], want[0]) and np.array_equal(got[1], want[1]) and vc.same_f32(got[2][:, keep], want[2][:, keep])


def test_far_rows_beyond_4_gib(cuda, hip_lib):
    """n = 3 with an item stride of 2^29 + 3 floats: the last row lies more than 2^32 bytes behind the first.  The buffer is
    only allocated; the three rows are written and nothing is copied whole."""
    from deephar_amd import _lib
    C, n, nseq, stride = 15, 3, 2, (1 << 29) + 3
    assert (n - 1) * stride * 4 >= 1 << 32
    rng = np.random.default_rng(23)
    rows = vc.softmax_rows(rng, n, C)
    seq = np.array([1, 0, 1], np.int32)
    want = vc.host_vote(hip_lib, [rows], seq, nseq)
    buf = torch.empty((n - 1) * stride + C, dtype=torch.float32, device=cuda)
    for k in range(n):
        buf[k * stride:k * stride + C] = torch.from_numpy(rows[k]).to(cuda)
    srcs = (_lib.VoteSrc * 1)(_lib.VoteSrc(buf.data_ptr(), stride))
    sd = torch.from_numpy(seq).to(cuda)
    acc = torch.ones((1, nseq, C), dtype=torch.float64, device=cuda)
    label = torch.full((1, n), CANARY_I, dtype=torch.int32, device=cuda)
    scores = torch.full((1, n, C), CANARY_F32, dtype=torch.float32, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert hip_lib.dh_vote_products_f64(srcs, 1, C, sd.data_ptr(), n, nseq, acc.data_ptr(), label.data_ptr(), scores.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert _same((acc.cpu().numpy(), label.cpu().numpy(), scores.cpu().numpy()), want)
    del buf


def test_functional_vote_products(cuda, hip_lib):
    from deephar_amd import functional as Fn
    rng = np.random.default_rng(24)
    nb, C, n, nseq = 3, 60, 10, 3
    preds = vc.random_preds(rng, nb, n, C)
    seq = rng.integers(0, nseq, n).astype(np.int32)
    want = vc.host_vote(hip_lib, preds, seq, nseq)
    dense = [torch.from_numpy(p).to(cuda) for p in preds]
    wide = torch.full((n, nb, C + 4), float('nan'), dtype=torch.float32, device=cuda)
    for b in range(nb):
        wide[:, b, 2:C + 2] = dense[b]
    acc, label, scores = Fn.vote_products(dense, seq, nseq, keep_scores=True)
    assert acc.dtype == torch.float64 and label.dtype == torch.int32 and scores.dtype == torch.float32
    assert _same((acc.cpu().numpy(), label.cpu().numpy(), scores.cpu().numpy()), want)
    out = Fn.vote_products([wide[:, b, 2:C + 2] for b in range(nb)], torch.from_numpy(seq).to(cuda), nseq)       # views, no scores
    assert len(out) == 2 and _same((out[0].cpu().numpy(), out[1].cpu().numpy(), None), (want[0], want[1], None))
    # acc is multiplied in place: two calls over a split
    acc2, l1 = Fn.vote_products([d[:4] for d in dense], seq[:4], nseq)
    acc3, l2 = Fn.vote_products([d[4:] for d in dense], seq[4:], nseq, acc=acc2)
    assert acc3 is acc2 and vc.same_f64(acc3.cpu().numpy(), want[0])
    assert np.array_equal(torch.cat([l1, l2], dim=1).cpu().numpy(), want[1])
    for bad in [dict(probs=[dense[0], dense[1][:, :5]]), dict(probs=[dense[0].double()]), dict(seq=seq[:-1]), dict(nseq=0),
                dict(probs=[]), dict(acc=torch.ones((nb, nseq, C), dtype=torch.float32, device=cuda)), dict(probs=[preds[0]])]:
        with pytest.raises(ValueError):
            Fn.vote_products(**dict(dict(probs=dense, seq=seq, nseq=nseq), **bad))


# ---- whole models ----------------------------------------------------------------------------------------------------------
T = 4
COUNTS = [3, 1, 2]                                        # clips per sequence; x 2 flips = 12 items
FIRST = [0, 6, 2]                                         # the stored frame of every sequence's frame 0
LENGTH = [6, 4, 5]                                        # frames per sequence: clip f covers frames f .. f + 3


def _merge_model(streams=1):
    from test_gpu_models import _merge
    model, _ = _merge(2, T, 16, 2, num_actions=15)
    if streams > 1:
        model.num_streams = streams
    return model


@pytest.fixture(scope='module')
def clip_model(cuda, hip_lib):
    return _merge_model()


@pytest.fixture(scope='module')
def clips(clip_model):
    """12 frames of 360 x 480, the per-frame box dictionary, and the items in the reference's order; the action outputs of the
    model; loop='host' at batch 5, computed once"""
    from deephar_amd import evaltools
    from deephar_amd.evaltools import clip_window, compute_clip_bbox
    images = [cropref.synthetic_image(900 + i, 360, 480) for i in range(12)]
    boxes = {'%d.%d' % (s, f): [40 + 9 * f + 30 * s, 20 + 4 * f, 400 - 7 * f + 20 * s, 340 - 5 * f + s]
             for s in range(3) for f in range(LENGTH[s])}
    boxes['1.2'] = [200, 150, 215, 330]                                       # sequence 1 keeps its other frames' union
    boxes['2.0'] = [-35, -22, 180, 300]                                       # a window that leaves the image
    seq, keys = vc.sequences(COUNTS)
    index, windows, hflip = [], [], []
    for s, c in enumerate(COUNTS):
        for f in range(c):
            frames = list(range(f, f + T))
            w = clip_window(compute_clip_bbox(boxes, s, frames))
            for h in (0, 1):
                index.append([FIRST[s] + t for t in frames])
                windows.append(w)
                hflip.append(h)
    index, windows, hflip = np.array(index), np.stack(windows), np.array(hflip)
    assert index.shape == (12, T) and windows.shape == (12, 4) and windows.dtype.kind == 'i'
    actions = [k for k, v in enumerate(clip_model.outputs) if len(v.shape) == 1]
    assert len(actions) >= 2 and all(tuple(clip_model.outputs[k].shape) == (15,) for k in actions)
    a_true = np.eye(15)[[3, 7, 11]]
    return dict(images=images, index=index, windows=windows, hflip=hflip, seq=seq, keys=keys, actions=actions, a_true=a_true)


def _run(model, c, tmp, loop, batch, pred_file='a_pred.npy'):
    from deephar_amd.evaltools import multiclip_votes_frames
    log = tmp / ('%s_%d_%s' % (loop, batch, pred_file))
    log.mkdir()
    scores = multiclip_votes_frames(model, c['images'], c['index'], c['windows'], c['hflip'], c['seq'], c['a_true'], c['keys'],
                                    batch_size=batch, loop=loop, outidx=c['actions'], logdir=str(log), pred_file=pred_file, verbose=0)
    return scores, np.load(str(log / pred_file)), json.load(open(str(log / 'missing-clips.json'))), np.load(str(log / 'a_true.npy'))


@pytest.mark.parametrize('streams,batch', [(1, 5), (1, 16), (2, 5), (2, 16)])
def test_multiclip_votes_frames_loop_device_equals_host(streams, batch, cuda, hip_lib, clip_model, clips, tmp_path):
    """batch 5: ragged, sequences straddle chunks; batch 16: one chunk"""
    model = clip_model if streams == 1 else _merge_model(streams)
    if streams > 1:
        model.executor.tune_table = clip_model.executor.tune_table          # (tilings never move a bit; this spares the timing)
    nb = len(clips['actions'])
    for pred_file, shape in (('a_pred.npy', (nb, 3, 15)), ('allpred.npy', (nb, 2 * COUNTS[-1], 15))):
        want = _run(model, clips, tmp_path, 'host', batch, pred_file)
        got = _run(model, clips, tmp_path, 'device', batch, pred_file)
        assert want[1].shape == shape and want[1].dtype == np.float64 and got[1].dtype == np.float64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert np.array_equal(got[3], want[3]) and np.array_equal(want[3], clips['a_true'])
        assert want[0].shape == (nb,)
    assert len(want[2]) > 0                                                  # (synthetic weights: some running label is wrong)


def test_votes_from_frames_labels_follow_its_products_and_refusals(cuda, hip_lib, clip_model, clips):
    from deephar_amd import frontend
    from deephar_amd.evaltools import vote_products
    c = clips
    a = (c['images'], c['index'], c['windows'], c['hflip'], c['seq'])
    a_pred, labels, scores = frontend.votes_from_frames(clip_model, *a, nseq=3, outidx=c['actions'], keep_scores=True, batch_size=5)
    nb = len(c['actions'])
    assert a_pred.shape == (nb, 3, 15) and a_pred.dtype == np.float64 and labels.shape == (nb, 12) and labels.dtype == np.int32
    assert scores.shape == (nb, 12, 15) and scores.dtype == np.float32
    again, relabel = vote_products([scores[b] for b in range(nb)], c['seq'], 3)
    assert np.array_equal(again, a_pred) and np.array_equal(relabel, labels)
    b_pred, b_labels, none = frontend.votes_from_frames(clip_model, *a, outidx=c['actions'][-1:], batch_size=16)   # nseq from seq
    assert none is None and np.array_equal(b_pred[0], a_pred[-1]) and np.array_equal(b_labels[0], labels[-1])
    pose = [k for k, v in enumerate(clip_model.outputs) if len(v.shape) != 1][0]
    bad_seq = c['seq'].copy()
    bad_seq[3] = 3
    for kw in [dict(outidx=[pose]), dict(outidx=[c['actions'][0], pose]), dict(windows=c['windows'].astype(np.float64)),
               dict(seq=bad_seq), dict(seq=-c['seq']), dict(index=c['index'] + 3), dict(index=c['index'][:, 0]),
               dict(hflip=c['hflip'][:-1])]:
        k = dict(dict(index=c['index'], windows=c['windows'], hflip=c['hflip'], seq=c['seq'], nseq=3, outidx=c['actions']), **kw)
        with pytest.raises(ValueError):
            frontend.votes_from_frames(clip_model, c['images'], k['index'], k['windows'], k['hflip'], k['seq'], nseq=k['nseq'],
                                       outidx=k['outidx'], batch_size=5)
    # a window the program builder refuses (an empty one): the error of the host path, after a clean drain
    empty = c['windows'].copy()
    empty[7] = [80, 60, 50, 200]
    with pytest.raises(ValueError, match='empty crop box'):
        frontend.votes_from_frames(clip_model, c['images'], c['index'], empty, c['hflip'], c['seq'], outidx=c['actions'], batch_size=5)
    with pytest.raises(ValueError, match='empty crop box'):
        frontend.predict_from_frames(clip_model, c['images'], c['index'], empty, c['hflip'], batch_size=5)
    after = frontend.votes_from_frames(clip_model, *a, nseq=3, outidx=c['actions'], keep_scores=True, batch_size=5)
    assert np.array_equal(after[0], a_pred) and np.array_equal(after[1], labels) and np.array_equal(after[2], scores)


def test_loop_host_equals_predict_on_loader_path_crops(cuda, hip_lib, clip_model, clips, tmp_path):
    """independence from the front end: Model.predict on the crops the loaders would make (tests/cropref.py, mirrored ones
    included) at the same batch size, voted on the host"""
    from deephar_amd.evaltools import vote_products
    c = clips
    x = np.stack([np.stack([cropref.crop_resize(c['images'][i], c['windows'][k], (256, 256), bool(c['hflip'][k]))
                            for i in c['index'][k]]) for k in range(12)])
    assert x.shape == (12, T, 256, 256, 3) and x.dtype == np.uint8
    for batch in (5, 16):
        outs = clip_model.predict(x, batch_size=batch)
        a_pred, labels = vote_products([outs[k] for k in c['actions']], c['seq'], 3)
        want = _run(clip_model, c, tmp_path, 'host', batch)
        assert np.array_equal(a_pred, want[1])
        missing = {c['keys'][k]: [int(np.argmax(c['a_true'][c['seq'][k]])), int(labels[-1, k])] for k in range(12)
                   if np.argmax(c['a_true'][c['seq'][k]]) != labels[-1, k]}
        assert missing == want[2]
