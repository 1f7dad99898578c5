"""The multi-clip vote's index module (csrc/vote_index.h) through its host twin, without a GPU: dh_vote_products_host against
evaltools.action._multiclip itself (driven by a stub dataset and a stub model), against evaltools.action.vote_products and a
long-hand scalar loop bit for bit, the edge items, split calls, strided sources, more than one launch's worth of sources, every
refusal, the C-ABI surface, compute_clip_bbox / clip_window on hand-computed answers, the argument checks of
multiclip_votes_frames, and tools/vote_sweep.cpp built plainly and run."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import votecases as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DH_EINVAL = -1
FAKE = 0x10000                                            # a non-NULL, 8-byte aligned address no refusal may touch


# ---- against _multiclip ------------------------------------------------------------------------------------------------------
class _Conf:
    fixed_hflip = 0


class _StubClips:
    """the dataset surface _multiclip calls: sequence i has counts[i] clips; a clip's 'frame' carries its item number"""

    def __init__(self, counts, C, labels):
        self.counts, self.C, self.labels = counts, C, labels
        self.first = np.concatenate([[0], np.cumsum(2 * np.array(counts))])
        self.dataconf = _Conf()

    def get_length(self, mode):
        return len(self.counts)

    def get_shape(self, key):
        return (self.C,)

    def get_clip_index(self, i, mode, subsamples=(1,)):
        return [[f] for f in range(self.counts[i])]

    def get_data(self, i, mode, frame_list=None):
        k = self.first[i] + 2 * frame_list[0] + self.dataconf.fixed_hflip
        onehot = np.zeros(self.C)
        onehot[self.labels[i]] = 1
        return {'frame': np.full((1, 1, 1, 3), float(k)), 'pennaction': onehot}


class _StubModel:
    """predict returns row k of the precomputed float32 outputs, k read from the clip"""

    def __init__(self, preds):
        self.preds, self.outputs = preds, [None] * len(preds)

    def predict(self, x):
        k = int(x[0, 0, 0, 0, 0])
        return [p[k:k + 1] for p in self.preds]


@pytest.mark.parametrize('nb', [1, 3, 9])
@pytest.mark.parametrize('C', [15, 60])
def test_twin_and_numpy_loop_equal_multiclip(hip_lib, nb, C, tmp_path):
    from deephar_amd.evaltools import action
    rng = np.random.default_rng(100 * nb + C)
    counts = [int(c) for c in rng.permutation([1, 2, 3, 5])]                 # 4 sequences of 1-5 clips x 2 flips
    seq, keys = vc.sequences(counts)
    n, nseq = len(seq), len(counts)
    preds = vc.random_preds(rng, nb, n, C)
    # labels: the first two sequences get what the last output votes for, the others something else -> both kinds of keys
    final, _ = vc.longhand(preds[-1:], seq, nseq)
    labels = [int(np.argmax(final[0, i])) if i < 2 else int((np.argmax(final[0, i]) + 1) % C) for i in range(nseq)]
    ds, model = _StubClips(counts, C, labels), _StubModel(preds)
    logs = []
    for name in ('a_pred.npy', 'allpred.npy'):
        log = tmp_path / name.split('.')[0]
        log.mkdir()
        scores = action._multiclip(model, ds, 'pennaction', 1, None, str(log), 0, name)
        logs.append(log)
    a_pred = np.load(str(logs[0] / 'a_pred.npy'))
    allpred = np.load(str(logs[1] / 'allpred.npy'))
    missing = json.load(open(str(logs[0] / 'missing-clips.json')))
    a_true = np.load(str(logs[0] / 'a_true.npy'))

    acc, label, kept = vc.host_vote(hip_lib, preds, seq, nseq)
    acc_np, label_np = action.vote_products(preds, seq, nseq)
    assert a_pred.dtype == np.float64 and a_pred.shape == (nb, nseq, C)
    assert np.array_equal(acc, a_pred) and np.array_equal(acc_np, a_pred)
    assert np.array_equal(label, label_np) and label_np.dtype == np.int32
    want_missing = {keys[k]: [labels[seq[k]], int(label[-1, k])] for k in range(n) if labels[seq[k]] != label[-1, k]}
    assert missing == want_missing and 0 < len(missing) < n
    last = np.flatnonzero(seq == nseq - 1)
    assert allpred.shape == (nb, len(last), C) and np.array_equal(allpred, kept[:, last].astype(np.float64))
    for b in range(nb):
        assert np.array_equal(kept[b], preds[b])
    hit = np.argmax(a_true, axis=-1)[None, :] == np.argmax(acc, axis=-1)
    assert np.array_equal(scores, 100 * np.sum(hit, axis=-1) / nseq)


# ---- against the long-hand loop ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb,C,n,nseq', [(1, 1, 5, 2), (2, 15, 17, 4), (3, 64, 9, 3), (1, 65, 33, 5), (4, 130, 12, 12)])
def test_twin_equals_longhand_bit_for_bit(hip_lib, nb, C, n, nseq):
    rng = np.random.default_rng(n * C)
    preds = vc.random_preds(rng, nb, n, C)
    seq = rng.integers(0, nseq, n).astype(np.int32)                          # unsorted
    acc0 = rng.uniform(0.5, 2.0, (nb, nseq, C))
    want_acc, want_label = vc.longhand(preds, seq, nseq, acc0)
    acc, label, kept = vc.host_vote(hip_lib, preds, seq, nseq, acc0.copy())
    assert vc.same_f64(acc, want_acc) and np.array_equal(label, want_label)
    assert all(vc.same_f32(kept[b], preds[b]) for b in range(nb))
    untouched = np.setdiff1d(np.arange(nseq), seq)                           # canary rows: sequences no item names
    assert np.array_equal(acc[:, untouched].view(np.uint64), acc0[:, untouched].view(np.uint64))


@pytest.mark.parametrize('case', vc.edge_cases(), ids=lambda c: c[0])
def test_edge_cases(hip_lib, case):
    name, rows, seq, nseq, by_hand = case
    acc, label, kept = vc.host_vote(hip_lib, [rows], seq, nseq)
    assert label[0].tolist() == by_hand
    want_acc, want_label = vc.longhand([rows], seq, nseq)
    assert vc.same_f64(acc, want_acc) and np.array_equal(label, want_label)
    with np.errstate(all='ignore'):
        from deephar_amd.evaltools import action
        acc_np, label_np = action.vote_products([rows], seq, nseq)
    assert vc.same_f64(acc, acc_np) and np.array_equal(label, label_np)
    assert vc.same_f32(kept[0], rows)
    if name == 'subnormal_then_zero':
        run, _, _ = vc.host_vote(hip_lib, [rows[:9]], seq[:9], nseq)
        tiny = np.finfo(np.float64).tiny
        assert np.all(run > 0) and np.all(run < tiny), 'the ninth product is not subnormal'
        assert not acc.any()


def test_every_edge_is_there():
    names = {c[0] for c in vc.edge_cases()}
    assert {'ties', 'subnormal_then_zero', 'nan_then_lower_nan', 'inf_times_zero', 'negative', 'one_class'} <= names


# ---- split calls, strides, many sources -----------------------------------------------------------------------------------------
def test_split_calls_equal_one_call(hip_lib):
    rng = np.random.default_rng(5)
    nb, C, n, nseq = 3, 15, 14, 6
    preds = vc.random_preds(rng, nb, n, C)
    preds[1][6, 3] = np.nan
    seq = rng.integers(0, 4, n).astype(np.int32)                             # sequences 4 and 5 are never named
    acc0 = rng.uniform(0.5, 2.0, (nb, nseq, C))
    acc, label, kept = vc.host_vote(hip_lib, preds, seq, nseq, acc0.copy())
    assert np.array_equal(acc[:, 4:].view(np.uint64), acc0[:, 4:].view(np.uint64))
    for n1 in range(1, n):
        part = acc0.copy()
        _, la, ka = vc.host_vote(hip_lib, [p[:n1] for p in preds], seq[:n1], nseq, part)
        _, lb, kb = vc.host_vote(hip_lib, [p[n1:] for p in preds], seq[n1:], nseq, part)
        assert vc.same_f64(part, acc), n1
        assert np.array_equal(np.concatenate([la, lb], axis=1), label)
        assert vc.same_f32(np.concatenate([ka, kb], axis=1), kept)


def test_strided_sources_and_odd_offsets(hip_lib):
    """rows read in place from wider NaN-filled slabs, each source with its own stride and its own (odd) offset"""
    rng = np.random.default_rng(6)
    nb, C, n, nseq = 3, 15, 7, 3
    dense = vc.random_preds(rng, nb, n, C)
    seq = rng.integers(0, nseq, n).astype(np.int32)
    want = vc.host_vote(hip_lib, dense, seq, nseq)
    views = []
    for b, (stride, off) in enumerate([(15 + 1, 1), (40, 7), (33, 17)]):
        slab = np.full(n * stride + off, np.nan, np.float32)
        view = np.lib.stride_tricks.as_strided(slab[off:], (n, C), (4 * stride, 4))
        view[:] = dense[b]
        views.append(view)
    got = vc.host_vote(hip_lib, views, seq, nseq)
    assert vc.same_f64(got[0], want[0]) and np.array_equal(got[1], want[1]) and vc.same_f32(got[2], want[2])


def test_33_sources_no_scores_and_a_bad_sequence(hip_lib):
    """nb = 33 (the device sends the 33rd source in a second launch); scores_out = NULL; an item whose sequence is out of range
    gets label -1, moves nothing and leaves its neighbours alone"""
    rng = np.random.default_rng(7)
    nb, C, n, nseq = 33, 15, 6, 2
    preds = vc.random_preds(rng, nb, n, C)
    seq = np.array([0, 1, 0, 1, 1, 0], np.int32)
    acc, label, kept = vc.host_vote(hip_lib, preds, seq, nseq)
    want_acc, want_label = vc.longhand(preds, seq, nseq)
    assert vc.same_f64(acc, want_acc) and np.array_equal(label, want_label)
    acc2, label2, none = vc.host_vote(hip_lib, preds, seq, nseq, keep_scores=False)
    assert none is None and vc.same_f64(acc2, acc) and np.array_equal(label2, label)
    for bad_value in (-1, nseq, 0x7fffffff, -0x80000000):
        bad = seq.copy()
        bad[2] = bad_value
        keep = np.array([0, 1, 3, 4, 5])
        acc3, label3, kept3 = vc.host_vote(hip_lib, preds, bad, nseq)
        ref_acc, ref_label = vc.longhand([p[keep] for p in preds], seq[keep], nseq)
        assert np.all(label3[:, 2] == -1) and np.array_equal(label3[:, keep], ref_label) and vc.same_f64(acc3, ref_acc)
        assert np.all(kept3[:, 2] == np.float32(-777.125)) and vc.same_f32(kept3[:, keep], kept[:, keep])


# ---- refusals and the C-ABI -------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    from deephar_amd import _lib
    lib = hip_lib

    def vote(p=FAKE, stride=15, nsrc=2, nb=2, C=15, seq=FAKE, n=4, nseq=3, acc=FAKE, label=FAKE, scores=FAKE, srcs=True):
        table = (_lib.VoteSrc * nsrc)(*[_lib.VoteSrc(p, stride) for _ in range(nsrc)]) if srcs else None
        a = (table, nb, C, seq, n, nseq, acc, label, scores)
        host, dev = lib.dh_vote_products_host(*a), lib.dh_vote_products_f64(*a, None)
        assert host == dev                                                   # refused before anything is read or enqueued
        return host

    big = (1 << 40) + 1
    for kw in [dict(srcs=False), dict(p=None), dict(seq=None), dict(acc=None), dict(label=None),
               dict(p=FAKE + 2), dict(p=FAKE + 1), dict(seq=FAKE + 2), dict(acc=FAKE + 4), dict(label=FAKE + 1), dict(scores=FAKE + 2),
               dict(nb=0), dict(nb=-1), dict(C=0), dict(C=-15), dict(n=0), dict(n=-4), dict(nseq=0), dict(nseq=-3),
               dict(stride=14), dict(stride=0), dict(stride=-15), dict(stride=big),
               dict(n=0x7fffffff, stride=1 << 40),                           # (n - 1) * item_stride above 2^58
               dict(nseq=0x7fffffff, C=0x7fffffff), dict(n=0x7fffffff, C=0x7fffffff, stride=0x7fffffff)]:   # tables above 2^58
        assert vote(**kw) == DH_EINVAL, kw


def test_c_abi_lists_the_new_symbols(hip_lib):
    from deephar_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deephar_hip.h')).read()
    for name in ('dh_vote_products_f64', 'dh_vote_products_host'):
        assert name in _lib.SIGNATURES and 'int %s(' % name in header, name
        assert getattr(hip_lib, name).argtypes == _lib.SIGNATURES[name][1]
    f64, host = _lib.SIGNATURES['dh_vote_products_f64'][1], _lib.SIGNATURES['dh_vote_products_host'][1]
    assert f64[:-1] == host and len(f64) == len(host) + 1                    # exactly the stream more
    assert 'typedef struct dh_vote_src' in header
    import ctypes as C
    assert C.sizeof(_lib.VoteSrc) == 16


# ---- the box dictionary -> clip windows ------------------------------------------------------------------------------------
def test_compute_clip_bbox_and_clip_window_by_hand():
    from deephar_amd import evaltools
    from deephar_amd.evaltools import bbox
    assert evaltools.compute_clip_bbox is bbox.compute_clip_bbox and evaltools.clip_window is bbox.clip_window
    boxes = {'3.0': [100, 50, 300, 400], '3.1': [90, 60, 310, 390], '3.2': [120, 40, 280, 410], '4.0': [0, 0, 1, 1]}
    b = bbox.compute_clip_bbox(boxes, 3, [0, 1, 2])
    assert b.dtype == np.float64 and b.tolist() == [90.0, 40.0, 310.0, 410.0]
    assert bbox.compute_clip_bbox(boxes, 3, [1]).tolist() == [90.0, 60.0, 310.0, 390.0]
    with pytest.raises(KeyError):
        bbox.compute_clip_bbox(boxes, 3, [0, 3])
    with pytest.raises(KeyError):
        bbox.compute_clip_bbox(boxes, 5, [0])
    # centre (200, 225), window (220, 370): the box itself
    w = bbox.clip_window(b)
    assert w.dtype.kind == 'i' and w.tolist() == [90, 40, 310, 410]
    # an odd side: centre (100.5, 60), window (201, 100) -> corners 0, 10, 201, 110
    assert bbox.clip_window(np.array([0., 10., 201., 110.])).tolist() == [0, 10, 201, 110]
    # the 32-pixel floor: a (10, 200) box around (105, 200) becomes (32, 32) -- BOTH sides, as the loaders do
    assert bbox.clip_window(np.array([100., 100., 110., 300.])).tolist() == [89, 184, 121, 216]
    # a negative corner truncates toward zero: centre (2.5, 3), window (40, 33) -> -17.5, -13.5, 22.5, 19.5
    assert bbox.clip_window(np.array([-17.5, -13.5, 22.5, 19.5])).tolist() == [-17, -13, 22, 19]
    # the floor on a box around a corner of the image: centre (1, 1), window (32, 32) -> -15, -15, 17, 17
    assert bbox.clip_window(np.array([0., 0., 2., 2.])).tolist() == [-15, -15, 17, 17]


def test_vote_products_and_multiclip_votes_frames_argument_checks():
    from deephar_amd import evaltools
    from deephar_amd.evaltools import action
    assert evaltools.vote_products is action.vote_products and evaltools.multiclip_votes_frames is action.multiclip_votes_frames
    p = vc.softmax_rows(np.random.default_rng(0), 4, 5)
    with pytest.raises(ValueError):
        action.vote_products([p], [0, 1, 2, 3], 3)                           # a sequence outside [0, nseq)
    with pytest.raises(ValueError):
        action.vote_products([p], [0, -1, 0, 0], 3)
    with pytest.raises(ValueError):
        action.vote_products([p], [0, 1, 2], 3)                              # three sequence numbers for four items
    with pytest.raises(ValueError):
        action.vote_products([p, p[:, :4]], [0, 1, 2, 0], 3)
    with pytest.raises(ValueError):
        action.vote_products([], [], 3)
    acc, label = action.vote_products([p], [2, 2, 0, 2], 3)
    assert acc.shape == (1, 3, 5) and np.all(acc[0, 1] == 1.0) and label.shape == (1, 4)

    index = np.zeros((4, 2), np.int64)
    windows = np.tile(np.array([[0, 0, 32, 32]]), (4, 1))
    a_true = np.eye(5)[:2]
    good = dict(model=None, frames=None, index=index, windows=windows, hflip=[0, 1, 0, 1], seq=[0, 0, 1, 1], a_true=a_true,
                keys=['a', 'b', 'c', 'd'])
    for kw in [dict(loop='gpu'), dict(windows=windows[:3]), dict(hflip=[0, 1, 0]), dict(seq=[0, 0, 1]), dict(keys=['a', 'b', 'c']),
               dict(seq=[0, 0, 1, 2]), dict(seq=[0, 0, -1, 1]), dict(a_true=np.eye(5)[0]), dict(seq=[0., 0., 1., 1.])]:
        with pytest.raises(ValueError):
            action.multiclip_votes_frames(**dict(good, **kw))


def test_vote_outputs_picks_action_outputs():
    from types import SimpleNamespace as NS
    from deephar_amd import frontend
    outs = [NS(shape=(4, 16, 2)), NS(shape=(15,)), NS(shape=(15,)), NS(shape=(60,))]
    assert frontend.vote_outputs(outs, [1, 2]) == ([1, 2], 15)
    assert frontend.vote_outputs(outs, [-1]) == ([3], 60)
    assert frontend.vote_outputs(outs[1:3]) == ([0, 1], 15)
    for bad in ([0], [1, 3], [4], [], None):
        with pytest.raises(ValueError):
            frontend.vote_outputs(outs, bad)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
def test_vote_sweep_builds_and_passes(tmp_path):
    """tools/vote_sweep.cpp, the stand-alone sweep of the header (its own main(), nothing loaded into Python), built plainly and
    run: items, edge values and refusals in heap blocks of exactly their length.  Its sanitizer build (the command in the file's
    head) is run by hand on a CPU host; this keeps the sweep compiling and passing."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'vote_sweep')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'deephar_amd', 'csrc'),
                        os.path.join(ROOT, 'tools', 'vote_sweep.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'vote_sweep: ok' in r.stdout, r.stdout + r.stderr
