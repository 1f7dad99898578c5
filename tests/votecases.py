"""Cases of the multi-clip action vote (csrc/vote_index.h), shared by tests/test_vote_host.py and tests/test_gpu_vote.py: random
soft-max rows, hand-made edge items with the labels worked out by hand, the ctypes call of the host twin, and a long-hand
scalar restatement (Python floats are IEEE doubles; its arg-max is spelled out, not np.argmax).  GPU-free."""
import ctypes as C
import math

import numpy as np

F32 = np.float32


def softmax_rows(rng, n, C_):
    """float32 [n, C]: the soft-max of random logits"""
    logits = rng.normal(0.0, 2.0, (n, C_))
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(F32)


def random_preds(rng, nb, n, C_):
    return [softmax_rows(rng, n, C_) for _ in range(nb)]


def sequences(counts, flips=2):
    """the reference's item order for sequences of counts[i] clips: per sequence, clip-major, flip fastest.
    Returns (seq int32 [N], keys: the '%04d.%03d.%d' strings)"""
    seq, keys = [], []
    for i, c in enumerate(counts):
        for f in range(c):
            for h in range(flips):
                seq.append(i)
                keys.append('%04d.%03d.%d' % (i, f, h))
    return np.array(seq, np.int32), keys


def edge_cases():
    """(name, preds: one float32 [n, C] array, seq, nseq, the labels worked out by hand)"""
    nan, inf = np.nan, np.inf
    z = np.zeros
    cases = []
    # exact ties: the first index wins; then class 1 pulls ahead
    cases.append(('ties', np.array([[.25, .25, .25, .25], [.5, .5, .25, .25], [.5, 1., 1., 1.]], F32), z(3, np.int32), 1, [0, 0, 1]))
    # (2, 3, 4)e-38 per item (normal float32): (2.6e-302, 6.6e-301, 6.6e-300) after eight items, times 1e-10 SUBNORMAL in every
    # class (2.6e-312 .. 6.6e-310, class 2 the largest), then zero in every class -- a tie of zeros, class 0
    tiny = np.tile(np.array([[2e-38, 3e-38, 4e-38]], F32), (8, 1))
    rows = np.concatenate([tiny, np.array([[1e-10, 1e-10, 1e-10]], F32), np.array([[2e-38, 3e-38, 4e-38]], F32)])
    cases.append(('subnormal_then_zero', rows, z(10, np.int32), 1, [2] * 9 + [0]))
    # a float32 input that is itself subnormal converts exactly
    cases.append(('subnormal_input', np.array([[1e-40, 2e-40], [1., .25]], F32), z(2, np.int32), 1, [1, 0]))
    # a NaN in the middle beats every number; a NaN in a lower class later is the first NaN
    cases.append(('nan_then_lower_nan', np.array([[.1, .2, nan, .4], [.3, .5, .5, .5], [nan, .5, .5, .5]], F32), z(3, np.int32), 1,
                  [2, 2, 0]))
    # inf * 0 = NaN in classes 0 and 2: the first NaN; class 3 stays a number
    cases.append(('inf_times_zero', np.array([[inf, 1., 0., .5], [0., 1., inf, 2.]], F32), z(2, np.int32), 1, [0, 0]))
    # inf beats every number but not a NaN behind it (np.argmax([inf, nan]) == 1)
    cases.append(('inf_then_nan', np.array([[inf, nan]], F32), z(1, np.int32), 1, [1]))
    # negative inputs: [-.5, -.25, -1, -2] -> 1; times [-1, -1, -3, 0] = [.5, .25, 3, -0] -> 2
    cases.append(('negative', np.array([[-.5, -.25, -1., -2.], [-1., -1., -3., 0.]], F32), z(2, np.int32), 1, [1, 2]))
    # +0 and -0 are equal: np.argmax([0.0, -0.0]) == 0; and [-0.0, 0.0] as well
    cases.append(('signed_zeros', np.array([[0., -0.], [-1., -1.]], F32), z(2, np.int32), 1, [0, 0]))
    # one class: always label 0, a NaN included
    cases.append(('one_class', np.array([[.5], [nan], [2.]], F32), np.array([0, 1, 0], np.int32), 2, [0, 0, 0]))
    # two sequences interleaved: the rows of one never touch the other
    cases.append(('interleaved', np.array([[.1, .9], [.8, .2], [.9, .1], [.5, .5]], F32), np.array([0, 1, 0, 1], np.int32), 2,
                  [1, 0, 0, 0]))
    return cases


def pointer(a):
    return a.ctypes.data if a is not None else None


def sources(preds):
    """the dh_vote_src table of float32 arrays [n, C] (any row stride, unit class stride: views of wider slabs are read in place)"""
    from deephar_amd import _lib
    table = (_lib.VoteSrc * len(preds))()
    for b, p in enumerate(preds):
        assert p.dtype == F32 and p.ndim == 2 and (p.shape[1] == 1 or p.strides[1] == 4) and p.strides[0] % 4 == 0
        table[b].p = p.ctypes.data
        table[b].item_stride = max(p.strides[0] // 4, p.shape[1]) if p.shape[0] > 1 else p.shape[1]
    return table


def host_vote(lib, preds, seq, nseq, acc=None, keep_scores=True):
    """dh_vote_products_host -> (acc float64 [nb, nseq, C] -- `acc` itself when given, multiplied in place --, label int32
    [nb, n], scores float32 [nb, n, C] or None)"""
    nb, (n, C_) = len(preds), preds[0].shape
    seq = np.ascontiguousarray(seq, np.int32)
    if acc is None:
        acc = np.ones((nb, nseq, C_))
    label = np.full((nb, n), -7, np.int32)
    scores = np.full((nb, n, C_), -777.125, F32) if keep_scores else None
    rc = lib.dh_vote_products_host(sources(preds), nb, C_, pointer(seq), n, nseq, pointer(acc), pointer(label), pointer(scores))
    assert rc == 0, rc
    return acc, label, scores


def longhand_argmax(row):
    """np.argmax's rule spelled out: the first NaN if any, else the first maximum"""
    best = 0
    for c in range(len(row)):
        if math.isnan(row[c]):
            return c
        if row[c] > row[best]:
            best = c
    return best


def longhand(preds, seq, nseq, acc=None):
    """the scalar loop: one Python float multiply per class, in item order -> (acc, label)"""
    nb, (n, C_) = len(preds), preds[0].shape
    acc = np.ones((nb, nseq, C_)) if acc is None else acc.copy()
    label = np.zeros((nb, n), np.int32)
    for k in range(n):
        s = int(seq[k])
        for b in range(nb):
            row = [float(acc[b, s, c]) * float(preds[b][k, c]) for c in range(C_)]
            for c in range(C_):
                acc[b, s, c] = row[c]
            label[b, k] = longhand_argmax(row)
    return acc, label


def same_f64(a, b):
    """bit for bit where both are numbers, a NaN where the other has one (the bits of a NaN are the platform's)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def same_f32(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))
