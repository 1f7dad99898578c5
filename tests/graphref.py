"""A generic interpreter of the graph IR (deephar_amd/graph.py) on torch-CPU, and the bar a fused plan is held to.  TEST
INFRASTRUCTURE.

The hand-written oracles (oracle/reception.py, oracle/spnet.py, oracle/action.py, tests/resample_ref.py) restate ONE model's
forward each.  `evaluate` walks any graph the public `layers` vocabulary can build, node by node, with the op statements of
oracle/ops.py -- nothing is fused, re-associated or viewed -- so whatever the planner makes of the graph can be compared with
it: float64 is the arbiter, float32 is "what plain fp32 does".  tests/test_graphref_host.py pins the interpreter to the
hand-written oracles.

The split-bf16 ladder inside the interpreter: evaluate(..., split=(parts, param_ids)) evaluates every dense convolution (a
`conv` node, the pointwise half of a `sepconv` node) and every `convtranspose` node whose weight Param is in `param_ids` as
E_parts of tests/bf16_modes_ref.py -- the operand it receives rounded to float32, both operands split into bf16 parts, exact
products.  `split_param_ids` reads the ids off a bound model: the fp64 interpreter then IS the mode the plan was bound with,
layer by layer (tests/test_synth_split_host.py, tests/test_gpu_synth_graphs_split.py).  Without the hook nothing changes.

What the IR does not record is derived: the bottom / right padding of a convolution or pooling from its output shape
(max((OH - 1) * sh + kh - H - pt, 0)); leading clip dims are folded into the batch.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import bf16_modes_ref as B
import paritylog
import resample_ref as R
from deephar_amd import graph as G
from deephar_amd.engine.packing import LAYOUTS
from oracle import ops

SKIPPABLE = ('bn', 'relu', 'scale', 'sigmoid', 'add')      # shape-preserving nodes `skip=` can turn into the identity
DECODER_OPS = ('expect2d', 'jointprob')      # the read-outs compare_decoder has a conditioned tolerance for
LAYER_COST = dict(conv=1, sepconv=2, convtranspose=1)
SPLIT_CODES = tuple(sorted(c for c, l in LAYOUTS.items() if l.parts))      # dh_conv_args.w_split of the split-bf16 packings


def _param(layer, role, dtype):
    for p in layer.params:
        if p.role == role:
            return torch.from_numpy(p.value).to(dtype)
    return None


def _parts(layer, role, split):
    """the number of bf16 parts the layer's `role` kernel is evaluated with under the hook `split`, 0 for plain arithmetic"""
    if split is None:
        return 0
    parts, ids = split
    return parts if any(p.role == role and id(p) in ids for p in layer.params) else 0


def _conv2d(x, kernel, strides, parts):
    if parts:
        return B.conv_ep(ops.conv2d, x, kernel, strides, 'valid', parts)
    return ops.conv2d(x, kernel, strides, 'valid')


def split_param_ids(m):
    """The weight Params of the convolution / transposed-convolution steps a BOUND model runs with a split-bf16 packing
    (attrs['w_split'] in SPLIT_CODES), as a set of id()s for evaluate(split=(parts, ids)); the parts of a merged
    convolution's ConcatParam each.  Call it after the first bind (a predict): the executor writes w_split when it binds."""
    ids = set()
    for s in m.plan.steps:
        if s.kind in ('conv', 'convtranspose') and s.attrs.get('w_split', 0) in SPLIT_CODES:
            w = s.params['w']
            ids.update(id(p) for p in getattr(w, 'parts', [w]))
    return ids


def _fold(x, nd):
    """[N, lead.., last nd dims] -> [N * lead, last nd dims]"""
    return x.reshape((-1,) + tuple(x.shape[-nd:]))


def _pad(x, a, out_shape, value=0.0):
    """explicit padding of a folded NHWC tensor for window (kh, kw) at stride (sh, sw): pt / pl from the attributes, the
    bottom / right amounts from the output extent"""
    h, w = x.shape[1], x.shape[2]
    oh, ow = out_shape[-3], out_shape[-2]
    pt, pl = a.get('pt', 0), a.get('pl', 0)
    pb = max((oh - 1) * a.get('sh', 1) + a['kh'] - h - pt, 0)
    pr = max((ow - 1) * a.get('sw', 1) + a['kw'] - w - pl, 0)
    if pt or pl or pb or pr:
        x = F.pad(x, (0, 0, pl, pr, pt, pb), value=value)
    return x


def _eval_node(node, xs, dtype, split=None):
    op, a = node.op, node.attrs
    shape = node.outputs[0].shape
    strides = (a.get('sh', 1), a.get('sw', 1))
    if op == 'conv':
        x = _pad(_fold(xs[0], 3), a, shape)
        return _conv2d(x, _param(node.layers['conv'], 'conv', dtype), strides, _parts(node.layers['conv'], 'conv', split))
    if op == 'sepconv':
        layer = node.layers['sepconv']
        x = _pad(_fold(xs[0], 3), a, shape)
        x = ops.depthwise_conv2d(x, _param(layer, 'depthwise', dtype), strides, 'valid')
        return _conv2d(x, _param(layer, 'conv', dtype), (1, 1), _parts(layer, 'conv', split))
    if op == 'convtranspose':
        x, k, parts = _fold(xs[0], 3), _param(node.layers['convt'], 'convt', dtype), _parts(node.layers['convt'], 'convt', split)
        if parts:        # (tests/test_gpu_convt_split.py: _convt)
            return B.conv_ep(lambda a_, k_, _s, _p: R.conv_transpose2x2(a_, k_), x, k, None, None, parts)
        return R.conv_transpose2x2(x, k)
    if op == 'bn':
        layer = node.layers['bn']
        return ops.batchnorm(xs[0], _param(layer, 'beta', dtype), _param(layer, 'mean', dtype), _param(layer, 'var', dtype),
                             gamma=_param(layer, 'gamma', dtype))
    if op == 'relu':
        return ops.relu(xs[0])
    if op == 'add':
        y = xs[0]
        for x in xs[1:]:
            y = y + x
        return y
    if op == 'mul':
        return xs[0] * xs[1]
    if op == 'scale':
        return a['k'] * xs[0]
    if op == 'sigmoid':
        return torch.sigmoid(xs[0])
    if op == 'concat':
        return torch.cat(xs, dim=-1)
    if op == 'slice':
        return xs[0][..., a['start']:a['stop']]
    if op == 'reshape':
        return xs[0]                                  # row-major view: the caller reshapes to the node's shape
    if op == 'pool':
        pool = (a['kh'], a['kw'])
        mp = lambda z: ops.maxpool2d(_pad(z, a, shape, -math.inf), pool, strides, 'valid')
        x = _fold(xs[0], 3)
        return mp(x) - mp(-x) if a.get('mode', 0) == 1 else mp(x)      # layers.max_min_pooling (ops.max_min_pooling)
    if op == 'upsample':
        return ops.upsample2d(_fold(xs[0], 3))
    if op == 'zeropad':
        x = _fold(xs[0], 3)
        pt, pl = a.get('pt', 0), a.get('pl', 0)
        return F.pad(x, (0, 0, pl, shape[-2] - x.shape[2] - pl, pt, shape[-3] - x.shape[1] - pt))
    if op == 'depthsum':                              # oracle/spnet.py, tests/resample_ref.py: (sigmoid(d) * h).sum over (H, W)
        return (torch.sigmoid(_fold(xs[0], 3)) * _fold(xs[1], 3)).sum(dim=(1, 2)).unsqueeze(-1)
    if op == 'softmax2d':
        return ops.channel_softmax_2d(_fold(xs[0], 3), a['alpha'])
    if op == 'expect2d':
        return ops.softargmax2d_from_prob(_fold(xs[0], 3))
    if op == 'jointprob':
        x = _fold(xs[0], 3)
        return ops.joints_probability(a['scale'] * x if a.get('scale', 1.0) != 1.0 else x)
    if op == 'globalmax2d':
        return torch.amax(_fold(xs[0], 3), dim=(1, 2))
    if op == 'globalmax1d':
        return torch.amax(_fold(xs[0], 2), dim=1)
    if op == 'depthmean':                             # oracle.reception.pose_regression_3d: channel c = d * J + j
        x = _fold(xs[0], 3)
        h5 = x.reshape(x.shape[0], x.shape[1], x.shape[2], a['D'], a['J'])
        return h5.mean(dim=3) if a['axis'] == 'd' else h5.mean(dim=(1, 2))
    if op == 'softargmax1d':
        return ops.softargmax1d(_fold(xs[0], 2))
    if op == 'context_agg':
        ys, yc, pc = (_fold(x, 2) for x in xs)
        return ops.context_aggregation(ys, yc, pc, ys.shape[1], a['nctx'], a['alpha'])
    if op == 'kronecker':
        return ops.kronecker_prod(xs[0], xs[1])
    if op == 'globalmaxmin':
        return ops.global_max_min_pooling(_fold(xs[0], 3))
    if op == 'softmax':
        return torch.softmax(xs[0], dim=-1)
    raise NotImplementedError('graphref: no statement for op %r' % op)


def evaluate(inputs, outputs, feeds, dtype, taps=None, skip=None, split=None):
    """Evaluate the graph inputs -> outputs on the arrays `feeds` ([N, ...] each) at `dtype`; one numpy array per output.
    taps (a dict) receives every tensor, the inputs included, by uid.  skip=<node>: that shape-preserving node (SKIPPABLE;
    an add is reduced to its first operand) is the identity -- the mutation the host test uses to show that the bar bites.
    split=(parts, param_ids): the layers whose weight Param is in param_ids (split_param_ids) are evaluated as E_parts, the
    split-bf16 mode with `parts` bf16 parts per operand; every other layer, and everything without the hook, as before."""
    if skip is not None and skip.op not in SKIPPABLE:
        raise ValueError('only %s nodes can be skipped, not %r' % ('/'.join(SKIPPABLE), skip.op))
    n = int(np.asarray(feeds[0]).shape[0])
    val = {}
    with torch.no_grad():
        for t, x in zip(inputs, feeds):
            val[t.uid] = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape((n,) + t.shape)
        for node in G.topo_nodes(outputs):
            xs = [val[t.uid] for t in node.inputs]
            y = xs[0] if node is skip else _eval_node(node, xs, dtype, split)
            val[node.outputs[0].uid] = y.reshape((n,) + node.outputs[0].shape)
    if taps is not None:
        taps.update({uid: v.numpy() for uid, v in val.items()})
    return [val[t.uid].numpy() for t in outputs]


def layers_on_longest_path(outputs):
    """L: the largest number of GEMM / depthwise layers on any input-to-output path (conv 1, sepconv 2, convtranspose 1)."""
    depth = {}
    for node in G.topo_nodes(outputs):
        d = max([depth.get(t.uid, 0) for t in node.inputs] + [0]) + LAYER_COST.get(node.op, 0)
        for o in node.outputs:
            depth[o.uid] = d
    return max([depth.get(t.uid, 0) for t in outputs] + [1])


def amplitude(taps64):
    """A = max(1, the largest |value| of any tensor of the fp64 evaluation)"""
    return max(1.0, max(float(np.abs(v).max()) for v in taps64.values() if v.size))


def bar(o64, taps64, L):
    """Per-element tolerance L * (3e-5 * A + 2e-5 * |o64|): the bar of tests/test_gpu_ops.py for ONE fused convolution (atol
    3e-5 + rtol 2e-5 at O(1) activations), added linearly over the L layers of the longest path as test_mini_pyramid argues;
    A scales it with the graph's largest activation.  Computed from the fp64 evaluation alone."""
    return L * (3e-5 * amplitude(taps64) + 2e-5 * np.abs(np.asarray(o64, np.float64)))


def compare(name, got, o32, o64, taps64, L, case=None, log=True, **extra):
    """|got - o64| <= bar element-wise, and max|got - o64| <= 4 * max|o32 - o64| + 1e-6 * A (the fp32-family clause of
    test_mini_pyramid / test_gpu_conv_views).  Prints and records (paritylog.record) both errors and the bar at the worst
    element (log=False: neither -- the host's mutation check).  Returns max(|got - o64| / bar)."""
    got, o32, o64 = (np.asarray(v, np.float64) for v in (got, o32, o64))
    assert got.shape == o64.shape, '%s: shape %s, reference %s' % (name, got.shape, o64.shape)
    A = amplitude(taps64)
    tol = bar(o64, taps64, L)
    err = np.abs(got - o64)
    finite = bool(np.all(np.isfinite(got)))
    worst = int(np.argmax(np.where(np.isfinite(err), err / tol, np.inf)))
    e_hip, e_cpu = float(err.max()) if finite else float('inf'), float(np.abs(o32 - o64).max())
    ratio = float(err.flat[worst] / tol.flat[worst]) if finite else float('inf')
    case = case or os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]
    if log:
        print('%-28s |got-o64|=%.3e  |o32-o64|=%.3e  bar there=%.3e  e/bar=%.3f  L=%d A=%.2f' % (
            name, e_hip, e_cpu, tol.flat[worst], ratio, L, A))
    if finite and log:
        paritylog.record(name, got, o32, o64, case, px=False, graphref=True, bar=float(tol.flat[worst]), ratio_to_bar=ratio,
                         layers=int(L), amplitude=A, **extra)
    assert finite, '%s: non-finite values' % name
    assert ratio <= 1.0, '%s: differs from the fp64 interpreter by %.3e where the bar is %.3e (L = %d, A = %.2f)' % (
        name, err.flat[worst], tol.flat[worst], L, A)
    assert e_hip <= 4 * e_cpu + 1e-6 * A, '%s: %.3e from fp64, the fp32 interpreter is %.3e from it' % (name, e_hip, e_cpu)
    return ratio


def is_decoder_output(t):
    """soft-argmax coordinates / confidences (and their product): held to paritylog.conditioned_tolerance, not to `bar`"""
    if t.node is not None and t.node.op == 'mul':
        return all(is_decoder_output(x) for x in t.node.inputs)
    return t.node is not None and t.node.op in DECODER_OPS


def decoder_logits(t, taps64):
    """the fp64 heat-map logits behind a decoder output (expect2d / jointprob of a channel soft-max, or jointprob of raw maps)"""
    src = t.node.inputs[0]
    if t.node.op == 'mul':
        src = src.node.inputs[0]
    if src.node is not None and src.node.op == 'softmax2d':
        src = src.node.inputs[0]
    x = taps64[src.uid]
    return x.reshape((-1,) + x.shape[-3:])


def compare_decoder(name, t, got, o32, o64, taps64):
    """coordinates and confidences of a read-out through paritylog.check_conditioned, as the SPNet tests do: the a-priori
    conditioned tolerance is REPORTED with the record, the assertion is check_conditioned's sanity bound.  The tolerance of a
    product (x, y) * c, tol_xy + tol_c, is this module's own and likewise only reported."""
    if t.node.op not in DECODER_OPS + ('mul',):
        raise NotImplementedError('no conditioned tolerance for a %r output' % t.node.op)
    tol_xy, _, tol_c = paritylog.conditioned_tolerance(decoder_logits(t, taps64))
    fold = lambda v: np.asarray(v).reshape((-1,) + tuple(np.asarray(v).shape[-2:]))
    if t.node.op == 'mul':          # (x, y) * c with x, y, c in [0, 1]: |d(x c)| <= |dx| + |dc|
        paritylog.check_conditioned(name, fold(got), fold(o32), fold(o64), tol_xy + tol_c)
    elif t.node.op == 'expect2d':
        paritylog.check_conditioned(name, fold(got), fold(o32), fold(o64), tol_xy)
    else:
        paritylog.check_conditioned(name, fold(got)[..., 0], fold(o32)[..., 0], fold(o64)[..., 0], tol_c, px=False)
