"""The launch arguments of a planner Step: pure arithmetic on shapes, pitches and offsets -- no torch, no device.

`bind(step, n, env)` -> (entry-point name, [ctypes structs], [trailing scalars]) through one small binder per Step.kind
(BINDERS).  Addresses come from `env`: env.ptr(value) (an arena address), env.affine(layer) -> (scale ptr, shift ptr),
env.constant(key, make) -> ptr, env.dw_weight(param) -> ptr, env.u8_input(buf) -> (byte ptr, lut ptr) or None when that input
is not normalised on load.  executor.BoundPlan is the env over a device arena and a WeightStore, FakeEnv the one of the host
tests.  The conv / convtranspose binders leave `w` (and `w_split`) unset: every other field is final, which is the state in
which the library's eligibility rules are asked (weight_layout, convt_weight_layout) before a weight is packed.
"""
import ctypes as C

import numpy as np

from .. import _lib
from . import packing


def grid_x(w):
    """float32 x grid of utils/math.py:6-19 (np.linspace(0,1,W) stored into a float32 array)."""
    return np.linspace(0.0, 1.0, num=w).astype(np.float32)


def grid_depth(d):
    """layers.py:141-143: linspace(1/(2D), 1-1/(2D), D) stored in float32 Conv1D weights."""
    s = 1 / (2 * d)
    return np.linspace(s, 1 - s, num=d).astype(np.float32)


class FakeEnv:
    """The host-test environment: an arena for n frames at `base` (16-byte aligned, as torch's allocations are) and every
    table (BN affine, constant, depthwise kernel) at a fake address of its own, k << 20 for k = 1, 2, ... (`tables`)."""

    def __init__(self, n, base=256):
        self.n, self.base, self.tables = n, base, {}

    def _table(self, key):
        return self.tables.setdefault(key, (len(self.tables) + 1) << 20)

    def ptr(self, v):
        return self.base + 4 * (v.buf.offset * self.n + v.coff)

    def affine(self, layer):
        return self._table(('scale', id(layer))), self._table(('shift', id(layer)))

    def constant(self, key, make):
        return self._table(key)

    def dw_weight(self, p):
        return self._table(('dw', id(p)))

    def u8_input(self, buf):
        return None


def bind(s, n, env):
    if s.kind not in BINDERS:
        raise NotImplementedError('no binding for step kind %r' % s.kind)
    return BINDERS[s.kind](s, n, env)


def _opt(env, v):
    return env.ptr(v) if v is not None else None


def _view(env, args, v, field, ld):
    """an operand that may be absent: its address and its pixel pitch"""
    if v is not None:
        setattr(args, field, env.ptr(v))
        setattr(args, ld, v.ld)


def _pre_bn(s, args, env):
    if 'pre_bn' in s.params:
        args.pre_scale, args.pre_shift = env.affine(s.params['pre_bn'])


def _packed_dims(kh, kw, cin, cout):
    kp, np_ = C.c_int(), C.c_int()
    _lib.check(_lib.load().dh_conv2d_packed_dims(kh, kw, cin, cout, C.byref(kp), C.byref(np_)))
    return kp.value, np_.value


def _conv(s, n, env):
    a, x, y, P = s.attrs, s.ins['x'], s.outs['y'], env.ptr
    args = _lib.ConvArgs()
    args.x, args.y = P(x), P(y)
    _pre_bn(s, args, env)
    if 'post_bn' in s.params or 'post_affine' in s.params:
        args.post_scale, args.post_shift = env.affine(s.params.get('post_bn') or s.params['post_affine'])
    up = 2 if a['up2'] else 1
    args.N = n * x.lead(3)
    args.H, args.W, args.Cin, args.ldx = x.shape[-3], x.shape[-2], x.C, x.ld
    sg = a.get('seg')                          # planner rule R14: x = [MaxPooling2D(x) | x2], read in place
    if sg is not None:                         # (H, W: the extent the convolution sees; Cin: both segments)
        args.H, args.W, args.Cin = x.shape[-3] // sg['pool_sh'], x.shape[-2] // 2, a['Cin']
    rs = a.get('x_resample', 0)                # planner rule R12: x is stored at another resolution than the conv sees
    if rs:
        args.x_resample = rs
        args.H, args.W = (2 * x.shape[-3], 2 * x.shape[-2]) if rs == 1 else (x.shape[-3] // 2, x.shape[-2] // 2)
    args.OH, args.OW, args.Cout, args.ldy = y.shape[-3] // up, y.shape[-2] // up, a['Cout'], y.ld
    args.KH, args.KW, args.SH, args.SW, args.PT, args.PL = a['kh'], a['kw'], a['sh'], a['sw'], a['pt'], a['pl']
    args.K, (args.Kp, args.Np) = a['K'], _packed_dims(a['kh'], a['kw'], args.Cin, a['Cout'])
    _view(env, args, s.ins.get('res1'), 'res1', 'ldr1')
    _view(env, args, s.ins.get('res2'), 'res2', 'ldr2')
    args.pre_relu, args.post_relu, args.up2 = a['pre_relu'], a['post_relu'], a['up2']
    args.res2_down = a.get('res2_down', 0)
    _view(env, args, s.outs.get('ypool'), 'y_pool', 'ldyp')        # planner rule R7: the 2x2 max-pooled second output
    u8 = env.u8_input(x.buf)
    if u8 is not None:
        (args.x, args.in_lut), args.x_u8 = u8, 1
    if sg is None:
        return 'dh_conv2d_f32', [args], [a.get('tile_cfg', -1)]
    seg = _lib.ConvSeg()
    _view(env, seg, s.ins.get('x2'), 'x2', 'ldx2')
    seg.c_split, seg.pool_sh = sg['c_split'], sg['pool_sh']
    return 'dh_conv2d_seg_f32', [args, seg], []


def _convtranspose(s, n, env):
    a, x, y = s.attrs, s.ins['x'], s.outs['y']     # Conv2DTranspose((2, 2), strides=(2, 2)): the fp32 launch (the split one: BoundPlan._bind)
    args = _lib.ConvtArgs()
    args.x, args.y = env.ptr(x), env.ptr(y)
    _pre_bn(s, args, env)
    _view(env, args, s.ins.get('res1'), 'res', 'ldr')
    args.N, args.H, args.W, args.Cin, args.ldx = n * x.lead(3), x.shape[-3], x.shape[-2], x.C, x.ld
    args.Cout, args.ldy, (args.Kp, args.Np) = a['Cout'], y.ld, _packed_dims(1, 1, x.C, 4 * a['Cout'])
    args.pre_relu, args.post_relu = a['pre_relu'], a['post_relu']
    return 'dh_conv2d_transpose2x2_f32', [args], [a.get('tile_cfg', -1)]


def _dwconv(s, n, env):
    a, x, y = s.attrs, s.ins['x'], s.outs['y']
    strided = (a.get('sh', 1), a.get('sw', 1)) != (1, 1)       # the depthwise half of a strided SeparableConv2D
    args = _lib.DwsArgs() if strided else _lib.DwArgs()
    args.x, args.w, args.y = env.ptr(x), env.dw_weight(s.params['w']), env.ptr(y)
    _pre_bn(s, args, env)
    args.ldx, args.ldy, args.pre_relu = x.ld, y.ld, a['pre_relu']
    if strided:
        args.N, args.H, args.W, args.C = n * x.lead(3), x.shape[-3], x.shape[-2], x.C
        args.OH, args.OW = y.shape[-3], y.shape[-2]
        args.KH, args.KW, args.SH, args.SW, args.PT, args.PL = a['kh'], a['kw'], a['sh'], a['sw'], a['pt'], a['pl']
        return 'dh_dwconv2d_strided_f32', [args], []
    args.N, args.H, args.W, args.C = n * y.lead(3), y.shape[-3], y.shape[-2], x.C      # (up_in: x is at half resolution)
    args.KH, args.KW, args.PT, args.PL, args.up_in = a['kh'], a['kw'], a['pt'], a['pl'], a.get('up_in', 0)
    return 'dh_dwconv2d_f32', [args], []


def _pool(s, n, env):
    a, x, y = s.attrs, s.ins['x'], s.outs['y']
    args = _lib.PoolArgs()
    args.x, args.y = env.ptr(x), env.ptr(y)
    args.N, args.H, args.W, args.C, args.ldx = n * x.lead(3), x.shape[-3], x.shape[-2], x.C, x.ld
    args.OH, args.OW, args.ldy = y.shape[-3], y.shape[-2], y.ld
    args.KH, args.KW, args.SH, args.SW, args.PT, args.PL = a['kh'], a['kw'], a['sh'], a['sw'], a['pt'], a['pl']
    args.mode = a.get('mode', 0)
    return 'dh_pool2d_f32', [args], []


def _upsample_add(s, n, env):
    av, b, y = s.ins.get('a'), s.ins['b'], s.outs['y']
    return 'dh_upsample2x_add_f32', [], [_opt(env, av), av.ld if av is not None else 0, env.ptr(b), b.ld, env.ptr(y), y.ld,
                                         n * y.lead(3), y.shape[-3], y.shape[-2], y.C]


def _eltwise(s, n, env):
    a, av, y = s.attrs, s.ins['a'], s.outs['y']
    args = _lib.EltArgs()
    args.a, args.y, args.lda, args.ldy = env.ptr(av), env.ptr(y), av.ld, y.ld
    _view(env, args, s.ins.get('b'), 'b', 'ldb')
    _view(env, args, s.ins.get('c'), 'c', 'ldc')
    if 'bn' in s.params:
        args.scale, args.shift = env.affine(s.params['bn'])
    elif 'scale_const' in a:
        kc, cc = a['scale_const'], av.C
        args.scale = env.constant(('const', kc, cc), lambda: np.full(cc, kc, np.float32))
        args.shift = env.constant(('const', 0.0, cc), lambda: np.zeros(cc, np.float32))
    args.npix, args.C = n * av.npix, av.C
    args.relu, args.op, args.bcast_b = a.get('relu', 0), a.get('op', 0), a.get('bcast_b', 0)
    return 'dh_eltwise_f32', [args], []


def _sam_args(h, n, env, alpha, conf_scale, conf_raw):
    """what `sam` and `sam_ctx` share: the heat maps, the grids, the raw confidence output"""
    H, W = h.shape[-3], h.shape[-2]
    args = _lib.SamArgs()
    args.h = env.ptr(h)
    args.gx = env.constant(('gx', W), lambda: grid_x(W))
    args.gy = env.constant(('gx', H), lambda: grid_x(H))
    _view(env, args, conf_raw, 'conf_raw', 'ldcr')
    args.F, args.H, args.W, args.C, args.ldh = n * h.lead(3), H, W, h.C, h.ld
    args.alpha, args.conf_scale = alpha, conf_scale
    return args


def _sam(s, n, env):
    a, o = s.attrs, s.outs
    args = _sam_args(s.ins['h'], n, env, a['alpha'], a['conf_scale'], o.get('conf_raw'))
    _view(env, args, o.get('xy'), 'xy', 'ldxy')
    _view(env, args, o.get('conf_prob'), 'conf_prob', 'ldcp')
    _view(env, args, o.get('prob'), 'prob', 'ldp')
    if o.get('gmax') is not None:
        assert o['gmax'].dense
        args.gmax = env.ptr(o['gmax'])
    args.xy_times_conf = a.get('xy_times_conf', 0)
    return 'dh_softargmax2d_f32', [args], []


def _sam_ctx(s, n, env):
    a, y = s.attrs, s.outs['y']
    args = _sam_args(s.ins['h'], n, env, a['sam_alpha'], a['conf_scale'], s.outs.get('conf_raw'))
    return 'dh_softargmax2d_context_f32', [args], [a['J'], a['nctx'], a['alpha'], env.ptr(y), y.ld]


def _context_agg(s, n, env):
    P, ys, y = env.ptr, s.ins['ys'], s.outs['y']
    return 'dh_context_aggregation_f32', [], [P(ys), P(s.ins['yc']), P(s.ins['pc']), P(y), n * ys.lead(2), ys.shape[-2],
                                              s.attrs['nctx'], s.attrs['alpha'], y.ld]


def _depth_means(s, n, env):
    h = s.ins['h']
    return 'dh_depth_means_f32', [], [env.ptr(h), h.ld, _opt(env, s.outs.get('hxy')), _opt(env, s.outs.get('hz')),
                                      n * h.lead(3), h.shape[-3] * h.shape[-2], s.attrs['D'], s.attrs['J']]


def _softargmax1d(s, n, env):
    hz, z = s.ins['hz'], s.outs.get('z')
    D, J = hz.shape[-2], hz.shape[-1]
    return 'dh_softargmax1d_f32', [], [env.ptr(hz), env.constant(('gd', D), lambda: grid_depth(D)), _opt(env, z),
                                       z.ld if z is not None else 1, _opt(env, s.outs.get('vz')), n * hz.lead(2), D, J]


def _kronecker(s, n, env):
    P, hm, x, y = env.ptr, s.ins['hm'], s.ins['x'], s.outs['y']
    return 'dh_kronecker_f32', [], [P(hm), hm.ld, P(x), x.ld, P(y), y.ld, n * hm.lead(3), hm.shape[-3] * hm.shape[-2],
                                    hm.C, x.C]


def _globalmaxmin(s, n, env):
    x, y = s.ins['x'], s.outs['y']
    return 'dh_global_maxmin_softmax_f32', [], [env.ptr(x), x.ld, env.ptr(y), n * x.lead(3), x.shape[-3] * x.shape[-2], x.C,
                                                s.attrs['softmax']]


def _copy(s, n, env):
    x, y = s.ins['x'], s.outs['y']
    return 'dh_copy_channels_f32', [], [env.ptr(x), x.ld, env.ptr(y), y.ld, n * x.npix, x.C]


def _zeropad(s, n, env):
    a, x, y = s.attrs, s.ins['x'], s.outs['y']
    return 'dh_zeropad2d_f32', [], [env.ptr(x), env.ptr(y), n * x.lead(3), x.shape[-3], x.shape[-2], x.C, y.shape[-3],
                                    y.shape[-2], a.get('pt', 0), a.get('pl', 0)]


def _depthsum(s, n, env):
    P, d, h, z = env.ptr, s.ins['d'], s.ins['h'], s.outs['z']
    return 'dh_depth_from_maps_f32', [], [P(d), d.ld, P(h), h.ld, P(z), z.ld, n * d.lead(3), d.shape[-3] * d.shape[-2], d.C]


BINDERS = {'conv': _conv, 'convtranspose': _convtranspose, 'dwconv': _dwconv, 'pool': _pool, 'upsample_add': _upsample_add,
           'eltwise': _eltwise, 'sam': _sam, 'sam_ctx': _sam_ctx, 'context_agg': _context_agg, 'depth_means': _depth_means,
           'softargmax1d': _softargmax1d, 'kronecker': _kronecker, 'globalmaxmin': _globalmaxmin, 'copy': _copy,
           'zeropad': _zeropad, 'depthsum': _depthsum}


# ---- which packing a weight is bound with ------------------------------------------------------------------------------------
def weight_layout(lib, plan, args):
    """dh_conv_args.w_split of a conv step (packing.LAYOUTS): 1 / 3 / 4 = split-bf16 (plan.gemm_precision == 'bf16x3' / 'bf16x2'
    / 'bf16' and the library takes the layer: dh_conv2d_split_eligible, one rule for the three), 2 = fp32 chunk-major for the
    halo-resident K x K kernel (dh_conv2d_halo_eligible: a rule on the per-frame geometry), else 0.  The LIBRARY decides, asked
    with the launch's own argument struct before the weights are packed -- a layer is never bound with a packing its launch
    rejects.  Under plan.gemm_scope == 'extended' the wider rule is asked instead (dh_conv2d_split_wide_eligible) and the layer
    is bound with the extended scope's code, 5 / 6 / 7; a layer it refuses falls to halo / fp32 as under 'standard'."""
    wide = getattr(plan, 'gemm_scope', 'standard') == 'extended'
    code = packing.LAYOUT_CODES['extended' if wide else 'standard'].get(getattr(plan, 'gemm_precision', 'f32'))
    if code and (lib.dh_conv2d_split_wide_eligible if wide else lib.dh_conv2d_split_eligible)(C.byref(args)):
        return code
    if plan.rules.halo_conv and lib.dh_conv2d_halo_eligible(C.byref(args)):
        return 2
    return 0


def convt_weight_layout(lib, plan, args):
    """The same for a convtranspose step: the split-bf16 form (1 / 3 / 4 under either scope) when the library takes the layer
    (dh_conv2d_transpose2x2_split_eligible, one rule for the three modes), else 0: the fp32 kernel."""
    code = packing.LAYOUT_CODES['standard'].get(getattr(plan, 'gemm_precision', 'f32'), 0)
    return code if code and lib.dh_conv2d_transpose2x2_split_eligible(C.byref(args)) else 0


def conv_signature(step):
    a, x, y = step.attrs, step.ins['x'], step.outs['y']
    r1, r2 = step.ins.get('res1'), step.ins.get('res2')
    # the 16-byte alignment of every view decides which kernels / epilogues are eligible (gemm1x1_eligible, the
    # vector epilogue), so it is part of the identity of a tuned shape -- as are padding and the output size
    align = (x.coff % 4, y.coff % 4, r1.coff % 4 if r1 is not None else 0, r2.coff % 4 if r2 is not None else 0,
             r1.ld % 4 if r1 is not None else 0, r2.ld % 4 if r2 is not None else 0)
    return (x.lead(3), x.shape[-3], x.shape[-2], x.C, x.ld, y.ld, a['Cout'], a['kh'], a['kw'], a['sh'],
            a['sw'], a['pre_relu'], a['post_relu'], a['up2'], 'res1' in step.ins, 'res2' in step.ins,
            'pre_bn' in step.params, 'post_bn' in step.params or 'post_affine' in step.params, a['pt'], a['pl'], y.shape[-3], y.shape[-2], a.get('res2_down', 0), 'ypool' in step.outs) + align
