"""Host-side weight re-layout for the gfx950 kernels (delegates to the C-ABI so that other hosts get the
exact same packing: dh_conv2d_pack_weights_host)."""
import collections
import ctypes as C

import numpy as np

from .. import _lib


def pack_conv(w_hwio):
    """Keras HWIO conv kernel [kh,kw,cin,cout] -> ([Kp/4][Np][4] float32 flat array, Kp, Np)."""
    lib = _lib.load()
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    kh, kw, cin, cout = w.shape
    kp, np_ = C.c_int(), C.c_int()
    _lib.check(lib.dh_conv2d_packed_dims(kh, kw, cin, cout, C.byref(kp), C.byref(np_)), 'packed_dims')
    out = np.empty(kp.value * np_.value, dtype=np.float32)
    _lib.check(lib.dh_conv2d_pack_weights_host(w.ctypes.data, out.ctypes.data, kh, kw, cin, cout), 'pack')
    return out, kp.value, np_.value


def convt_matrix(w):
    """Keras Conv2DTranspose kernel [2, 2, Cout, Cin] -> the [1, 1, Cin, 4 * Cout] pointwise kernel of the GEMM
    dh_conv2d_transpose2x2_f32 runs: column (2 a + b) * Cout + co holds W[a, b, co, :]."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    kh, kw, cout, cin = w.shape
    if (kh, kw) != (2, 2):
        raise ValueError('only 2x2 transposed-convolution kernels are packed, got %dx%d' % (kh, kw))
    return np.ascontiguousarray(w.transpose(3, 0, 1, 2)).reshape(1, 1, cin, 4 * cout)


def pack_convt(w, parts=None):
    """Keras Conv2DTranspose kernel [2, 2, Cout, Cin] -> ([Kp/4][Np][4] float32, Kp, Np): the [Cin, 4 * Cout] B operand
    through the pointwise packer; the four column blocks are contiguous, the padding to Np follows the last one.
    parts = 3 / 2 / 1: the same matrix through the split-bf16 packer (pack_conv_split: [Kp/8][parts][Np][8] bf16, as a
    float32-typed array) for dh_conv2d_transpose2x2_split_f32; None: the fp32 packing."""
    if parts is None:
        return pack_conv(convt_matrix(w))
    return pack_conv_split(convt_matrix(w), parts=parts)


HALO_CHUNK = 16      # channels per resident chunk of csrc/conv_halo.hip


def halo_order(w_hwio):
    """HWIO kernel -> the [1, 1, K, Cout] kernel whose K runs chunk-major, [Cin/16][KH][KW][16], the order in which the
    halo-resident K x K kernel sums (dh_conv_args.w_split = 2, include/deephar_hip.h: dh_conv2d_halo_eligible)."""
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    kh, kw, cin, cout = w.shape
    if cin % HALO_CHUNK:
        raise ValueError('chunk-major packing needs Cin %% %d == 0, got %d' % (HALO_CHUNK, cin))
    w = w.reshape(kh, kw, cin // HALO_CHUNK, HALO_CHUNK, cout).transpose(2, 0, 1, 3, 4)
    return np.ascontiguousarray(w).reshape(1, 1, kh * kw * cin, cout)


def pack_conv_halo(w_hwio):
    """Keras HWIO conv kernel -> ([Kp/4][Np][4] float32, Kp, Np) with K chunk-major (see halo_order)."""
    return pack_conv(halo_order(w_hwio))


def unpack_conv(packed, kh, kw, cin, cout):
    """Inverse of pack_conv (tests)."""
    k = kh * kw * cin
    kp = (k + 31) // 32 * 32
    np_ = (cout + 31) // 32 * 32
    a = packed.reshape(kp // 4, np_, 4).transpose(0, 2, 1).reshape(kp, np_)
    return a[:k, :cout].reshape(kh, kw, cin, cout)


Layout = collections.namedtuple('Layout', 'mode scope parts base')
# THE vocabulary of dh_conv_args.w_split (include/deephar_hip.h): code -> the mode's name (Plan.gemm_precision; 'halo': the fp32
# chunk-major packing of the halo-resident K x K kernel), the Plan.gemm_scope it is bound under (None: either), the bf16 parts
# per operand (None: an fp32 packing) and the code whose packed bytes it shares.  Every other table is derived from this one.
LAYOUTS = {
    0: Layout('f32', None, None, 0),
    2: Layout('halo', None, None, 2),
    1: Layout('bf16x3', 'standard', 3, 1), 3: Layout('bf16x2', 'standard', 2, 3), 4: Layout('bf16', 'standard', 1, 4),
    5: Layout('bf16x3', 'extended', 3, 1), 6: Layout('bf16x2', 'extended', 2, 3), 7: Layout('bf16', 'extended', 1, 4),
}
LAYOUT_MODE = {code: l.mode for code, l in LAYOUTS.items()}
LAYOUT_CODES = {scope: {l.mode: code for code, l in LAYOUTS.items() if l.scope == scope} for scope in ('standard', 'extended')}
MODE_PARTS = {l.mode: l.parts for l in LAYOUTS.values() if l.parts}              # gemm_precision -> bf16 parts per operand
SPLIT_PARTS = {code: l.parts for code, l in LAYOUTS.items() if l.scope == 'standard'}
WIDE_SPLIT_PARTS = {code: l.parts for code, l in LAYOUTS.items() if l.scope == 'extended'}    # the packings of 1 / 3 / 4
WIDE_SPLIT_BASE = {code: l.base for code, l in LAYOUTS.items() if l.scope == 'extended'}      # ... byte for byte


def pack_conv_split(w_hwio, parts=3):
    """Keras HWIO conv kernel -> split-bf16 packing for dh_conv_args.w_split = 1 / 3 / 4 (parts = 3 / 2 / 1): every
    weight as `parts` bf16 parts by repeated round-to-nearest-even (w1 = bf16(w), w2 = bf16(w - w1), w3 = bf16(w - w1 - w2);
    exact for three: w = w1 + w2 + w3), laid out [Kp/8][parts][Np][8]; returned as a float32-typed flat array of
    parts / 2 * Kp * Np words (the bf16 bit patterns, two per word), Kp, Np.  Delegates to
    dh_conv2d_pack_weights_parts_host (parts = 3: dh_conv2d_pack_weights_split_host, the same bytes)."""
    if parts not in (1, 2, 3):
        raise ValueError('parts must be 1, 2 or 3, got %r' % (parts,))
    lib = _lib.load()
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    kh, kw, cin, cout = w.shape
    kp, np_ = C.c_int(), C.c_int()
    _lib.check(lib.dh_conv2d_packed_dims(kh, kw, cin, cout, C.byref(kp), C.byref(np_)), 'packed_dims')
    out = np.empty(parts * kp.value * np_.value, dtype=np.uint16)
    if parts == 3:
        _lib.check(lib.dh_conv2d_pack_weights_split_host(w.ctypes.data, out.ctypes.data, kh, kw, cin, cout), 'pack split')
    else:
        _lib.check(lib.dh_conv2d_pack_weights_parts_host(w.ctypes.data, out.ctypes.data, kh, kw, cin, cout, parts),
                   'pack parts')
    return out.view(np.float32), kp.value, np_.value


def unpack_conv_split(packed, kh, kw, cin, cout, parts=3):
    """Inverse of pack_conv_split (tests): the sum of the parts (three reproduce the weights exactly) and the parts
    themselves, [Kp/8][parts][Np][8] float32."""
    k = kh * kw * cin
    kp = (k + 31) // 32 * 32
    np_ = (cout + 31) // 32 * 32
    u = packed.view(np.uint16).reshape(kp // 8, parts, np_, 8).astype(np.uint32) << 16
    pt = u.view(np.float32)                                     # [kg, part, n, 8]
    tot = pt.astype(np.float64).sum(axis=1).transpose(0, 2, 1).reshape(kp, np_)
    return tot[:k, :cout].reshape(kh, kw, cin, cout), pt
