"""Convolution launches on channel-slab views.  TEST INFRASTRUCTURE (a plain module, imported like tests/slabview.py).

tests/test_gpu_conv_views.py (GPU) and tests/test_conv_views_host.py (CPU) share what is here:

  * the case tables: every dh_conv2d_f32 case as a `Case` (geometry, operands, weight packing, the tilings to force);
  * `fill_args`: a dh_conv_args from a case, one (pointer, pitch) per operand and the table pointers -- real device pointers on
    the GPU, fake ones of the intended alignment in the host test;
  * `route` / `paths`: what the library says a launch will be (dh_conv2d_route: family, tiling, A gather, epilogue bits, pool
    form) and, per output tile, the epilogue path it takes -- `direct_tile`'s interior condition is kernel-side geometry and is
    the one thing restated here;
  * `refusal`: the launches that must answer DH_EUNSUPPORTED, and nothing else may;
  * `launch`: build the views (slabview.slab / out_slab), fill the struct, launch, synchronise, check the canaries of every
    output slab, return the views' values.

Input fill.  NaN wherever the kernel masks what lies outside its view; LOUD = 2**100 (finite, exact in fp32 and bf16) for the
LDS-DMA family when Cin % 32 != 0: there the padded k slots of a pixel are DMA'd from the floats that follow it in memory --
on a view, the neighbouring channels of the slab -- and meet zero weights (include/deephar_hip.h, "Inputs must be FINITE"):
0 * LOUD is an exact zero, a leak through a non-zero weight is about 1e29.
"""
import ctypes as C

import numpy as np

import slabview as SV

LOUD = 2.0 ** 100
DH_EUNSUPPORTED = -2
OPERANDS = ('x', 'y', 'res1', 'res2', 'y_pool')        # operand number k of slabview.layout: no two share a pitch or offset
NUM_GENERAL = 9                                        # tile_cfg 0..8: implicit-GEMM kernel; 9..17: the same tiles on the LDS-DMA GEMM
# dh_conv_route.kernel -> Case.family_of (the extended scope's kernels are a split family too)
FAMILY_OF_KERNEL = {1: 'general', 2: 'dma', 3: 'split', 4: 'split', 5: 'halo', 6: 'skinny', 7: 'stem'}


def same_pad(size, k, s):
    """TF 'SAME': (pad in front, output extent)."""
    out = -(-size // s)
    return max((out - 1) * s + k - size, 0) // 2, out


class Case:
    """One convolution layer and the launches a test makes of it.
    pre: 'none' | 'relu' | 'bn' | 'bnrelu'; res2: None | 'full' | 'down' (half resolution) | 'up' (with up2: at the up-sampled
    resolution); family: 'fp32' (tile_cfg picks general / DMA), 'halo', 'split', 'skinny', 'stem'."""

    def __init__(self, name, shape, cout, k=1, stride=1, pre='none', bn=False, relu=False, res1=False, res2=None, up2=False,
                 pool=False, w_split=0, cfgs=(-1,), family='fp32', x_resample=0, x_u8=False):
        self.name, (self.N, self.H, self.W, self.Cin), self.Cout = name, shape, cout
        self.k, self.stride, self.pre, self.bn, self.relu, self.res1, self.res2 = k, stride, pre, bn, relu, res1, res2
        self.up2, self.pool, self.w_split, self.cfgs, self.family = up2, pool, w_split, tuple(cfgs), family
        self.x_resample, self.x_u8 = x_resample, x_u8
        self.PT, self.OH = same_pad(self.H, k, stride)
        self.PL, self.OW = same_pad(self.W, k, stride)
        self.K = k * k * self.Cin
        self.Kp, self.Np = (self.K + 31) // 32 * 32, (cout + 31) // 32 * 32      # dh_conv2d_packed_dims
        self.M = self.N * self.OH * self.OW

    # families that refuse an x that is not 16-byte aligned instead of falling back
    fixed_x = property(lambda s: s.family in ('halo', 'split', 'stem'))
    pre_bn = property(lambda s: s.pre in ('bn', 'bnrelu'))
    pre_relu = property(lambda s: s.pre in ('relu', 'bnrelu'))

    @property
    def fill(self):
        dma = self.family == 'split' or (self.family == 'fp32' and any(c < 0 or c >= NUM_GENERAL for c in self.cfgs))
        return LOUD if dma and self.Cin % 32 != 0 else np.nan

    def operands(self):
        return [o for o in OPERANDS if o in ('x', 'y') or (o == 'res1' and self.res1) or (o == 'res2' and self.res2) or
                (o == 'y_pool' and self.pool)]

    def shape_of(self, op):
        n, oh, ow, co = self.N, self.OH, self.OW, self.Cout
        if op == 'x':
            h, w = {0: (self.H, self.W), 1: (self.H // 2, self.W // 2), 2: (2 * self.H, 2 * self.W),
                    3: (2 * self.H, 2 * self.W)}[self.x_resample]
            return (n, h, w, self.Cin)
        if op == 'y':
            return (n, 2 * oh, 2 * ow, co) if self.up2 else (n, oh, ow, co)
        if op == 'res1':
            return (n, oh, ow, co)
        if op == 'res2':
            return {'full': (n, oh, ow, co), 'down': (n, oh // 2, ow // 2, co), 'up': (n, 2 * oh, 2 * ow, co)}[self.res2]
        return (n, oh // 2, ow // 2, co)

    def family_of(self, cfg):
        if self.family != 'fp32':
            return self.family
        return 'auto' if cfg < 0 else ('general' if cfg < NUM_GENERAL else 'dma')

    def __repr__(self):
        return self.name


def layout_of(case, op, name):
    """(ld, off) of operand `op` in layout `name`."""
    return SV.layout(case.shape_of(op)[-1], name, OPERANDS.index(op))


def layout_sets(case):
    """name -> ({operand: layout name}, tables unaligned): dense, aligned, odd, one set per operand with that operand alone
    odd (the rest aligned), and the unaligned tables as a further single-operand set.  A family that refuses a misaligned x
    keeps x aligned in `odd`; its `odd_x` set is the refusal."""
    ops = case.operands()

    def mk(default, **over):
        d = {o: default for o in ops}
        d.update(over)
        return d
    sets = {'dense': (mk('dense'), False), 'aligned': (mk('aligned'), False),
            'odd': (mk('odd', x='aligned') if case.fixed_x else mk('odd'), False)}
    for o in ops:
        if not (o == 'x' and case.family == 'stem'):           # (the first-layer rule needs ldx == 3: x stays dense there)
            sets['odd_' + o] = (mk('aligned', **{o: 'odd'}), False)
    if case.pre_bn or case.bn:
        sets['tables'] = (mk('aligned'), True)
    if case.family == 'stem':
        sets = {n: (dict(l, x='dense'), t) for n, (l, t) in sets.items()}
    return sets


def refusal(case, lay, tables_unaligned, cfg):
    """Why dh_conv2d_f32 must answer DH_EUNSUPPORTED for this launch (None: it must run).  These are all the refusals an
    alignment may cause; every other -2 is a failure of the test."""
    x_odd = lay['x'] == 'odd'
    if x_odd and case.w_split in (1, 3, 4):
        return 'split-bf16 needs a 16-byte aligned x'
    if x_odd and case.w_split == 2:
        return 'the halo kernel needs a 16-byte aligned x'
    if case.family in ('skinny', 'stem'):
        return None                                            # rules "never on alignment"
    if x_odd and case.up2:
        return 'the up-sampling epilogue needs the float4 gather'
    if x_odd and cfg >= NUM_GENERAL:
        return 'the LDS-DMA GEMM needs a 16-byte aligned x'
    if case.pool and (any(lay.get(o) == 'odd' for o in ('y', 'y_pool', 'res1', 'res2')) or (tables_unaligned and case.bn)):
        return 'the pooled second output needs the 16-byte epilogue'
    return None


def refused_by_shape(case, cfg):
    """The launches of the tables the library refuses on EVERY layout, as test_gpu_conv_views.test_conv2d_on_views states them:
    the 13 x 11 split cases (a skinny layer by the shape rule) and the wide tilings 14 and 15 below three parts."""
    return case.family == 'split' and ('13x11' in case.name or (cfg in (14, 15) and case.w_split != 1))


def fill_args(case, ptr, ld, w=16, tables=None, in_lut=None):
    """dh_conv_args of `case`: ptr / ld map an operand to its view's pointer / pixel pitch, tables maps 'pre_scale' .. to
    pointers.  No pointer is dereferenced here."""
    from deephar_amd import _lib
    t = tables or {}
    a = _lib.ConvArgs()
    a.x, a.w, a.y = ptr['x'], w, ptr['y']
    a.pre_scale, a.pre_shift = t.get('pre_scale'), t.get('pre_shift')
    a.post_scale, a.post_shift = t.get('post_scale'), t.get('post_shift')
    a.res1, a.res2, a.y_pool, a.in_lut = ptr.get('res1'), ptr.get('res2'), ptr.get('y_pool'), in_lut
    a.N, a.H, a.W, a.Cin, a.ldx = case.N, case.H, case.W, case.Cin, ld['x']
    a.OH, a.OW, a.Cout, a.ldy = case.OH, case.OW, case.Cout, ld['y']
    a.KH = a.KW = case.k
    a.SH = a.SW = case.stride
    a.PT, a.PL, a.K, a.Kp, a.Np = case.PT, case.PL, case.K, case.Kp, case.Np
    a.ldr1, a.ldr2, a.ldyp = ld.get('res1', 0), ld.get('res2', 0), ld.get('y_pool', 0)
    a.pre_relu, a.post_relu, a.up2 = int(case.pre_relu), int(case.relu), int(case.up2)
    a.x_u8, a.w_split, a.res2_down, a.x_resample = int(case.x_u8), case.w_split, int(case.res2 == 'down'), case.x_resample
    return a


def fake_args(case, lay, tables_unaligned):
    """fill_args with fake pointers of the alignment the layouts give (the host test): 1 MB apart, 16-byte aligned bases."""
    ptr, ld = {}, {}
    for i, o in enumerate(case.operands()):
        ld[o], off = layout_of(case, o, lay[o])
        ptr[o] = 0x100000 * (i + 1) + 4 * off
    tab = {}
    names = (['pre_scale', 'pre_shift'] if case.pre_bn else []) + (['post_scale', 'post_shift'] if case.bn else [])
    for i, n in enumerate(names):
        tab[n] = 0x4000000 + 0x1000 * i + (4 if tables_unaligned else 0)
    return fill_args(case, ptr, ld, 0x8000000, tab, in_lut=0x9000000 if case.x_u8 else None)


# ---- what the library says a launch will be ------------------------------------------------------------------------------------
def route(lib, a, cfg):
    """dh_conv2d_route(a, cfg) as a ctypes struct: rc, kernel, tile_cfg, parts, bm, bn, tm, vec4, epi, pool, tiles."""
    from deephar_amd import _lib
    return _lib.conv_route(lib, a, cfg)


def direct_tile(m0, n0, bm, bn, M, cout):
    """EpiPrefetch::direct_tile: the tile lies fully inside the output."""
    return m0 + bm <= M and n0 + bn <= cout


def paths(lib, case, a, cfg):
    """What a launch that runs (a forced tiling of the general kernel, the DMA GEMM or the halo kernel) goes through:
    'vec4' / 'scalar_a' (general kernel), per output tile 'direct' / 'staged_vec' / 'staged_scalar', the form of a
    half-resolution second residual and of the pooled second output."""
    r = route(lib, a, cfg)
    fam = FAMILY_OF_KERNEL.get(r.kernel)
    assert r.rc == 0 and fam == case.family_of(cfg) and fam in ('general', 'dma', 'halo', 'split') and cfg >= 0, (case, cfg, r.rc, fam)
    out = set()
    if fam == 'general':
        out.add('vec4' if r.vec4 else 'scalar_a')
    e = r.epi & 1
    # the direct path needs the launcher's bit (the fp32 DMA GEMM, and the halo kernel without a second residual; the general
    # kernel and the split GEMM get plain `epi`) and a tiling that prefetches a residual tile (tm == 1)
    d = bool(r.epi & 2) and r.tm == 1
    ohw = a.OH * a.OW
    pow2 = (a.OW & (a.OW - 1)) == 0 and (ohw & (ohw - 1)) == 0
    for m0 in range(0, case.M, r.bm):
        for n0 in range(0, a.Cout, r.bn):
            kind = 'direct' if d and direct_tile(m0, n0, r.bm, r.bn, case.M, a.Cout) else ('staged_vec' if e else 'staged_scalar')
            out.add(kind)
            if a.res2_down:
                out.add('down_direct' if kind == 'direct' else
                        ('down_staged_pow2' if pow2 else 'down_staged_div') if kind == 'staged_vec' else 'down_scalar')
    if r.pool:
        out.add('pool_pair' if r.pool == 1 else 'pool_in_wave')
    return out


# ---- case tables ------------------------------------------------------------------------------------------------------------
def _cases():
    cs = []
    for k in (1, 3):            # (a) implicit-GEMM kernel: M = 874 and Cout = 200 are ragged in every tile
        cs.append(Case('a_general_%dx%d' % (k, k), (2, 19, 23, 96), 200, k=k, pre='relu', bn=True, res1=True, cfgs=(3, 8)))
    # (b) the same pointwise layer on the LDS-DMA GEMM: TM = 2 staged | prefetched residual, direct on the 6 x 3 interior tiles
    # | 32 x 32; -1 is the library's own pick (an odd x sends it to the general kernel: the bits of tile_cfg = 3)
    cs.append(Case('b_dma', (2, 19, 23, 96), 200, pre='relu', bn=True, res1=True, cfgs=(10, 12, 17, 3, -1)))
    cs.append(Case('b_dma_ktail', (2, 19, 23, 100), 200, pre='relu', bn=True, res1=True, cfgs=(10, 12, 17, 3, -1)))
    cs.append(Case('b_dma_bn_prologue', (2, 19, 23, 96), 200, pre='bnrelu', bn=True, res1=True, cfgs=(10, 12, 17, 3, -1)))
    # (c) K x K on the DMA GEMM.  13 x 11 -> 72 looks small enough for it, but with 143 positions, K = 576 and 72 channels the
    # library's shape rule gives it to the skinny-conv kernel whatever tiling is asked for (dh_conv2d_uses_split_k), so it is
    # kept as a skinny case and 35 x 33 (1155 / 306 positions) is what reaches the DMA GEMM's K x K form
    for s in (1, 2):
        cs.append(Case('c_kxk_13x11_s%d' % s, (2, 13, 11, 64), 72, k=3, stride=s, pre='relu', bn=True, res1=True,
                       cfgs=(12, 17, 3), family='skinny'))
        cs.append(Case('c_kxk_dma_s%d' % s, (2, 35, 33, 64), 72, k=3, stride=s, pre='relu', bn=True, res1=True, cfgs=(12, 17, 3)))
    # (d) fused up-sampling: res1 at [2, 8, 8], res2 and y at [2, 16, 16]
    cs.append(Case('d_up2', (2, 8, 8, 32), 96, bn=True, res1=True, res2='up', up2=True, cfgs=(5, 11)))
    # (e) res2 at half resolution: the power-of-two direct form, and the staged form with integer divides.  K = 32 < 64: not a
    # skinny layer (that kernel refuses res2_down)
    cs.append(Case('e_down_pow2', (2, 16, 16, 32), 96, bn=True, res1=True, res2='down', cfgs=(13, 16, 4)))
    cs.append(Case('e_down_div', (2, 12, 20, 32), 96, bn=True, res1=True, res2='down', cfgs=(13, 16, 4)))
    # (f) both residuals at full resolution
    cs.append(Case('f_two_residuals', (1, 30, 30, 64), 100, bn=True, res1=True, res2='full', cfgs=(4, 13)))
    # (g) pooled second output: wave pair (OW = 32) and in-wave (OW = 16, 8)
    cs.append(Case('g_pool_32', (1, 32, 32, 32), 40, bn=True, relu=True, res1=True, pool=True, cfgs=(3, 12)))
    cs.append(Case('g_pool_16', (2, 16, 16, 32), 40, bn=True, relu=True, res1=True, pool=True, cfgs=(3, 12, 8, 17)))
    cs.append(Case('g_pool_8', (4, 8, 8, 32), 40, bn=True, relu=True, res1=True, pool=True, cfgs=(8, 17)))
    # (h) halo kernel (chunk-major packing); Cout = 70: the scalar epilogue
    for co in (72, 70):
        cs.append(Case('h_halo_%d' % co, (1, 32, 32, 48), co, k=3, pre='relu', bn=True, relu=True, res1=True, w_split=2,
                       cfgs=(0, 1, 2), family='halo'))
    # (i) split-bf16 GEMM: every tiling, three modes.  The 13 x 11 shape is a skinny layer by the shape rule, which
    # the split modes refuse on every layout (dh_conv2d_split_eligible == 0); 35 x 33 is the K x K form that runs
    for ws in (1, 3, 4):
        for nm, shape, co, k in (('pw', (2, 19, 23, 96), 200, 1), ('pw_ktail', (2, 19, 23, 100), 200, 1),
                                 ('kxk_13x11', (2, 13, 11, 64), 72, 3), ('kxk', (2, 35, 33, 64), 72, 3)):
            cs.append(Case('i_split%d_%s' % (ws, nm), shape, co, k=k, pre='relu', bn=True, res1=True, w_split=ws,
                           cfgs=tuple(range(-1, 16)), family='split'))
    # (j) skinny kernel: 3x3, a 1x1 with Cin % 4 != 0 (dword loads on every layout), up2 once, resampling on load
    cs.append(Case('j_skinny_3x3', (2, 8, 8, 64), 24, k=3, pre='relu', bn=True, res1=True, res2='full', family='skinny'))
    cs.append(Case('j_skinny_1x1_cin70', (2, 8, 16, 70), 40, pre='bnrelu', bn=True, res1=True, res2='full', family='skinny'))
    cs.append(Case('j_skinny_up2', (2, 8, 8, 64), 24, k=3, pre='relu', bn=True, res1=True, res2='up', up2=True, family='skinny'))
    for rs in (1, 2, 3):
        cs.append(Case('j_skinny_resample%d' % rs, (2, 8, 8, 64), 24, k=3, pre='bnrelu', bn=True, res1=True, family='skinny',
                       x_resample=rs))
    # (k) first-layer kernel: [1, 16, 256, 3] -> 32, 3x3 stride 2 (OW = 128, OH = 8), float frames and uint8 frames
    cs.append(Case('k_stem', (1, 16, 256, 3), 32, k=3, stride=2, bn=True, relu=True, family='stem'))
    cs.append(Case('k_stem_u8', (1, 16, 256, 3), 32, k=3, stride=2, bn=True, relu=True, family='stem', x_u8=True))
    return cs


CASES = {c.name: c for c in _cases()}

# (l) transposed 2x2 / stride-2 convolution: (N, H, W, Cin) -> Cout; 18 channels per block: the scalar depth-to-space store
CONVT_SHAPE = (2, 6, 5, 24)
CONVT_COUTS = (20, 18)


# ---- device side ------------------------------------------------------------------------------------------------------------
def table(values, unaligned, device='cuda'):
    """A per-channel table on the device at a base 4 bytes past a 16-byte boundary (unaligned) or on one; NaN around it.
    Returns (tensor to keep alive, pointer)."""
    import torch
    v = np.asarray(values, np.float32)
    lead = 5 if unaligned else 4
    buf = np.full(v.size + 12, np.nan, np.float32)
    buf[lead:lead + v.size] = v
    t = torch.from_numpy(buf).to(device)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * lead


def pack(case, w_hwio, device='cuda'):
    """The weight of `case` in the packing its w_split asks for -> (device tensor, Kp, Np)."""
    import torch
    from deephar_amd import functional as F
    from deephar_amd.engine import packing
    if case.w_split == 0:
        return F.pack_conv_weight(w_hwio, device)
    pk, kp, np_ = packing.pack_conv_halo(w_hwio) if case.w_split == 2 else \
        packing.pack_conv_split(w_hwio, parts=packing.SPLIT_PARTS[case.w_split])
    return torch.from_numpy(pk).to(device), kp, np_


class Views:
    """The operand views of one launch: inputs in slabs holding `fill`, outputs in slabs of canaries."""

    def __init__(self, case, data, lay, fill=None):
        self.case, self.t, self.ptr, self.ld, self.off = case, {}, {}, {}, {}
        fill = case.fill if fill is None else fill
        for o in case.operands():
            ld, off = layout_of(case, o, lay[o])
            if o in ('y', 'y_pool'):
                self.t[o], self.ptr[o] = SV.out_slab(case.shape_of(o), ld, off)
            elif o == 'x' and case.x_u8:
                continue
            else:
                self.t[o], self.ptr[o] = SV.slab(data[o], ld, off, fill if o == 'x' else np.nan)
            self.ld[o], self.off[o] = ld, off

    def outputs(self, what=''):
        """Canaries of every output slab checked; the views' values."""
        out = {}
        for o in ('y', 'y_pool'):
            if o in self.t:
                SV.assert_untouched(self.t[o], self.off[o], self.case.Cout, what='%s %s' % (what, o))
                out[o] = SV.view(self.t[o], self.off[o], self.case.Cout)
        return out

    def assert_nothing_written(self, what=''):
        """A refused launch: every output slab still holds its canary everywhere, inside the view too."""
        for o in ('y', 'y_pool'):
            if o in self.t:
                SV.assert_untouched(self.t[o], 0, 0, what='%s (refused) %s' % (what, o))


def launch(lib, case, data, lay, w, cfg=-1, tables_unaligned=False, x_lead=0, what=''):
    """One dh_conv2d_f32 launch of `case` on views: data maps operand / table names to NumPy arrays, lay an operand to its
    layout name, w = pack(case, ...).  x_lead (dense uint8 / float frames only): floats (bytes for uint8) between a 16-byte
    boundary and the frames' base.  Returns (rc, {'y': values, 'y_pool': values}); after rc != 0 nothing was written."""
    import torch
    v = Views(case, data, lay)
    keep, tab = [], {}
    for n in (['pre_scale', 'pre_shift'] if case.pre_bn else []) + (['post_scale', 'post_shift'] if case.bn else []):
        t, tab[n] = table(data[n], tables_unaligned)
        keep.append(t)
    lut = None
    if case.x_u8:                                       # dense bytes (ldx = Cin), base x_lead bytes past a 16-byte boundary
        b = np.zeros(data['x_u8'].size + 32, np.uint8)
        b[16 + x_lead:16 + x_lead + data['x_u8'].size] = data['x_u8'].ravel()
        xb = torch.from_numpy(b).cuda()
        lutd = torch.from_numpy(np.ascontiguousarray(data['lut'], np.float32)).cuda()
        keep += [xb, lutd]
        v.ptr['x'], v.ld['x'], lut = xb.data_ptr() + 16 + x_lead, case.Cin, lutd.data_ptr()
    elif x_lead:
        assert lay['x'] == 'dense'
        t, p = SV.slab(np.asarray(data['x'], np.float32).reshape(1, -1), data['x'].size + x_lead + 3, x_lead, case.fill)
        keep.append(t)
        v.ptr['x'] = p
    wt, kp, np_ = w
    assert (kp, np_) == (case.Kp, case.Np), (case, kp, np_)
    a = fill_args(case, v.ptr, v.ld, wt.data_ptr(), tab, in_lut=lut)
    rc = lib.dh_conv2d_f32(C.byref(a), cfg, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert route(lib, a, cfg).rc == rc, (case, what, cfg, rc)          # the library said so before it launched
    if rc != 0:
        v.assert_nothing_written(what)
        return rc, None
    return rc, v.outputs(what)
