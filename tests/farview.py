"""Views whose last pixel lies 2^31 .. 2^33 bytes behind the first.  TEST INFRASTRUCTURE (a plain module, imported like
tests/slabview.py and tests/convview.py; used by tests/test_far_offsets_host.py and tests/test_gpu_far_offsets.py).

Every kernel takes (pointer, pixel pitch) views, so a map of ~2048 pixels at a pitch of 2^18 .. 2^25 floats puts its last pixel
at the byte offsets of a batch of thousands.  `far_slab` / `far_out_slab` build such a view ON THE DEVICE (torch.full for the
fill, a strided copy for the small values; the guard runs of slabview around it), `far_untouched` counts on the device what
a launch wrote outside the view, `far_view` gathers the view; the buffers are never copied whole to the host.

AUDIT: the largest offset each kernel family forms for a launch its host rule accepts, in exact integers, and the type it is
held in.  P = N*H*W input pixels, M = N*OH*OW output pixels, F = H*W pixels of a frame; pitches in floats.

  family (file)                      operand   largest offset                                   held in           rule that bounds it
  ---------------------------------  --------  -----------------------------------------------  ----------------  ------------------------------------
  LDS-DMA GEMM fp32 / split / ext,   x         pointwise: voffset (pixel*ldx + slot)*4, slot <=  unsigned bytes +  P*ldx*4 <= 0xf0000000: the sum stays
  both transposed convs (gemm1x1_              28, soffset (Kp-32)*4: end ((P-1)*ldx + Kp)*4;    int soffset,      below 0xf0000000 + 4*Kp < OOB; reads
  body.h, gemm1x1s_body.h,                     K x K: voffset (pixel*ldx + c0 + slot)*4: end     (int)num_records  behind num_records return zeros
  gemm1x1s_launch.h, convt2x2*.hip)            ((P-1)*ldx + Cin)*4; padding taps: OOB =
                                               0xfffffff0.  num_records = ((P-1)*ldx + Cin)*4
                                               is NEGATIVE as an int from 2^31 on: the hardware
                                               compares it as unsigned
                                     w         Kp*Np*4 (fp32), Kp*Np*6 (split)                   unsigned          Kp*Np*6 <= 0xf0000000 (split rules)
  halo kernel (conv_halo.hip)        x         voffset (pixel*ldx + 12)*4, soffset (Cin-16)*4:   unsigned + int    P*ldx*4 <= 0xf0000000
                                               end ((P-1)*ldx + Cin)*4
  direct epilogue (conv_common.h):   y, res1   ((M-1)*ld + Cout-1)*4 = voffset + soffset         int + int         M*ld*4 < 0x7fffffff (epi_with_direct)
  DMA GEMM, halo kernel              res2      ((M/4-1)*ldr2 + Cout-1)*4                         int + int         (M/4)*ldr2*4 < 0x7fffffff
  staged epilogue, general kernel,   all       pixel * ld + c                                    size_t            conv_check_geometry: P, M (4 M with
  skinny epilogue (conv_common.h,                                                                                  up2) <= 2^31 - 1 keeps every int pixel
  conv_igemm.hip, conv_splitk.hip)                                                                                 index (n*H*W + ih*W + iw, fr*OH + ..) exact
  first-layer kernel (conv_stem.hip) y         ((M-1)*ldy + Cout-1)*4                            int + int         M*ldy*4 < 0x7fffffff, else the route
                                     x         n*H*W*3 + ..                                      size_t            goes on to the tap-major kernels
  skinny kernel (conv_splitk.hip)    x         frame base (size_t) + ((F-1)*ldx + Cin-1)         int elements      F*ldx <= 0x7fffffff; x_resample >= 2
                                               elements; x_resample >= 2: the frame is 4 F                         (pooled on load): 4*F*ldx <= 0x7fffffff
                                               pixels
  depthwise, LDS path (dw_lds.h)     x         frame base (size_t) + window offset in            int bytes         F*ld*4 < 0x7fffffff for x and y, AND
                                               [-PT*W*ldx*4, (bands*rows + KS-2-PT + 1)*W*ldx*4)                   [this change] the window's rows above /
                                               -- rows outside the frame must stay OUT of                          behind the frame inside [-2^31, 2^32)
                                               the descriptor's range, so must not wrap
                                     y         frame base (size_t) + ((F-1)*ldy + C-1)*4         int bytes
  depthwise register kernels, pool,  all       ((n*H + h)*W + w)*ld + c: `n*H + h` is an int     int, then size_t  [this change] every tensor of a launch
  upsample2x_add, zeropad                      product, the rest 64-bit                                            holds <= 2^31 - 1 pixels (DH_EINVAL)
  (spatial.hip)
  eltwise, copy_channels             all       px*ld + c                                         long long         --
  decoder.hip (softargmax2d[_context], all     (f*HW + px)*ld + c                                size_t            --
  depth_means, depth_from_maps,
  kronecker, global_maxmin_softmax)

What the audit found (both fixed in the same change; neither moves a launch of the existing tests):
  * dw_lds.h on a ONE-row map (or with a caller's PT > H): the rows of the window behind the frame are (H + KS-2-PT + 1) rows
    from its base; with F*ldx*4 just below 2^31 that is up to 3 * 2^31 bytes for a 5 x 5 filter on H = 1, the offset wraps
    past 2^32 and lands INSIDE the frame, so a padding tap reads data.  From H = 2 on (and 'same' padding) the old rule
    already implied the bound.  The host rule now states it (dw_lds_geometry: `halo32`).
  * spatial.hip: `n * p.H + h` wraps from N*H = 2^31 rows on (8 GiB of one-channel pixels at least).  The launchers now
    refuse more than 2^31 - 1 pixels per tensor with DH_EINVAL, as dh_conv2d_f32 always has.
"""
import ctypes as C

import numpy as np

import convview as CV
import slabview as SV

GIB = 1 << 30
OOB = 0xfffffff0
MAX_BUFFER_BYTES = 0xf0000000
INT31 = 0x7fffffff
DH_EINVAL = -1


def need(nbytes):
    """Skip (the only skip of the far-offset tests) when the device cannot spare `nbytes` and 2 GiB beside them."""
    import pytest
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + 2 * GIB:
        pytest.skip('%.1f GiB of device memory free, the test needs %.1f + 2' % (free / GIB, nbytes / GIB))


def release():
    """What every far-offset test calls at its end (its tensors are locals that died with the frame that held them)."""
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def slab_bytes(shape, ld):
    return 4 * (int(np.prod(shape[:-1])) * ld + 2 * SV.GUARD)


def far_slab(values, ld, off, fill, device='cuda'):
    """slabview.slab built on the device: `values` [..., C] in channels [off, off + C) of [..., ld] pixels holding `fill`,
    between two guard runs.  Returns (tensor, device pointer of the view)."""
    import torch
    v = torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(device)
    lead, ch = tuple(v.shape[:-1]), v.shape[-1]
    assert 0 <= off and off + ch <= ld, (ch, ld, off)
    n = int(np.prod(lead)) * ld
    base = torch.full((n + 2 * SV.GUARD,), fill, dtype=torch.float32, device=device)
    t = base[SV.GUARD:SV.GUARD + n].view(lead + (ld,))
    t[..., off:off + ch] = v
    assert t._base is base and t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off


def far_out_slab(shape, ld, off, canary=SV.CANARY, device='cuda'):
    """An output view of `shape` = [..., C]: the whole slab, the view included, holds the canary."""
    import torch
    lead = tuple(shape[:-1])
    assert 0 <= off and off + shape[-1] <= ld, (shape, ld, off)
    n = int(np.prod(lead)) * ld
    base = torch.full((n + 2 * SV.GUARD,), canary, dtype=torch.float32, device=device)
    t = base[SV.GUARD:SV.GUARD + n].view(lead + (ld,))
    assert t._base is base and t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off


def far_untouched(t, off, C, canary=SV.CANARY):
    """Number of floats outside channels [off, off + C) of a tensor made by far_slab / far_out_slab, guard runs included,
    that no longer hold `canary` bit for bit (0: untouched).  Counted on the device, 2^28 floats at a time."""
    import torch
    want = int(np.array(canary, np.float32).view(np.int32))
    bits = t._base.view(torch.int32)
    bad = 0
    for i in range(0, bits.numel(), 1 << 28):
        bad += int((bits[i:i + (1 << 28)] != want).sum())
    if C:
        bad -= int((t[..., off:off + C].contiguous().view(torch.int32) != want).sum())
    return bad


def far_view(t, off, C):
    """The view's values as a NumPy array [..., C] (gathered on the device)."""
    return t[..., off:off + C].contiguous().cpu().numpy()


# ---- the audit's formulas, for the host test -------------------------------------------------------------------------------
def largest_offsets(a, r):
    """The audit table evaluated for a dh_conv_args `a` that dh_conv2d_route accepted as `r`: a list of
    (what, value, bound, inclusive) -- value <= bound (inclusive) or value < bound must hold for each."""
    P, M = a.N * a.H * a.W, a.N * a.OH * a.OW
    F = a.H * a.W
    out = []
    if r.kernel in (CV_KERNEL['dma'], CV_KERNEL['split'], CV_KERNEL['split_ext'], CV_KERNEL['halo']):
        span = a.Kp if (a.KH == 1 and a.KW == 1) else a.Cin      # pointwise: the K tail is read behind the pixel's channels
        out.append(('x descriptor bytes', ((P - 1) * a.ldx + a.Cin) * 4, MAX_BUFFER_BYTES, True))
        out.append(('x voffset + soffset + 16', ((P - 1) * a.ldx + span) * 4, OOB, False))
    if r.kernel in (CV_KERNEL['dma'], CV_KERNEL['halo']) and r.epi & 2:
        out.append(('y direct', ((M - 1) * a.ldy + a.Cout) * 4, 1 << 31, False))
        if a.res1:
            out.append(('res1 direct', ((M - 1) * a.ldr1 + a.Cout) * 4, 1 << 31, False))
        if a.res2:
            out.append(('res2 direct', ((M // 4 - 1) * a.ldr2 + a.Cout) * 4, 1 << 31, False))
    if r.kernel == CV_KERNEL['stem']:
        out.append(('y first layer', ((M - 1) * a.ldy + a.Cout) * 4, 1 << 31, False))
    if r.kernel == CV_KERNEL['skinny']:
        frame = F * (4 if a.x_resample >= 2 else 1) // (4 if a.x_resample == 1 else 1)
        out.append(('x skinny elements', (frame - 1) * a.ldx + a.Cin, 1 << 31, False))
    return out


CV_KERNEL = {'general': 1, 'dma': 2, 'split': 3, 'split_ext': 4, 'halo': 5, 'skinny': 6, 'stem': 7}     # dh_conv_route.kernel
THIRTYTWO_BIT = (2, 3, 4, 5)          # families that read x through a buffer descriptor


# ---- the layers of the far-offset tests: N = 2 on 32 x 32 maps (P = M = 2048) unless the family needs another shape ------
def _far_cases():
    K = CV.Case
    cs = [
        # direct epilogue of the fp32 DMA GEMM, tile_cfg 12 = 128 x 64 (tm == 1): with Cout = 96 the column tiles at n0 = 0 are
        # interior (direct), those at n0 = 64 are not (staged); 13 = 128 x 32 on Cout = 96: every tile direct, res2 at half resolution
        K('direct', (2, 32, 32, 64), 96, pre='relu', bn=True, relu=True, res1=True, cfgs=(12,)),
        K('direct_down', (2, 32, 32, 32), 96, bn=True, res1=True, res2='down', cfgs=(13,)),
        K('halo', (2, 32, 32, 48), 72, k=3, pre='relu', bn=True, relu=True, res1=True, w_split=2, cfgs=(0,), family='halo'),
        # x through a buffer descriptor
        K('pw_ktail', (2, 32, 32, 100), 96, pre='relu', bn=True, res1=True, cfgs=(12,)),
        K('pw_bn', (2, 32, 32, 96), 96, pre='bnrelu', bn=True, res1=True, cfgs=(12,)),
        K('kxk', (2, 32, 32, 64), 72, k=3, pre='relu', bn=True, res1=True, cfgs=(12,)),
        K('ext_pw', (2, 32, 32, 96), 96, pre='bnrelu', bn=True, res1=True, w_split=5, cfgs=(3,), family='split'),
        K('ext_kxk', (2, 32, 32, 48), 72, k=3, pre='relu', bn=True, res1=True, w_split=5, cfgs=(3,), family='split'),
        # 64-bit: the general kernel and the staged epilogue
        K('general_1x1', (2, 32, 32, 32), 40, pre='relu', bn=True, res1=True, cfgs=(3,)),
        K('general_3x3', (2, 32, 32, 32), 40, k=3, pre='relu', bn=True, res1=True, cfgs=(3,)),
        # first-layer kernel: OH = 2, OW = 128, M = 512
        K('stem', (2, 4, 256, 3), 32, k=3, stride=2, bn=True, relu=True, family='stem'),
        K('stem_u8', (2, 4, 256, 3), 32, k=3, stride=2, bn=True, relu=True, family='stem', x_u8=True),
        # skinny kernel: a rule on the frame (N = 1)
        K('skinny', (1, 8, 8, 64), 24, k=3, pre='relu', bn=True, res1=True, family='skinny'),
        K('skinny_rs2', (1, 8, 8, 64), 24, k=3, pre='bnrelu', bn=True, res1=True, family='skinny', x_resample=2),
    ]
    for ws in (1, 3, 4):
        cs.append(K('split%d' % ws, (2, 32, 32, 96), 96, pre='relu', bn=True, res1=True, w_split=ws, cfgs=(3,), family='split'))
    return {c.name: c for c in cs}


CASES = _far_cases()


def with_batch(case, n, w_split=None):
    """The same layer at another batch size (and split code)."""
    c = CV.Case(case.name, (n, case.H, case.W, case.Cin), case.Cout, k=case.k, stride=case.stride, pre=case.pre, bn=case.bn,
                relu=case.relu, res1=case.res1, res2=case.res2, up2=case.up2, pool=case.pool,
                w_split=case.w_split if w_split is None else w_split, cfgs=case.cfgs, family=case.family,
                x_resample=case.x_resample, x_u8=case.x_u8)
    return c


def steps_around(limit, per_float, inclusive):
    """The four pitches (multiples of 4 floats) around a byte / element limit on pixels * ld * per_float: one step below the
    last pitch the condition holds for, that pitch, and one and two steps above.  -> [(ld, holds)]"""
    holds = (lambda ld: ld * per_float <= limit) if inclusive else (lambda ld: ld * per_float < limit)
    ld0 = limit // per_float // 4 * 4
    while not holds(ld0):
        ld0 -= 4
    assert holds(ld0) and not holds(ld0 + 4)
    return [(ld, holds(ld)) for ld in (ld0 - 4, ld0, ld0 + 4, ld0 + 8)]


# ---- convolution launches with far operands -----------------------------------------------------------------------------
def pack(case, w_hwio, device='cuda'):
    """convview.pack, and the packings of the extended scope (w_split 5 / 6 / 7: the bytes of 1 / 3 / 4)."""
    import torch
    from deephar_amd.engine import packing
    if case.w_split < 5:
        return CV.pack(case, w_hwio, device)
    pk, kp, np_ = packing.pack_conv_split(w_hwio, parts=packing.WIDE_SPLIT_PARTS[case.w_split])
    return torch.from_numpy(pk).to(device), kp, np_


def conv_launch(lib, case, data, w, cfg, far=None, lay='aligned', what=''):
    """One dh_conv2d_f32 launch of `case`: operands in `far` = {operand: pitch} on device-built far views, the others on
    slabview views of layout `lay` (a name, or {operand: name}); offsets are those of the layout in both.  Canaries of y
    are checked (everything, the view included, after a refusal).  Returns (rc, route, args, y values or None)."""
    import torch
    far = far or {}
    t, ptr, ld, off, keep = {}, {}, {}, {}, []
    for o in case.operands():
        name = lay[o] if isinstance(lay, dict) else lay
        ld[o], off[o] = CV.layout_of(case, o, name)
        if o in far:
            assert far[o] >= off[o] + case.shape_of(o)[-1]
            ld[o] = far[o]
        out = o in ('y', 'y_pool')
        if o == 'x' and case.x_u8:
            continue
        if o in far:
            t[o], ptr[o] = far_out_slab(case.shape_of(o), ld[o], off[o]) if out else \
                far_slab(data[o], ld[o], off[o], case.fill if o == 'x' else np.nan)
        else:
            t[o], ptr[o] = SV.out_slab(case.shape_of(o), ld[o], off[o]) if out else \
                SV.slab(data[o], ld[o], off[o], case.fill if o == 'x' else np.nan)
    tab = {}
    for n in (['pre_scale', 'pre_shift'] if case.pre_bn else []) + (['post_scale', 'post_shift'] if case.bn else []):
        tt, tab[n] = CV.table(data[n], False)
        keep.append(tt)
    lut = None
    if case.x_u8:                                       # dense bytes, as convview.launch lays them out
        b = np.zeros(data['x_u8'].size + 32, np.uint8)
        b[16:16 + data['x_u8'].size] = data['x_u8'].ravel()
        xb = torch.from_numpy(b).cuda()
        lutd = torch.from_numpy(np.ascontiguousarray(data['lut'], np.float32)).cuda()
        keep += [xb, lutd]
        ptr['x'], ld['x'], lut = xb.data_ptr() + 16, case.Cin, lutd.data_ptr()
    wt, kp, np_ = w
    assert (kp, np_) == (case.Kp, case.Np), (case, kp, np_)
    a = CV.fill_args(case, ptr, ld, wt.data_ptr(), tab, in_lut=lut)
    r = CV.route(lib, a, cfg)
    rc = lib.dh_conv2d_f32(C.byref(a), cfg, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert r.rc == rc, (case, what, cfg, rc, r.rc)                      # the library said so before it launched
    y = None
    if 'y' in far:
        n_bad = far_untouched(t['y'], off['y'] if rc == 0 else 0, case.Cout if rc == 0 else 0)
        assert n_bad == 0, '%s: %d floats written outside the view of y' % (what, n_bad)
        if rc == 0:
            y = far_view(t['y'], off['y'], case.Cout)
    else:
        SV.assert_untouched(t['y'], off['y'] if rc == 0 else 0, case.Cout if rc == 0 else 0, what=what)
        if rc == 0:
            y = SV.view(t['y'], off['y'], case.Cout)
    return rc, r, a, y
