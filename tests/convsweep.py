"""A seeded sweep of convolution, depthwise and pooling geometry.  TEST INFRASTRUCTURE (a plain module, imported like
tests/convview.py, whose launch plumbing it reuses).

dh_conv2d_f32 takes KH, KW, SH, SW, PT, PL, OH, OW as independent fields and engine/binding.py fills them one by one from
layer attributes; the hand-picked tables of tests/convview.py know only square kernels, one stride and TF-SAME padding.  Here:

  * `cases(lib)`: a deterministic draw with one stratum per kernel family (general, LDS-DMA, skinny, halo, split-bf16
    standard, split-bf16 extended class (a) and (b)).  A `Sweep` is a convview.Case with the free geometry: rectangular
    kernels, SH != SW, padding TF-SAME / 'valid' / explicit (pt, pb), (pl, pr) with 0 <= pad < kernel extent, so that every
    window starts inside the padded frame and none lies wholly in padding -- the set a Keras layer stack can produce.  A
    candidate is kept when dh_conv2d_route (on fake pointers of the layout's alignment) puts it in the stratum's family;
  * `data`: Gaussian operands with a spread of magnitudes -- every input channel of x times 2^U(-3, 3), every output channel
    of w, post_shift, res1 and res2 times (one) 2^U(-6, 6) -- so that an error confined to a small output channel is seen;
  * `statement`: the layer written from the definition (explicit zero padding, a strided correlation, a crop), at a dtype:
    fp64 is the truth, fp32 the CPU result, and on absolute values it gives the magnitude sum
        B = |post_scale| (|pro(x)| conv |w|) + |post_shift| + |res1| + |res2|;
    `swap` evaluates it the way a kernel would get the geometry wrong (tests/test_conv_sweep_host.py: discrimination);
  * `bound`: the bar per element, |y - fp64| <= ((K + 8) 2^-24 + SPLIT_TERM[mode]) B: the forward error of a length-K fp32
    sum in any order ((K - 1) u for the additions, u for the product's rounding where it is not fused), plus the roundings
    of the prologue's fused multiply-add, of post_scale / post_shift and of the two residual additions; ReLU is 1-Lipschitz.
    A split mode adds what its dropped products can amount to per unit of |x| |w|.  bf16 keeps 8 significant bits, so a
    round to nearest leaves |x - x_1| <= u |x| with u = 2^-8, and |x - x_1 - x_2| <= u^2 |x| (x = x_1 + x_2 + x_3 exactly):
        bf16    drops x (w - w_1) + (x - x_1) w_1                     <= 2 u             = 2^-7
        bf16x2  drops x_2 w_2 + x_3 w + (x_1 + x_2) w_3               <= 3 u^2 (1 + ..)  < 2^-14
        bf16x3  drops x_2 w_3 + x_3 w_2 + x_3 w_3                     <= 2 u^3 (1 + ..)  < 2^-22
    (Constants of 2^-8, 2^-16 and 2^-25 follow if one takes |x - x_1| <= 2^-9 |x|; that is half of what a bf16 rounding can
    leave, and the fp64 emulation of the one-part mode exceeds 2^-8 B on the CPU, by 9 % on split_02.)
    Derived, not fitted: the host test checks the CPU fp32 statement and the fp64 emulations E_P (bf16_modes_ref.conv_ep)
    against it;
  * `launch` / `launches`: every launch a test makes of a case -- tile_cfg = -1, one forced general tiling, one forced
    LDS-DMA tiling with TM == 1, the split / halo packings of the case's stratum -- on the views of the case's layout set.

The same window generator and statement builder serve dh_pool2d_f32, dh_dwconv2d_f32 and dh_dwconv2d_strided_f32
(`pool_cases`, `dw_cases`, `dws_cases`).
"""
import ctypes as C
import functools
import zlib

import numpy as np

import convview as CV
import slabview as SV

U24 = 2.0 ** -24
SPLIT_TERM = {3: 2.0 ** -22, 2: 2.0 ** -14, 1: 2.0 ** -7}      # bf16 parts per operand -> truncation per unit of |x| |w|
PARTS_OF = {1: 3, 3: 2, 4: 1, 5: 3, 6: 2, 7: 1}                 # dh_conv_args.w_split -> parts
STRATA = (('general', 48), ('dma', 48), ('skinny', 48), ('halo', 20), ('split', 32), ('ext_a', 16), ('ext_b', 16))
CELLS = ('KH != KW', 'SH != SW', 'non-SAME', 'BN prologue, KH*KW > 1', 'res2 full', 'res2 down', 'odd layout')
# the cells a family's rule admits: a BN prologue belongs to the register-gather and skinny kernels and to the pointwise DMA
# form; the skinny kernel refuses res2_down; the halo kernel is stride 1; class (a) is pointwise by definition
ADMITS = {'general': CELLS, 'skinny': tuple(c for c in CELLS if c != 'res2 down'),
          'dma': tuple(c for c in CELLS if not c.startswith('BN')),
          'halo': tuple(c for c in CELLS if not c.startswith('BN') and c != 'SH != SW'),
          'split': tuple(c for c in CELLS if not c.startswith('BN')),
          'ext_a': ('res2 full', 'res2 down', 'odd layout'),
          'ext_b': tuple(c for c in CELLS if not c.startswith('BN'))}
SKINNY_DOWN = 'the skinny kernel has no half-resolution second residual'
DEFAULT_REFUSALS = (SKINNY_DOWN,)        # every reason a default launch (tile_cfg = -1, w_split = 0) of the sweep may be refused for


# ---- windows ---------------------------------------------------------------------------------------------------------------
def window(rng, size, k, s, kind):
    """One axis of a window geometry -> (pad in front, pad behind, output extent), or None when `kind` does not exist for it.
    'explicit': 0 <= front, behind < k.  Always (out - 1) * s - front < size: every window starts inside the padded frame
    and holds at least one pixel."""
    if kind == 'same':
        front, out = CV.same_pad(size, k, s)
        return front, max((out - 1) * s + k - size, 0) - front, out
    if kind == 'valid':
        return (0, 0, (size - k) // s + 1) if size >= k else None
    front, behind = int(rng.integers(0, k)), int(rng.integers(0, k))
    if size + front + behind < k:
        return None
    return front, behind, (size + front + behind - k) // s + 1


def is_same(size, k, s, front, out):
    return (front, out) == CV.same_pad(size, k, s)


class Sweep(CV.Case):
    """A convview.Case with free geometry.  `stratum`: the family it was drawn for; `layout`: its layout set; `gcfg` / `dcfg`:
    the forced general / LDS-DMA tiling; `scfg`: the forced tiling of its split or halo launches."""

    def __init__(self, name, stratum, shape, cout, kh, kw, sh, sw, pads, outs, pre, bn, relu, res1, res2, layout, gcfg, dcfg, scfg):
        self.name, self.stratum, (self.N, self.H, self.W, self.Cin), self.Cout = name, stratum, shape, cout
        self.KH, self.KW, self.SH, self.SW = kh, kw, sh, sw
        (self.PT, self.PB), (self.PL, self.PR) = pads
        self.OH, self.OW = outs
        self.k, self.stride = kh, sh                          # (convview.fill_args reads them; set_geometry overwrites the fields)
        self.pre, self.bn, self.relu, self.res1, self.res2 = pre, bn, relu, res1, res2
        self.up2, self.pool, self.w_split, self.x_resample, self.x_u8 = False, False, 0, 0, False
        self.layout, self.gcfg, self.dcfg, self.scfg = layout, gcfg, dcfg, scfg
        self.cfgs = (-1, gcfg, dcfg)
        self.family = 'skinny' if stratum == 'skinny' else 'fp32'
        self.K = kh * kw * self.Cin
        self.Kp, self.Np = (self.K + 31) // 32 * 32, (cout + 31) // 32 * 32
        self.M = self.N * self.OH * self.OW

    # the families whose launches need a 16-byte aligned x keep it aligned in the odd layout set (convview.layout_sets)
    fixed_x = property(lambda s: s.stratum in ('dma', 'halo', 'split', 'ext_a', 'ext_b'))
    nonsame = property(lambda s: not (is_same(s.H, s.KH, s.SH, s.PT, s.OH) and is_same(s.W, s.KW, s.SW, s.PL, s.OW)))

    def geom(self):
        return dict(KH=self.KH, KW=self.KW, SH=self.SH, SW=self.SW, PT=self.PT, PL=self.PL, OH=self.OH, OW=self.OW)

    def cells(self):
        return {'KH != KW': self.KH != self.KW, 'SH != SW': self.SH != self.SW, 'non-SAME': self.nonsame,
                'BN prologue, KH*KW > 1': self.pre_bn and self.KH * self.KW > 1, 'res2 full': self.res2 == 'full',
                'res2 down': self.res2 == 'down', 'odd layout': self.layout == 'odd'}

    def key(self):
        return (self.name, self.stratum, self.N, self.H, self.W, self.Cin, self.Cout, self.KH, self.KW, self.SH, self.SW, self.PT,
                self.PB, self.PL, self.PR, self.OH, self.OW, self.pre, self.bn, self.relu, self.res1, self.res2, self.layout,
                self.gcfg, self.dcfg, self.scfg)

    def lay(self):
        return CV.layout_sets(self)[self.layout][0]

    def launches(self):
        """(w_split, tile_cfg) of every launch a test makes of the case; the fp32 ones first, tile_cfg = -1 first of all."""
        out = [(0, -1), (0, self.gcfg), (0, self.dcfg)]
        if self.stratum == 'halo':
            out += [(2, -1), (2, self.scfg % 3)]
        if self.stratum == 'split':
            out += [(ws, c) for ws in (1, 5, 3, 4, 6, 7) for c in (-1, self.scfg)]
        if self.stratum in ('ext_a', 'ext_b'):
            out += [(ws, c) for ws in (5, 6, 7) for c in (-1, self.scfg)]
        return out


def set_geometry(a, case, ws=0):
    a.KH, a.KW, a.SH, a.SW, a.PT, a.PL, a.OH, a.OW = case.KH, case.KW, case.SH, case.SW, case.PT, case.PL, case.OH, case.OW
    a.w_split = ws
    return a


def fake_args(case, ws=0):
    """dh_conv_args of a launch of the case on fake pointers of the alignment its layout set gives."""
    return set_geometry(CV.fake_args(case, case.lay(), False), case, ws)


def family(lib, case, ws=0, cfg=-1):
    """(return code, family name) the library answers for a launch."""
    r = CV.route(lib, fake_args(case, ws), cfg)
    return r.rc, CV.FAMILY_OF_KERNEL.get(r.kernel) if r.rc == 0 else None


def refusal(lib, case):
    """Why the default launch of a case is refused (None: it runs), in the style of convview.refusal."""
    if case.res2 == 'down' and lib.dh_conv2d_uses_split_k(C.byref(fake_args(case))):
        return SKINNY_DOWN
    return None


def ext_class(lib, case):
    """0: not a layer of the extended scope alone; 1 / 2: class (a) / (b) -- asked of the exported rules and the route."""
    a = fake_args(case, 5)
    if lib.dh_conv2d_split_eligible(C.byref(a)) or not lib.dh_conv2d_split_wide_eligible(C.byref(a)):
        return 0
    return 1 if case.pre_bn else 2


def in_stratum(lib, case):
    s = case.stratum
    rc, fam = family(lib, case)
    if s in ('general', 'dma'):
        return rc == 0 and fam == s
    if s == 'skinny':
        return bool(lib.dh_conv2d_uses_split_k(C.byref(fake_args(case))))
    if rc != 0 or fam == 'skinny':
        return False
    if s == 'halo':
        return family(lib, case, 2) == (0, 'halo')
    if s == 'split':
        return bool(lib.dh_conv2d_split_eligible(C.byref(fake_args(case, 1)))) and family(lib, case, 1) == (0, 'split')
    return ext_class(lib, case) == (1 if s == 'ext_a' else 2) and family(lib, case, 5) == (0, 'split')


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def _pick(rng, seq, p=None):
    return seq[int(rng.choice(len(seq), p=p))]


def _draw(rng, stratum, name, i):
    """One candidate of a stratum (None: the draw fell outside the set of Keras geometries or of the stratum's sizes)."""
    pointwise = stratum == 'ext_a' or (stratum in ('dma', 'split') and rng.random() < 0.3)
    ks = (1, 2, 3, 5)
    if pointwise:
        kh = kw = sh = sw = 1
        kind = 'same'
    else:
        kh, kw = _pick(rng, ks), _pick(rng, (1, 3, 5) if stratum == 'halo' else ks)
        if stratum == 'halo':
            kh = _pick(rng, (1, 2, 3, 5, 7))
        sh, sw = (1, 1) if stratum == 'halo' else (_pick(rng, (1, 2)), _pick(rng, (1, 2)))
        kind = _pick(rng, ('same', 'valid', 'explicit'), (0.3, 0.2, 0.5))
    if stratum == 'skinny':
        n, h, w = int(rng.integers(1, 4)), int(rng.integers(3, 17)), int(rng.integers(3, 17))
        cin, cout = _pick(rng, (6, 8, 12, 16, 20, 24, 32, 35, 48, 64, 70)), int(rng.integers(5, 73))
    elif stratum == 'halo':
        # the kernel's tiles are whole rows of a 32 x 32 or 16 x 64 OUTPUT map: the input extents follow from the padding
        n, (h, w), cin, cout = 1, _pick(rng, ((32, 32), (16, 64))), _pick(rng, (32, 48, 64)), _pick(rng, (24, 32, 40, 70, 72, 96))
    else:
        n, h, w = int(rng.integers(1, 3)), int(rng.integers(10, 41)), int(rng.integers(10, 41))
        cout = int(rng.integers(8, 101))
        if stratum == 'general':
            cin = _pick(rng, (3, 5, 8, 12, 20, 24, 36, 40))
        elif stratum == 'ext_b':
            cin = _pick(rng, (16, 48, 80))
        elif pointwise:
            cin = _pick(rng, (12, 20, 36, 64, 100, 132))
        else:
            cin = _pick(rng, (32, 64, 96))
    if stratum == 'halo':                     # (h, w) is the output map: stride 1, so H = OH + KH - 1 - pt - pb
        win = []
        for out, k in ((h, kh), (w, kw)):
            if kind == 'same':
                win.append(window(rng, out, k, 1, 'same'))
            elif kind == 'valid':
                win.append((0, 0, out))
            else:
                win.append((int(rng.integers(0, k)), int(rng.integers(0, k)), out))
        h, w = (o + k - 1 - f - b for (f, b, o), k in zip(win, (kh, kw)))
        wh, ww = win
    else:
        wh, ww = window(rng, h, kh, sh, kind), window(rng, w, kw, sw, kind)
    if wh is None or ww is None:
        return None
    (pt, pb, oh), (pl, pr, ow) = wh, ww
    assert oh >= 1 and ow >= 1 and (oh - 1) * sh - pt < h and (ow - 1) * sw - pl < w and 0 <= pt < kh and 0 <= pl < kw
    m = n * oh * ow
    if stratum == 'skinny' and oh * ow > 256:
        return None
    if stratum not in ('skinny', 'halo') and not 200 <= m <= 2200:
        return None
    pres = {'dma': ('none', 'relu', 'bn', 'bnrelu') if pointwise else ('none', 'relu'), 'halo': ('none', 'relu'),
            'split': ('none', 'relu'), 'ext_a': ('bn', 'bnrelu'), 'ext_b': ('none', 'relu')}.get(stratum, ('none', 'relu', 'bn', 'bnrelu'))
    pre = _pick(rng, pres)
    bn, relu, res1 = bool(rng.random() < 0.7), bool(rng.random() < 0.5), bool(rng.random() < 0.6)
    # the second residual and the layout set go round by the case's number, so that the small strata fill their cells too; a
    # skinny layer with a half-resolution residual is a documented refusal: two of them stay in
    res2 = (None, 'full', 'down')[i % 3]
    if stratum == 'skinny' and res2 == 'down' and i % 24 != 2:
        res2 = None
    if res2 == 'down' and (oh % 2 or ow % 2):
        return None
    layout = SV.LAYOUTS[(i + i // 3) % 3]
    gcfg, dcfg, scfg = int(rng.integers(0, CV.NUM_GENERAL)), CV.NUM_GENERAL + int(rng.integers(2, CV.NUM_GENERAL)), int(rng.integers(0, 14))
    return Sweep(name, stratum, (n, h, w, cin), cout, kh, kw, sh, sw, ((pt, pb), (pl, pr)), (oh, ow), pre, bn, relu, res1, res2,
                 layout, gcfg, dcfg, scfg)


def generate(lib, seed=20251):
    """The table: for every stratum the first candidates of its seeded stream that the library routes to its family."""
    out = []
    for si, (stratum, count) in enumerate(STRATA):
        rng = np.random.default_rng([seed, si])
        got = tries = 0
        while got < count:
            tries += 1
            assert tries < 1000 * count, 'stratum %s: %d of %d cases after %d draws' % (stratum, got, count, tries)
            c = _draw(rng, stratum, '%s_%02d' % (stratum, got), got)
            if c is not None and in_stratum(lib, c):
                out.append(c)
                got += 1
    return out


_TABLE = {}


def cases(lib):
    """name -> Sweep, generated once per process."""
    if not _TABLE:
        _TABLE.update((c.name, c) for c in generate(lib))
    return _TABLE


def chunks(stratum, size=32):
    """(stratum, first, last) index ranges of at most `size` cases: the parametrisation of the GPU test."""
    count = dict(STRATA)[stratum]
    return [(stratum, i, min(i + size, count)) for i in range(0, count, size)]


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _gauss(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def channel_scales(rng, n, span):
    return (2.0 ** rng.uniform(-span, span, n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _data(key):
    case = _TABLE[key[0]]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    cs, os_ = channel_scales(rng, case.Cin, 3), channel_scales(rng, case.Cout, 6)
    d = {'x': _gauss(rng, case.shape_of('x')) * cs,
         'w': _gauss(rng, (case.KH, case.KW, case.Cin, case.Cout), np.sqrt(1.0 / case.K)) * os_}
    if case.pre_bn:
        d['pre_scale'], d['pre_shift'] = rng.uniform(0.5, 1.5, case.Cin).astype(np.float32), _gauss(rng, (case.Cin,), 0.3) * cs
    if case.bn:
        d['post_scale'], d['post_shift'] = rng.uniform(0.5, 1.5, case.Cout).astype(np.float32), _gauss(rng, (case.Cout,), 0.3) * os_
    for o in ('res1', 'res2'):
        if o in case.operands():
            d[o] = _gauss(rng, case.shape_of(o)) * os_
    return d


def data(case):
    """Seeded operands of a case (shared by every launch of it, never modified)."""
    return _data(case.key())


# ---- the statement -------------------------------------------------------------------------------------------------------------
SWAPS = ('kh_kw', 'sh_sw', 'pt_pl', 'pb_is_pt', 'pad_first')


def correlate(a, w, KH, KW, SH, SW, PT, PL, OH, OW, pro=None):
    """The definition: a [N, H, W, Cin] zero-padded by PT rows above and PL columns in front (and by what the OH x OW windows
    need below and behind), out[oh, ow] = sum_{kh, kw, c} a[oh SH + kh, ow SW + kw, c] w[kh, kw, c].  `pro`: applied to the
    padded tensor (a kernel that pads BEFORE its prologue)."""
    import torch.nn.functional as TF
    assert w.shape[0] == KH and w.shape[1] == KW
    h, wd = a.shape[1], a.shape[2]
    below, behind = max((OH - 1) * SH + KH - (h + PT), 0), max((OW - 1) * SW + KW - (wd + PL), 0)
    ap = TF.pad(a.permute(0, 3, 1, 2), (PL, behind, PT, below))
    if pro is not None:
        ap = pro(ap.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
    y = TF.conv2d(ap, w.permute(3, 2, 0, 1).contiguous(), stride=(SH, SW))
    assert y.shape[2] >= OH and y.shape[3] >= OW
    return y[:, :, :OH, :OW].permute(0, 2, 3, 1).contiguous()


def up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def operand(case, d, dtype, exact_fma=False):
    """pro(x): the optional BatchNormalization and ReLU prologue.  exact_fma: the kernels' fused multiply-add, as one rounding
    of the fp64 value to fp32."""
    import torch
    x = torch.from_numpy(d['x'])
    if exact_fma:
        a = x.double()
        if case.pre_bn:
            a = (a * torch.from_numpy(d['pre_scale']).double() + torch.from_numpy(d['pre_shift']).double()).float().double()
        return (a.clamp_min(0) if case.pre_relu else a).to(dtype)
    a = x.to(dtype)
    if case.pre_bn:
        a = a * torch.from_numpy(d['pre_scale']).to(dtype) + torch.from_numpy(d['pre_shift']).to(dtype)
    return a.clamp_min(0) if case.pre_relu else a


def epilogue(case, d, y, mag=False):
    import torch
    t = lambda n: torch.from_numpy(d[n]).to(y.dtype)
    f = (lambda v: v.abs()) if mag else (lambda v: v)
    if case.bn:
        y = y * f(t('post_scale')) + f(t('post_shift'))
    if case.res1:
        y = y + f(t('res1'))
    if case.res2:
        y = y + f(up2(t('res2')) if case.res2 == 'down' else t('res2'))
    return y.clamp_min(0) if case.relu and not mag else y


def statement(case, d, dtype, swap=None, mag=False, parts=0):
    """The layer at `dtype` -> float64 NumPy [N, OH, OW, Cout].  mag: the magnitude sum B.  parts: the split mode's E_P of the
    fp32 operand (bf16_modes_ref.conv_ep) in place of the exact products.  swap: one of SWAPS; None where the swap is the
    identity for this case, an array holding NaN where it changes the output's extents."""
    import torch
    g = case.geom()
    w = torch.from_numpy(d['w']).to(dtype)
    pro = None
    if swap == 'kh_kw':                                    # tap -> (kh, kw) decoded with the extents exchanged
        if case.KH == case.KW:
            return None
        g['KH'], g['KW'] = case.KW, case.KH
        w = w.reshape(case.KW, case.KH, case.Cin, case.Cout)
    elif swap == 'sh_sw':
        if case.SH == case.SW:
            return None
        g['SH'], g['SW'] = case.SW, case.SH
    elif swap == 'pt_pl':
        if case.PT == case.PL:
            return None
        g['PT'], g['PL'] = case.PL, case.PT
    elif swap == 'pb_is_pt':                               # the output extents a symmetric padding would give
        oh, ow = (case.H + 2 * case.PT - case.KH) // case.SH + 1, (case.W + 2 * case.PL - case.KW) // case.SW + 1
        if oh >= case.OH and ow >= case.OW:                 # (zero rows below are zero rows: the first OH x OW windows are the same)
            return None
        out = np.full((case.N, case.OH, case.OW, case.Cout), np.nan)
        oh, ow = max(min(oh, case.OH), 0), max(min(ow, case.OW), 0)
        out[:, :oh, :ow] = statement(case, d, dtype)[:, :oh, :ow]
        return out
    elif swap == 'pad_first':                              # zero padding applied BEFORE the BatchNormalization prologue
        if not case.pre_bn:
            return None
        ps, pb = torch.from_numpy(d['pre_scale']).to(dtype), torch.from_numpy(d['pre_shift']).to(dtype)
        pro = lambda v: (v * ps + pb).clamp_min(0) if case.pre_relu else v * ps + pb
        y = correlate(torch.from_numpy(d['x']).to(dtype), w, pro=pro, **g)
        if torch.equal(y, correlate(operand(case, d, dtype), w, **g)):
            return None                                    # (no window of the case reaches into the padding)
        return epilogue(case, d, y).double().numpy()
    if mag:
        y = correlate(operand(case, d, dtype).abs(), w.abs(), **g)
    elif parts:
        import bf16_modes_ref as R
        y = R.conv_ep(lambda u, v, s, p: correlate(u, v, **g), operand(case, d, dtype, exact_fma=True), w, None, None, parts)
    else:
        y = correlate(operand(case, d, dtype), w, **g)
    return epilogue(case, d, y, mag).double().numpy()


def bound(case, B, parts=0):
    """The bar per element (module docstring)."""
    return ((case.K + 8) * U24 + (SPLIT_TERM[parts] if parts else 0.0)) * B


@functools.lru_cache(maxsize=None)
def _truth(key):
    import torch
    case = _TABLE[key[0]]
    d = data(case)
    ref = statement(case, d, torch.float64)
    cpu = statement(case, d, torch.float32)
    return ref, statement(case, d, torch.float64, mag=True), cpu


def truth(case):
    """(fp64 statement, B, fp32 CPU statement) -- computed once per case."""
    return _truth(case.key())


def assert_signs(case, d, ref):
    """Where a ReLU is on, both signs occur in what it is applied to (ref: the fp64 statement)."""
    if case.pre_relu:
        a = d['x'] * d['pre_scale'] + d['pre_shift'] if case.pre_bn else d['x']
        assert (a > 0).any() and (a < 0).any(), case
    if case.relu:
        assert (ref > 0).any() and (ref == 0).any(), case


def worst(err, lim):
    """(largest err / lim, its index): an element with lim == 0 must be exact (ratio inf otherwise)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err <= lim, np.where(lim > 0, err / lim, 0.0), np.where(lim > 0, err / lim, np.inf))
    r = np.where(np.isnan(err), np.inf, r)
    i = int(np.argmax(r))
    return float(r.ravel()[i]), np.unravel_index(i, r.shape)


# ---- device side -----------------------------------------------------------------------------------------------------------------
def pack(case, w_hwio, ws, device='cuda'):
    """The weight in the packing w_split = ws asks for -> (device tensor, Kp, Np)."""
    import torch
    from deephar_amd import functional as F
    from deephar_amd.engine import packing
    if ws == 0:
        return F.pack_conv_weight(w_hwio, device)
    pk, kp, np_ = packing.pack_conv_halo(w_hwio) if ws == 2 else packing.pack_conv_split(w_hwio, parts=PARTS_OF[ws])
    return torch.from_numpy(pk).to(device), kp, np_


def fill_of(lib, case, ws, cfg):
    """What the slab around x holds: NaN wherever the kernel masks what lies outside its view, LOUD where the LDS-DMA family
    reads the padded k slots of a pixel from the floats behind it and multiplies them by zero weights (convview)."""
    rc, fam = family(lib, case, ws, cfg)
    return CV.LOUD if fam in ('dma', 'split') and case.Cin % 32 != 0 else np.nan


def launch(lib, case, w, ws=0, cfg=-1, what=''):
    """One dh_conv2d_f32 launch of the case on the views of its layout set -> (rc, route, y or None).  The library said what it
    would do before it launched; a refused launch has written nothing; the canaries around y are checked."""
    import torch
    d = data(case)
    v = CV.Views(case, d, case.lay(), fill_of(lib, case, ws, cfg))
    keep, tab = [], {}
    for n in (['pre_scale', 'pre_shift'] if case.pre_bn else []) + (['post_scale', 'post_shift'] if case.bn else []):
        t, tab[n] = CV.table(d[n], False)
        keep.append(t)
    wt, kp, np_ = w
    assert (kp, np_) == (case.Kp, case.Np), (case, kp, np_)
    a = set_geometry(CV.fill_args(case, v.ptr, v.ld, wt.data_ptr(), tab), case, ws)
    r = CV.route(lib, a, cfg)
    fake = CV.route(lib, fake_args(case, ws), cfg)
    assert (r.rc, r.kernel, r.tile_cfg) == (fake.rc, fake.kernel, fake.tile_cfg), (case, what)     # the host test saw this launch
    rc = lib.dh_conv2d_f32(C.byref(a), cfg, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == r.rc, '%s %s: dh_conv2d_f32 answered %d, dh_conv2d_route %d' % (case, what, rc, r.rc)
    if rc != 0:
        v.assert_nothing_written(what)
        return rc, r, None
    return rc, r, v.outputs(what)['y']


# ---- pooling and depthwise convolutions: the same windows --------------------------------------------------------------------------
class Win:
    """A pooling / depthwise launch: x [N, H, W, C] -> [N, OH, OW, C]."""

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def _axes(rng, h, w, kh, kw, sh, sw, kind):
    a, b = window(rng, h, kh, sh, kind), window(rng, w, kw, sw, kind)
    return None if a is None or b is None else (a, b)


def pool_cases(seed=7):
    """dh_pool2d_f32, modes 0 and 1: rectangular windows, SH != SW, explicit padding (24 cases; every third one TF-SAME or
    'valid' so that the old cells stay in)."""
    rng, out = np.random.default_rng(seed), []
    while len(out) < 24:
        kh, kw, sh, sw = (int(rng.integers(1, 4)) for _ in range(4))
        h, w, c = int(rng.integers(4, 20)), int(rng.integers(4, 20)), _pick(rng, (20, 7, 32))
        kind = ('explicit', 'explicit', 'same', 'explicit', 'explicit', 'valid')[len(out) % 6]
        ax = _axes(rng, h, w, kh, kw, sh, sw, kind)
        if ax is None or (kind == 'explicit' and kh == kw and sh == sw):
            continue
        (pt, pb, oh), (pl, pr, ow) = ax
        out.append(Win('pool_%02d_%dx%d_s%d%d_%s_m%d' % (len(out), kh, kw, sh, sw, kind, len(out) % 2), N=2, H=h, W=w, C=c, KH=kh, KW=kw,
                       SH=sh, SW=sw, PT=pt, PL=pl, OH=oh, OW=ow, mode=len(out) % 2))
    return out


def pool_ref(x, g):
    """Max (mode 0) or max + min (mode 1) over the pixels of a window that lie inside the frame, in fp32: exact."""
    n, h, w, c = x.shape
    out = np.empty((n, g.OH, g.OW, c), np.float32)
    for oh in range(g.OH):
        r0, r1 = max(oh * g.SH - g.PT, 0), min(oh * g.SH - g.PT + g.KH, h)
        for ow in range(g.OW):
            c0, c1 = max(ow * g.SW - g.PL, 0), min(ow * g.SW - g.PL + g.KW, w)
            assert r0 < r1 and c0 < c1, (g, oh, ow)
            win = x[:, r0:r1, c0:c1].reshape(n, -1, c)
            out[:, oh, ow] = win.max(axis=1) + win.min(axis=1) if g.mode else win.max(axis=1)
    return out


def dw_rows(w):
    """The band height of the LDS depthwise kernel on a tall map of width w (dw_lds.h: dw_lds_geometry): 64 threads at W = 8,
    256 otherwise = 8 channel quads x min(W, 32) / 8 strips x rows."""
    tw = min(w, 32)
    return (64 if tw == 8 else 256) // (8 * (tw // 8))


DW_WIDTHS = (8, 16, 24, 32, 40, 56)


def dw_cases(seed=11):
    """dh_dwconv2d_f32: k in {1, 3, 5}, the three prologues, the widths of the LDS kernel's column tilings (24: three strips and
    10-row bands; 40 and 56: a last column tile 8 and 24 wide), heights around its band, explicit PT / PL in [0, k) (every
    third case TF-SAME), up_in where the extents are even.  C = 36 or 68: the test runs the first C - 4 channels (the LDS
    kernel where k > 1), all C on an aligned view (the strip kernel) and on an odd view (the generic kernel)."""
    rng, out = np.random.default_rng(seed), []
    pres = ('none', 'relu', 'bnrelu')
    i = 0
    for k in (1, 3, 5):
        for w in DW_WIDTHS:
            rows = dw_rows(w)
            for h in (1, rows - 1, rows, rows + 1, 2 * rows + 3):
                if k == 1 and h not in (1, rows, rows + 1):
                    continue
                i += 1
                pt, pl = ((k - 1) // 2, (k - 1) // 2) if i % 3 == 0 else (int(rng.integers(0, k)), int(rng.integers(0, k)))
                c = (36, 68)[i % 2]
                up = h % 2 == 0
                out.append(Win('dw_k%d_%dx%d_c%d_p%d%d_%s%s' % (k, h, w, c, pt, pl, pres[i % 3], '_up' if up else ''), N=2, H=h, W=w, C=c,
                               KH=k, KW=k, SH=1, SW=1, PT=pt, PL=pl, OH=h, OW=w, pre=pres[i % 3], up_in=up))
    return out


def dws_cases(seed=13):
    """dh_dwconv2d_strided_f32 (stride 2, k in {3, 5}): odd H and W, explicit PT / PL."""
    rng, out = np.random.default_rng(seed), []
    pres = ('none', 'relu', 'bnrelu')
    while len(out) < 12:
        k = (3, 5)[len(out) % 2]
        h, w, c = 2 * int(rng.integers(2, 9)) + 1, 2 * int(rng.integers(2, 9)) + 1, (32, 36, 35)[len(out) % 3]
        ax = _axes(rng, h, w, k, k, 2, 2, 'explicit' if len(out) % 4 else 'same')
        if ax is None:
            continue
        (pt, pb, oh), (pl, pr, ow) = ax
        out.append(Win('dws_k%d_%dx%d_c%d_p%d%d_%s' % (k, h, w, c, pt, pl, pres[len(out) % 3]), N=2, H=h, W=w, C=c, KH=k, KW=k, SH=2,
                       SW=2, PT=pt, PL=pl, OH=oh, OW=ow, pre=pres[len(out) % 3], up_in=False))
    return out


def dw_data(g):
    rng = np.random.default_rng(zlib.crc32(g.name.encode()))
    cs = channel_scales(rng, g.C, 3)
    h, w = (g.H // 2, g.W // 2) if g.up_in else (g.H, g.W)
    d = {'x': _gauss(rng, (g.N, h, w, g.C)) * cs, 'w': _gauss(rng, (g.KH, g.KW, g.C), 1.0 / g.KH) * channel_scales(rng, g.C, 6)}
    if g.pre == 'bnrelu':
        d['pre_scale'], d['pre_shift'] = rng.uniform(0.5, 1.5, g.C).astype(np.float32), _gauss(rng, (g.C,), 0.3) * cs
    return d


def dw_statement(g, d, dtype, mag=False):
    """The depthwise layer from the definition, channel by channel through `correlate` -> float64 NumPy.  An up-sampled input is
    written out (UpSampling2D((2, 2))) first."""
    import torch
    a = torch.from_numpy(d['x']).to(dtype)
    if g.up_in:
        a = up2(a)
    if g.pre == 'bnrelu':                          # at fp32 the kernels' fused multiply-add: one rounding (an unfused x s + b loses
        # everything where x s ~ -b, and B, built on |pro(x)|, is small just there)
        a = (a.double() * torch.from_numpy(d['pre_scale']).double() + torch.from_numpy(d['pre_shift']).double()).to(dtype)
    if g.pre != 'none':
        a = a.clamp_min(0)
    w = torch.from_numpy(d['w']).to(dtype)
    if mag:
        a, w = a.abs(), w.abs()
    ys = [correlate(a[..., ch:ch + 1], w[:, :, ch].reshape(g.KH, g.KW, 1, 1), g.KH, g.KW, g.SH, g.SW, g.PT, g.PL, g.OH, g.OW)
          for ch in range(g.C)]
    return torch.cat(ys, dim=-1).double().numpy()


# (name, channels left out, layout) -> the kernel a depthwise case runs on: the LDS-tiled one (C % 32 == 0, k > 1), the strip
# kernel (C % 4 == 0, 16-byte aligned views), the generic one
DW_VARIANTS = (('lds', 4, 'dense'), ('strip', 0, 'aligned'), ('generic', 0, 'odd'))


def dw_fake_args(g, chans, layname):
    """dh_dw_args of a variant on fake pointers of the layout's alignment (dh_dwconv2d_uses_lds_kernel dereferences none)."""
    from deephar_amd import _lib
    (ldx, ox), (ldy, oy) = SV.layout(chans, layname, 0), SV.layout(chans, layname, 1)
    a = _lib.DwArgs()
    a.x, a.w, a.y = 0x100000 + 4 * ox, 0x200000, 0x300000 + 4 * oy
    if g.pre == 'bnrelu':
        a.pre_scale, a.pre_shift = 0x400000, 0x500000
    a.N, a.H, a.W, a.C, a.ldx, a.ldy, a.KH, a.KW, a.PT, a.PL = g.N, g.H, g.W, chans, ldx, ldy, g.KH, g.KW, g.PT, g.PL
    a.pre_relu, a.up_in = int(g.pre != 'none'), int(g.up_in)
    return a


def dw_bound(g, B):
    """(k k + 4) 2^-24 B: k k fused multiply-adds, the prologue's fused multiply-add."""
    return (g.KH * g.KW + 4) * U24 * B
