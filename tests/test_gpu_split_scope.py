"""The extended scope of the split-bf16 ladder: dh_conv_args.w_split = 5 / 6 / 7 (csrc/gemm1x1s_ext.hip) and Model.gemm_scope =
'extended' -- pointwise convolutions with a BatchNormalization prologue and K x K convolutions with Cin % 16 == 0.

The contract is the one of tests/bf16_modes_ref.py, with the operand split AFTER the prologue and the ReLU:
a = relu?(fmaf(x, pre_scale, pre_shift)) in fp32, the operand of the fp32 kernel.  The tests:
  1. operands built so that every kept product and partial sum is exact in fp32: every tiling equals E_P bit for bit;
  2. random operands, every fused variant: within twice the shipped fp32 kernel's own error of E_P + epilogue in fp64;
  3. bit-equal across tilings, positions in the batch, packed-weight hand-in, channel slabs; code 5 / 6 / 7 == 1 / 3 / 4 on
     a layer of the standard scope;
  4. refusals;
  5. whole models against the fp64 oracle, bar from a CPU emulation of the mode: max(1e-3 px, 2 x emu_px);
  6. batch invariance of the model;
  7. an exported plan run by the C executor reproduces predict bit for bit, in the blob version of the standard scope.
Shapes are (N, H, W, Cin, Cout); every map has more than 256 output positions per frame (no skinny layer)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_modes_ref as R                          # noqa: E402
import split_scope_ref as SR                        # noqa: E402
from oracle import ops as O                         # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ('bf16x3', 'bf16x2', 'bf16')
UNSUPPORTED = 'rc=-2'


def _rand(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _tilings(hip_lib, run, need=3):
    """run(cfg) on the library's pick and on every tiling index of the split family; DH_EUNSUPPORTED (rc=-2) is the only
    refusal allowed, and never of the library's own pick.  -> {cfg: result}"""
    outs = {-1: run(-1)}
    for cfg in range(hip_lib.dh_conv2d_num_split_tile_cfgs()):
        try:
            outs[cfg] = run(cfg)
        except Exception as e:
            assert UNSUPPORTED in str(e), e
    torch.cuda.synchronize()
    assert len(outs) >= 1 + need, sorted(outs)
    return outs


# ---- 1. known answers, no tolerance ------------------------------------------------------------------------------------
# (N, H, W, Cin, Cout), (kh, kw), stride, BN prologue
EXACT_CASES = [
    ((2, 20, 16, 288, 96), (1, 1), 1, True),
    ((1, 20, 16, 48, 20), (1, 1), 1, True),
    ((3, 17, 19, 36, 24), (1, 1), 1, True),
    ((2, 20, 16, 16, 32), (3, 3), 1, False),      # K = 144: every K-step holds two taps
    ((1, 20, 16, 48, 32), (1, 5), 1, False),      # K = 240: a step straddles a tap boundary
    ((1, 40, 36, 16, 32), (3, 3), 2, False),
]


@pytest.mark.parametrize('mode', ['bf16x2', 'bf16'])
@pytest.mark.parametrize('case,ks,stride,bn', EXACT_CASES)
def test_known_answers_bit_for_bit(case, ks, stride, bn, mode, hip_lib, cuda):
    from deephar_amd import functional as F
    n, h, w, cin, cout = case
    kh, kw = ks
    assert kh * kw * cin <= 288 and -(-h // stride) * -(-w // stride) > 256
    rng = np.random.default_rng(sum(case) + kh + 10 * kw)
    xh, xl = SR.exact_operand(rng, (n, h, w, cin))
    wh, wl = SR.exact_operand(rng, (kh, kw, cin, cout))
    x, k = xh + xl, wh + wl
    t = lambda a: torch.from_numpy(a).double()
    if bn:                                         # scale in {1, 2}, shift 0, ReLU on: relu(ps * x) splits to (ps * hi, ps * lo, 0), masked
        ps = rng.choice(np.array([1.0, 2.0], np.float32), cin)
        pb = np.zeros(cin, np.float32)
        a = SR.operand(x, ps, pb, True)
        pos = (x > 0).astype(np.float32)
        ah, al = xh * ps * pos, xl * ps * pos
    else:
        ps = pb = None
        a = SR.operand(x)
        ah, al = xh, xl
    p = R.split_parts(a, 3)                        # the construction does what it says
    assert torch.equal(p[0], torch.from_numpy(ah)) and torch.equal(p[1], torch.from_numpy(al)) and not p[2].any()
    p = R.split_parts(torch.from_numpy(k), 3)
    assert torch.equal(p[0], torch.from_numpy(wh)) and torch.equal(p[1], torch.from_numpy(wl)) and not p[2].any()
    conv = lambda u, v: O.conv2d(u, v, (stride, stride), 'same')
    e = {'bf16': conv(t(ah), t(wh)), 'exact': conv(a.double(), t(k))}
    e['bf16x2'] = e['bf16'] + conv(t(al), t(wh)) + conv(t(ah), t(wl))
    for name in ('bf16', 'bf16x2'):
        assert torch.equal(e[name], R.conv_ep(O.conv2d, a.double(), t(k), (stride, stride), 'same', R.PARTS[name])), name
        assert torch.equal(e[name].float().double(), e[name])      # representable: the fp32 result can be the fp64 one
    for u in e:                                    # the case tells E_1, E_2 and the exact product apart (CPU references)
        for v in e:
            if u < v:
                assert float((e[u] != e[v]).double().mean()) > 0.9, (u, v)
    d = lambda v: None if v is None else torch.from_numpy(v).to(cuda)
    kw_ = dict(strides=(stride, stride), padding='same', pre_scale=d(ps), pre_shift=d(pb), pre_relu=bn)
    outs = _tilings(hip_lib, lambda cfg: F.conv2d(d(x), k, precision=mode, scope='extended', tile_cfg=cfg, **kw_))
    for cfg, y in outs.items():
        y = y.cpu().double()
        bad = int((y != e[mode]).sum())
        assert bad == 0, '%s tiling %d: %d of %d outputs differ from E_P, worst %.3e' % (
            mode, cfg, bad, y.numel(), float((y - e[mode]).abs().max()))
    y = outs[-1].cpu().double()
    for other in e:
        if other != mode:
            frac = float((y != e[other]).double().mean())
            assert frac > 0.9, 'E(%s) equals E(%s) on %.1f %% of the outputs' % (mode, other, 100 - 100 * frac)


# ---- 2. random operands, every fused variant ---------------------------------------------------------------------------
RANDOM_CASES = [
    ((2, 24, 24, 48, 96), (3, 3), 1, False),       # K = 432, K % 32 == 16: the last half-step is padding
    ((1, 32, 32, 144, 64), (3, 3), 1, False),      # the halo kernel in fp32
    ((2, 40, 36, 48, 64), (3, 3), 2, False),       # stride 2, TF-SAME padding
    ((1, 20, 16, 16, 40), (5, 1), 1, False),
    ((2, 20, 16, 80, 33), (1, 5), 1, False),       # Cout = 33: the scalar store path
    ((2, 32, 32, 64, 64), (1, 1), 1, True),        # the very call the standard codes refuse
    ((2, 20, 16, 48, 576), (1, 1), 1, True),
    ((1, 24, 24, 576, 96), (1, 1), 1, True),
    ((3, 17, 19, 36, 24), (1, 1), 1, True),
    ((1, 20, 16, 4096, 32), (1, 1), 1, True),      # the largest table
]
# name -> (ReLU prologue, post-BN, res1, res2, post-ReLU, pooled second output)
VARIANTS = [('plain', (0, 0, 0, 0, 0, 0)), ('relu prologue', (1, 0, 0, 0, 0, 0)), ('post-BN', (0, 1, 0, 0, 0, 0)),
            ('res1', (1, 1, 1, 0, 0, 0)), ('res2', (0, 1, 1, 1, 0, 0)), ('post-ReLU', (1, 1, 1, 0, 1, 0)),
            ('pooled', (1, 1, 1, 0, 1, 1))]


@pytest.mark.parametrize('case,ks,stride,bn', RANDOM_CASES)
def test_random_operands_every_fused_variant(case, ks, stride, bn, hip_lib, cuda):
    """Against E_P of the post-prologue operand + epilogue in fp64.  Bar: |hip - E_P| <= 2 x |shipped fp32 kernel - fp64| + 1e-6
    on the same inputs (tests/test_gpu_bf16_modes.py).  For P <= 2 the result is nearer to E_P than to the fp64 truth and is
    not the fp32 answer.  Every tiling gives the same bits."""
    from deephar_amd import functional as F
    n, h, w, cin, cout = case
    kh, kw = ks
    oh, ow = -(-h // stride), -(-w // stride)
    assert oh * ow > 256
    rng = np.random.default_rng(sum(case) + kh + 10 * kw)
    x = _rand(rng, (n, h, w, cin))
    k = _rand(rng, (kh, kw, cin, cout), np.sqrt(1.0 / (kh * kw * cin)))
    ps = rng.uniform(0.5, 1.5, cin).astype(np.float32) if bn else None
    pb = _rand(rng, (cin,), 0.3) if bn else None
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), _rand(rng, (cout,), 0.1)
    r1, r2 = _rand(rng, (n, oh, ow, cout)), _rand(rng, (n, oh, ow, cout))
    t = lambda a: torch.from_numpy(a).double()
    d = lambda a: None if a is None else torch.from_numpy(a).to(cuda)
    conv = lambda u, v, s_=None, p_=None: O.conv2d(u, v, (stride, stride), 'same')
    can_pool = (ow == 32 or (ow in (16, 8) and (oh * ow) % 32 == 0)) and oh % 2 == 0 and cout % 4 == 0
    # the convolutions once per prologue: fp64 truth and E_P of every mode
    base = {}
    for relu in (0, 1):
        a = SR.operand(x, ps, pb, bool(relu)).double()
        truth_in = t(x) * t(ps) + t(pb) if bn else t(x)
        truth_in = O.relu(truth_in) if relu else truth_in
        base[relu] = dict(truth=conv(truth_in, t(k)),
                          **{mode: R.conv_ep(conv, a, t(k), None, None, R.PARTS[mode]) for mode in MODES})
    failures = []
    pooled_seen = False
    for name, (relu, post, has_r1, has_r2, post_relu, pool) in VARIANTS:
        if pool and not can_pool:
            continue
        pooled_seen |= bool(pool)

        def epilogue(y):
            y = y * t(sc) + t(sh) if post else y
            y = y + t(r1) if has_r1 else y
            y = y + t(r2) if has_r2 else y
            return O.relu(y) if post_relu else y
        kw_ = dict(strides=(stride, stride), padding='same', pre_scale=d(ps), pre_shift=d(pb), pre_relu=bool(relu),
                   post_scale=d(sc) if post else None, post_shift=d(sh) if post else None, res1=d(r1) if has_r1 else None,
                   res2=d(r2) if has_r2 else None, post_relu=bool(post_relu))
        truth = epilogue(base[relu]['truth'])
        f32 = F.conv2d(d(x), k, **kw_)             # the shipped fp32 kernel (not code under test)
        e_f32 = (f32.cpu().double() - truth).abs().max().item()
        for mode in MODES:
            ref = epilogue(base[relu][mode])
            outs = _tilings(hip_lib, lambda cfg: F.conv2d(d(x), k, precision=mode, scope='extended', tile_cfg=cfg,
                                                          pool2=bool(pool), **kw_))
            if pool:
                for cfg, (y, yp) in outs.items():
                    assert torch.equal(yp, F.pool2d(y, (2, 2))), (name, mode, cfg)
                outs = {cfg: y for cfg, (y, yp) in outs.items()}
                assert torch.equal(outs[-1], F.conv2d(d(x), k, precision=mode, scope='extended', **kw_))
            first = outs[-1]
            for cfg, y in outs.items():
                assert torch.equal(y, first), '%s %s tiling %d differs' % (name, mode, cfg)
            e_mode = (first.cpu().double() - ref).abs().max().item()
            e_true = (first.cpu().double() - truth).abs().max().item()
            print('%s %s stride %d %s %s: |hip - E_P| = %.3e   |fp32 kernel - fp64| = %.3e   |hip - fp64| = %.3e   tilings %s' % (
                case, ks, stride, name, mode, e_mode, e_f32, e_true, sorted(outs)))
            if not e_mode <= 2.0 * e_f32 + 1e-6:
                failures.append((name, mode, 'bar', e_mode, e_f32))
            if R.PARTS[mode] <= 2:
                if not e_mode < e_true:
                    failures.append((name, mode, 'not E_P', e_mode, e_true))
                assert not torch.equal(first, f32), (name, mode)
    assert pooled_seen == can_pool
    assert not failures, failures


# ---- 3. invariance -----------------------------------------------------------------------------------------------------
INVARIANCE_CASES = [((3, 24, 24, 48, 96), (3, 3), 1, False), ((3, 40, 36, 48, 64), (3, 3), 2, False),
                    ((3, 20, 16, 80, 33), (1, 5), 1, False), ((3, 17, 19, 36, 24), (1, 1), 1, True),
                    ((3, 20, 16, 48, 576), (1, 1), 1, True)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case,ks,stride,bn', INVARIANCE_CASES)
def test_bits_depend_on_the_mode_and_the_geometry_only(case, ks, stride, bn, mode, hip_lib, cuda):
    from deephar_amd import functional as F
    from deephar_amd.engine import packing
    n, h, w, cin, cout = case
    kh, kw = ks
    oh, ow = -(-h // stride), -(-w // stride)
    rng = np.random.default_rng(5 + sum(case))
    x = _rand(rng, (n, h, w, cin))
    k = _rand(rng, (kh, kw, cin, cout), np.sqrt(1.0 / (kh * kw * cin)))
    ps = rng.uniform(0.5, 1.5, cin).astype(np.float32) if bn else None
    pb = _rand(rng, (cin,), 0.3) if bn else None
    r1 = _rand(rng, (n, oh, ow, cout))
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    kw_ = dict(strides=(stride, stride), padding='same', pre_scale=d(ps), pre_shift=d(pb), pre_relu=True, precision=mode,
               scope='extended')
    full = F.conv2d(d(x), k, res1=d(r1), **kw_)
    one = F.conv2d(d(x[:1]), k, res1=d(r1[:1]), **kw_)
    last = F.conv2d(d(x[-1:]), k, res1=d(r1[-1:]), **kw_)
    assert torch.equal(full[:1], one) and torch.equal(full[-1:], last)
    outs = _tilings(hip_lib, lambda cfg: F.conv2d(d(x), k, res1=d(r1), tile_cfg=cfg, **kw_))
    for cfg, y in outs.items():
        assert torch.equal(y, full), cfg
    for cfg in outs:
        assert torch.equal(F.conv2d(d(x[:1]), k, res1=d(r1[:1]), tile_cfg=cfg, **kw_), one), cfg
    # a packed weight handed in gives the same bits as packing on the fly
    pk, kp, np_ = packing.pack_conv_split(k, parts=R.PARTS[mode])
    packed = (torch.from_numpy(pk).to(cuda), kp, np_)
    plain = F.conv2d(d(x), k, **kw_)
    assert torch.equal(F.conv2d(d(x), k, packed=packed, **kw_), plain)
    # channel slabs: ldx > Cin (the padded k slots of a pixel would read the slab's neighbours), ldy > Cout; the padding stays
    code = SR.WIDE_CODES[mode]
    xw = d(np.concatenate([x, np.full((n, h, w, 8), 3.0, np.float32)], axis=-1))
    pre = (d(ps), d(pb)) if bn else None
    for pad_y in (12, 1, 5):                       # (a pitch that is no multiple of four: the scalar store path)
        for cfg in (-1, min(c for c in outs if c >= 0), max(outs)):
            out = torch.full((n, oh, ow, cout + pad_y), 7.0, device=cuda)
            assert SR.conv_on_views(hip_lib, xw, cin, packed, cout, kh, kw, stride, code, out, cfg, pre=pre, pre_relu=True) == 0
            assert torch.equal(out[..., :cout], plain), (pad_y, cfg)
            assert torch.all(out[..., cout:] == 7.0), (pad_y, cfg)


@pytest.mark.parametrize('mode', MODES)
def test_a_standard_layer_has_the_bits_of_the_standard_code(mode, hip_lib, cuda):
    """Code 5 / 6 / 7 on a layer dh_conv2d_split_eligible takes equals code 1 / 3 / 4 bit for bit, in every tiling."""
    from deephar_amd import functional as F
    rng = np.random.default_rng(9)
    for (n, h, w, cin, cout), ks, stride, up2 in (((2, 32, 32, 96, 200), 1, 1, False), ((2, 35, 33, 64, 72), 3, 1, False),
                                                   ((1, 40, 36, 32, 64), 3, 2, False), ((2, 16, 32, 288, 96), 1, 1, True)):
        x = torch.from_numpy(_rand(rng, (n, h, w, cin))).to(cuda)
        k = _rand(rng, (ks, ks, cin, cout), np.sqrt(1.0 / (ks * ks * cin)))
        oh, ow = -(-h // stride), -(-w // stride)
        r2 = torch.from_numpy(_rand(rng, (n, 2 * oh, 2 * ow, cout))).to(cuda) if up2 else None
        kw_ = dict(strides=(stride, stride), pre_relu=True, precision=mode, up2=up2, res2=r2)
        std = _tilings(hip_lib, lambda cfg: F.conv2d(x, k, tile_cfg=cfg, **kw_))
        ext = _tilings(hip_lib, lambda cfg: F.conv2d(x, k, tile_cfg=cfg, scope='extended', **kw_))
        assert sorted(std) == sorted(ext)
        for cfg in std:
            assert torch.equal(std[cfg], ext[cfg]) and torch.equal(std[cfg], std[-1]), cfg
    x = torch.from_numpy(_rand(rng, (2, 32, 32, 96))).to(cuda)
    k = _rand(rng, (1, 1, 96, 64), 0.1)
    assert torch.equal(F.conv2d(x, k, scope='extended'), F.conv2d(x, k))            # no effect under 'f32'


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib, cuda):
    from deephar_amd import functional as F
    from deephar_amd._lib import DeepharHipError
    z = lambda *s: torch.randn(*s, device=cuda)
    kz = lambda *s: np.zeros(s, np.float32)
    ones, zeros = (lambda c: torch.ones(c, device=cuda)), (lambda c: torch.zeros(c, device=cuda))
    for mode in MODES:
        kw_ = dict(precision=mode, scope='extended')
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # 3 x 3 with Cin = 24
            F.conv2d(z(2, 32, 32, 24), kz(3, 3, 24, 96), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # Kp = kMaxPreKp + 32
            F.conv2d(z(1, 20, 16, 4128), kz(1, 1, 4128, 32), pre_scale=ones(4128), pre_shift=zeros(4128), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # 3 x 3 with a BN prologue
            F.conv2d(z(2, 32, 32, 64), kz(3, 3, 64, 96), pre_scale=ones(64), pre_shift=zeros(64), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):
            F.conv2d(z(2, 32, 32, 48), kz(3, 3, 48, 96), pre_scale=ones(48), pre_shift=zeros(48), **kw_)
        with pytest.raises(DeepharHipError, match='rc=-1'):             # scale without shift: an invalid call for every code
            F.conv2d(z(2, 32, 32, 64), kz(1, 1, 64, 64), pre_scale=ones(64), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # a skinny layer (8 x 8 map, 128 channels)
            F.conv2d(z(2, 8, 8, 288), kz(1, 1, 288, 128), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # ... with a BN prologue
            F.conv2d(z(2, 8, 8, 288), kz(1, 1, 288, 128), pre_scale=ones(288), pre_shift=zeros(288), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # ... K x K with Cin = 48
            F.conv2d(z(2, 16, 16, 48), kz(3, 3, 48, 96), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # Cin = 3
            F.conv2d(z(1, 16, 16, 3), kz(3, 3, 3, 32), **kw_)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # uint8 frames
            F.conv2d(torch.zeros((1, 32, 32, 48), dtype=torch.uint8, device=cuda), kz(3, 3, 48, 32),
                     in_lut=torch.zeros((48, 256), device=cuda), **kw_)
        # ldx % 4 != 0: a pointwise layer on a view with a pixel pitch of 578 floats
        xs = torch.zeros((2, 32, 32, 578), device=cuda)
        out = torch.full((2, 32, 32, 64), 7.0, device=cuda)
        from deephar_amd.engine import packing
        pk, kp, np_ = packing.pack_conv_split(kz(1, 1, 576, 64), parts=R.PARTS[mode])
        w = (torch.from_numpy(pk).to(cuda), kp, np_)
        assert SR.conv_on_views(hip_lib, xs, 576, w, 64, 1, 1, 1, SR.WIDE_CODES[mode], out) == -2
        assert torch.all(out == 7.0)
        assert SR.conv_on_views(hip_lib, xs, 576, w, 64, 1, 1, 1, 8, out) == -1          # w_split = 8: DH_EINVAL
        assert SR.conv_on_views(hip_lib, xs[..., :576].contiguous(), 576, w, 64, 1, 1, 1, 8, out) == -1
        assert torch.all(out == 7.0)
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # the standard codes still refuse the BN-prologue call
            F.conv2d(z(2, 32, 32, 64), kz(1, 1, 64, 64), precision=mode, pre_scale=ones(64), pre_shift=zeros(64))
        with pytest.raises(DeepharHipError, match=UNSUPPORTED):         # ... and K x K with Cin = 48
            F.conv2d(z(2, 32, 32, 48), kz(3, 3, 48, 96), precision=mode)
    with pytest.raises(ValueError):
        F.conv2d(z(2, 32, 32, 64), kz(1, 1, 64, 64), precision='bf16', scope='wide')


# ---- 5. models ---------------------------------------------------------------------------------------------------------
def _predict(m, x, n, mode, scope):
    m.gemm_precision, m.gemm_scope = mode, scope
    m.executor.autotune = False                    # (every tiling gives the same bits; keeps the test to seconds)
    out = m.predict(x, batch_size=n)
    return out if isinstance(out, list) else [out]


def _counts(m):
    cc = SR.conv_codes(m)
    split = sum(1 for _, _, c in cc if c in (1, 3, 4, 5, 6, 7))
    odd = sum(1 for s, cin, c in cc if cin % 32 != 0 and c >= 5)
    bn_pw = sum(1 for s, cin, c in cc if c >= 5 and 'pre_bn' in s.params and s.attrs['kh'] == s.attrs['kw'] == 1)
    return split, odd, bn_pw


@pytest.fixture(scope='module')
def spnet_case():
    m, x, oracle, readout = SR.spnet_case()
    return m, x, oracle, readout, oracle(torch.float64)


def _model_body(m, x, n, oracle, poses, actions, o64, emulate, monkeypatch, name, min_odd, min_bn):
    f32 = _predict(m, x, n, 'f32', 'standard')
    assert all(np.array_equal(a, b) for a, b in zip(_predict(m, x, n, 'f32', 'extended'), f32))      # no effect under 'f32'
    failures = []
    for mode in MODES:
        with monkeypatch.context() as mp:
            emulate(mp, R.PARTS[mode])
            emu = oracle(torch.float64)
        emu_px = R.px(poses(emu), poses(o64))
        assert np.isfinite(emu_px)
        std = _predict(m, x, n, mode, 'standard')
        nstd = _counts(m)[0]
        assert all(c in (0, 2, SR.CODES[mode]) for _, _, c in SR.conv_codes(m))
        hip = _predict(m, x, n, mode, 'extended')
        nsplit, odd, bn_pw = _counts(m)
        assert all(c in (0, 2, SR.WIDE_CODES[mode]) for _, _, c in SR.conv_codes(m))
        assert odd >= min_odd and bn_pw >= min_bn and nsplit > nstd, (odd, bn_pw, nsplit, nstd)
        assert all(np.all(np.isfinite(v)) for v in hip)
        assert any(not np.array_equal(a, b) for a, b in zip(hip, std)), 'the extended plan returned the standard plan\'s bits'
        assert any(not np.array_equal(a, b) for a, b in zip(hip, f32)), 'the extended plan returned the fp32 plan\'s bits'
        hip_px, std_px = R.px(poses(hip), poses(o64)), R.px(poses(std), poses(o64))
        labels = sum(int((a.argmax(-1) != b.argmax(-1)).sum()) for a, b in zip(actions(hip), actions(o64)))
        bar = max(1e-3, 2.0 * emu_px)
        print(json.dumps(dict(case=name, mode=mode, scope='extended', emu_px=emu_px, bar_px=bar, hip_vs_o64_px=hip_px,
                              standard_scope_vs_o64_px=std_px, f32_path_vs_o64_px=R.px(poses(f32), poses(o64)),
                              labels_differ=labels, split_convs=nsplit, split_convs_standard=nstd, odd_cin_wide=odd,
                              bn_pointwise_wide=bn_pw)))
        if hip_px > bar:
            failures.append('%s %s: %.3e px from the fp64 oracle, bar %.3e px (emulation %.3e px)' % (name, mode, hip_px, bar, emu_px))
    assert not failures, failures


def test_spnet_within_the_emulated_bar(spnet_case, hip_lib, cuda, monkeypatch):
    """Pose SPNet, growth 96, two pyramids, 8 frames.  At 256 px: the entry flow's 144-channel 3 x 3 convolutions run on
    32 x 32 maps (at 128 px they run on 16 x 16 maps, are skinny layers and stay fp32 under every scope).  Per mode emu_px =
    distance of the extended emulation (tests/split_scope_ref.py) from the fp64 oracle; the engine under 'extended' stays within
    max(1e-3 px, 2 x emu_px) of the fp64 oracle."""
    m, x, oracle, readout, o64 = spnet_case
    _model_body(m, x, len(x), oracle, readout, lambda o: [], o64, SR.emulate, monkeypatch, 'spnet_growth96', 3, 8)


def test_ntu_within_the_emulated_bar(hip_lib, cuda, monkeypatch):
    """The 'ntu' case of bf16_modes_ref.model_case under 'extended', against the existing emulation (which evaluates every
    pointwise convolution as E_P, BN prologue or not).  Labels are reported, not asserted."""
    m, x, n, oracle, poses, actions = R.model_case('ntu')
    _model_body(m, x, n, oracle, poses, actions, oracle(torch.float64), R.emulate, monkeypatch, 'ntu', 0, 8)


# ---- 6. batch invariance of the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_model_batch_invariance_is_bit_exact(mode, spnet_case, hip_lib, cuda):
    m, x = spnet_case[0], spnet_case[1][:4]
    a = _predict(m, x, 4, mode, 'extended')
    assert _counts(m)[1] >= 3
    b = _predict(m, x, 2, mode, 'extended')
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


# ---- 7. exported plan ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['bf16', 'bf16x3'])
def test_c_plan_reproduces_predict(mode, spnet_case, hip_lib, cuda, tmp_path):
    m, x = spnet_case[0], spnet_case[1][:2]
    n = len(x)
    _predict(m, x, n, mode, 'standard')
    std_path = str(tmp_path / 'standard.dhplan')
    m.export_plan(std_path, n)
    std_version = int.from_bytes(open(std_path, 'rb').read()[4:8], 'little')
    ref = _predict(m, x, n, mode, 'extended')
    assert _counts(m)[1] >= 3 and _counts(m)[2] >= 8
    path = str(tmp_path / 'extended.dhplan')
    nbytes = m.export_plan(path, n)
    blob = open(path, 'rb').read()
    assert len(blob) == nbytes and blob[:4] == b'DHPL'
    assert int.from_bytes(blob[4:8], 'little') == std_version and std_version in (2, 3, 4)
    plan = C.c_void_p()
    assert hip_lib.dh_plan_create(blob, len(blob), C.byref(plan)) == 0
    try:
        assert hip_lib.dh_plan_batch(plan) == n and hip_lib.dh_plan_num_outputs(plan) == len(ref)
        xd = torch.from_numpy(x).to(cuda)
        outs = [torch.full(r.shape, float('nan'), device=cuda) for r in ref]
        ins_p = (C.c_void_p * 1)(xd.data_ptr())
        outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        assert hip_lib.dh_forward(plan, ins_p, n, outs_p, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        for o, r in zip(outs, ref):
            assert np.array_equal(o.cpu().numpy(), r)
        host = [np.full(r.shape, np.nan, np.float32) for r in ref]
        ins_h = (C.c_void_p * 1)(x.ctypes.data)
        outs_h = (C.c_void_p * len(host))(*[h_.ctypes.data for h_ in host])
        assert hip_lib.dh_forward_host(plan, ins_h, n, outs_h) == 0
        for h_, r in zip(host, ref):
            assert np.array_equal(h_, r)
    finally:
        assert hip_lib.dh_plan_destroy(plan) == 0
