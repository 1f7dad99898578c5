"""The reduced-precision rungs of the split-bf16 GEMM family: Model.gemm_precision = 'bf16x2' (two bf16 parts per operand,
three products) and 'bf16' (one part, one product) -- dh_conv_args.w_split = 3 / 4, csrc/gemm1x1s.hip.

A mode is a DEFINITION (tests/bf16_modes_ref.py): operands split by repeated round-to-nearest-even, E_P = the products with
i + j <= P + 1, exact products, fp32 accumulation, the unchanged fp32 epilogue.  The tests hold the kernels to it:
  1. operands built so that every kept product and every partial sum is exact in fp32: the kernel must equal E_P bit for bit;
  2. random operands, every epilogue: within the fp32 accumulation's error of E_P + epilogue evaluated in fp64;
  3. bit-equal across tilings, batch sizes, positions in the batch and repeated calls;
  4. whole models against the fp64 oracle, the bar taken from a CPU emulation of the mode: max(1e-3 px, 2 x emu_px);
  5. an exported plan run by the C executor reproduces predict bit for bit.
Records of (4) join the session's parity table (paritylog.record) and, when DEEPHAR_PARITY_BF16_MODES names a file, are
written there on their own (kept as profiles/parity_bf16_modes.json)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_modes_ref as R                          # noqa: E402
import paritylog                                    # noqa: E402
from oracle import ops as O                         # noqa: E402
from test_gpu_ops import SPLIT_CASES, _rand         # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ('bf16x2', 'bf16')
MODEL_RECORDS = []


def _tilings(hip_lib, run):
    """run(cfg) on the library's pick and on every tiling index of the split family; DH_EUNSUPPORTED (rc=-2) is the only
    refusal allowed.  -> {cfg: result}"""
    outs = {}
    for cfg in range(-1, hip_lib.dh_conv2d_num_split_tile_cfgs()):
        try:
            outs[cfg] = run(cfg)
        except Exception as e:
            assert 'rc=-2' in str(e), e
    torch.cuda.synchronize()
    return outs


# ---- 1. known answers, no tolerance ------------------------------------------------------------------------------------
def _exact_operand(rng, shape):
    """hi + lo with hi in {+-1, +-1.5}, lo in +-{4, 5, 6, 7} * 2^-12: the RNE split is exactly (hi, lo, 0); every kept term of
    P <= 2 is a multiple of 2^-13 and sum |terms| < 2^24 * 2^-13 up to K = 576, so any fp32 accumulation order is exact."""
    hi = rng.choice(np.array([1.0, -1.0, 1.5, -1.5], np.float32), shape)
    lo = (rng.integers(4, 8, shape) * rng.choice(np.array([1, -1]), shape)).astype(np.float32) * np.float32(2.0 ** -12)
    return hi, lo


EXACT_CASES = [(2, 32, 32, 576, 576, 1), (3, 16, 16, 288, 288, 1), (5, 8, 8, 288, 288, 1), (2, 32, 32, 64, 96, 3)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', EXACT_CASES)
def test_known_answers_bit_for_bit(case, mode, hip_lib, cuda):
    from deephar_amd import functional as F
    n, h, w, cin, cout, ks = case
    assert ks * ks * cin <= 576
    rng = np.random.default_rng(sum(case))
    xh, xl = _exact_operand(rng, (n, h, w, cin))
    wh, wl = _exact_operand(rng, (ks, ks, cin, cout))
    x, k = xh + xl, wh + wl
    t = lambda a: torch.from_numpy(a).double()
    for v, (vh, vl) in ((x, (xh, xl)), (k, (wh, wl))):              # the construction does what it says
        p = R.split_parts(torch.from_numpy(v), 3)
        assert torch.equal(p[0], torch.from_numpy(vh)) and torch.equal(p[1], torch.from_numpy(vl)) and not p[2].any()
    conv = lambda a, b: O.conv2d(a, b, (1, 1), 'same')
    e = {'bf16': conv(t(xh), t(wh)), 'exact': conv(t(x), t(k))}
    e['bf16x2'] = e['bf16'] + conv(t(xl), t(wh)) + conv(t(xh), t(wl))
    for name in ('bf16', 'bf16x2'):
        assert torch.equal(e[name], R.conv_ep(O.conv2d, t(x), t(k), (1, 1), 'same', R.PARTS[name])), name
        assert torch.equal(e[name].float().double(), e[name])      # representable: the fp32 result can be the fp64 one
    xd = torch.from_numpy(x).to(cuda)
    outs = _tilings(hip_lib, lambda cfg: F.conv2d(xd, k, precision=mode, tile_cfg=cfg))
    assert -1 in outs and len(outs) >= 9, sorted(outs)
    for cfg, y in outs.items():
        y = y.cpu().double()
        bad = int((y != e[mode]).sum())
        assert bad == 0, '%s tiling %d: %d of %d outputs differ from E_P, worst %.3e' % (
            mode, cfg, bad, y.numel(), float((y - e[mode]).abs().max()))
    y = outs[-1].cpu().double()
    for other in e:
        if other != mode:
            frac = float((y != e[other]).double().mean())
            assert frac > 0.9, 'E(%s) equals E(%s) on %.1f %% of the outputs: the case cannot tell them apart' % (
                mode, other, 100 - 100 * frac)


# ---- 2. random operands, full epilogues --------------------------------------------------------------------------------
# (N, H, W, Cin, Cout, k, stride, relu, residual, up2) + flags: '2' second full-resolution residual, 'd' half-resolution
# second residual (res2_down), 'p' pooled second output
EPILOGUE_CASES = [(c, '') for c in SPLIT_CASES] + [
    ((2, 32, 32, 48, 576, 1, 1, True, True, False), '2'),
    ((2, 32, 32, 576, 288, 1, 1, True, True, False), 'd'),
    ((2, 16, 16, 288, 288, 1, 1, False, False, False), 'd'),
    ((3, 32, 32, 96, 200, 1, 1, True, True, False), 'p'),
    ((2, 64, 64, 64, 96, 3, 2, False, True, False), 'p2'),
]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case,flags', EPILOGUE_CASES)
def test_random_operands_full_epilogues(case, flags, mode, hip_lib, cuda):
    """Against E_P + epilogue in fp64, with the tolerance tests/test_gpu_ops.py::test_conv2d_split_bf16 applies to bf16x3
    against fp64 (twice the fp32-MFMA path's own error + 1e-6): with the mode's rounding inside the reference, what remains
    is the same fp32 accumulation.  Every tiling gives the same bits."""
    from deephar_amd import functional as F
    n, h, w, cin, cout, ks, st, relu, res, up2 = case
    rng = np.random.default_rng(sum(int(v) for v in case) + len(flags))
    x = _rand(rng, (n, h, w, cin))
    k = _rand(rng, (ks, ks, cin, cout), np.sqrt(1.0 / (ks * ks * cin)))
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = _rand(rng, (cout,), 0.1)
    oh, ow = -(-h // st), -(-w // st)
    r1 = _rand(rng, (n, oh, ow, cout)) if res else None
    r2 = None
    if up2:
        r2 = _rand(rng, (n, 2 * oh, 2 * ow, cout))
    elif '2' in flags:
        r2 = _rand(rng, (n, oh, ow, cout))
    elif 'd' in flags:
        r2 = _rand(rng, (n, oh // 2, ow // 2, cout))
    t = lambda a: torch.from_numpy(a).double()
    xin = O.relu(t(x)) if relu else t(x)

    def epilogue(y):
        y = y * t(sc) + t(sh)
        if res:
            y = y + t(r1)
        if up2:
            y = O.upsample2d(y) + t(r2)
        elif 'd' in flags:
            y = y + O.upsample2d(t(r2))
        elif '2' in flags:
            y = y + t(r2)
        return y
    truth = epilogue(O.conv2d(xin, t(k), (st, st), 'same'))
    ref = epilogue(R.conv_ep(O.conv2d, xin, t(k), (st, st), 'same', R.PARTS[mode]))
    d = lambda a: None if a is None else torch.from_numpy(a).to(cuda)
    kw = dict(strides=(st, st), padding='same', pre_relu=relu, post_scale=d(sc), post_shift=d(sh), res1=d(r1), res2=d(r2),
              up2=up2, res2_down='d' in flags)
    pool = 'p' in flags
    f32 = F.conv2d(d(x), k, **kw)
    e_f32 = (f32.cpu().double() - truth).abs().max().item()
    outs = _tilings(hip_lib, lambda cfg: F.conv2d(d(x), k, precision=mode, tile_cfg=cfg, pool2=pool, **kw))
    assert len(outs) >= 3, sorted(outs)
    if pool:
        for cfg, (y, yp) in outs.items():
            assert torch.equal(yp, F.pool2d(y, (2, 2))), (mode, cfg)
        outs = {cfg: y for cfg, (y, yp) in outs.items()}
        plain = F.conv2d(d(x), k, precision=mode, **kw)
        assert all(torch.equal(y, plain) for y in outs.values())
    first = next(iter(outs.values()))
    for cfg, y in outs.items():
        assert torch.equal(y, first), '%s tiling %d differs' % (mode, cfg)
    e_mode = (first.cpu().double() - ref).abs().max().item()
    e_true = (first.cpu().double() - truth).abs().max().item()
    print('case %s%s %s: |hip - E_P| = %.3e   |fp32 mfma - fp64| = %.3e   |hip - fp64| = %.3e   tilings %s' % (
        case, flags, mode, e_mode, e_f32, e_true, sorted(outs)))
    assert e_mode <= 2.0 * e_f32 + 1e-6, (e_mode, e_f32)
    # the mode is engaged: the result is E_P, not the exact product -- it sits nearer to E_P (what separates them is fp32
    # accumulation, ~2^-24 per addition) than to the fp64 truth (the dropped products, ~2^-17 / ~2^-9 per product for
    # P = 2 / 1), and it is not the fp32 path's answer
    assert e_mode < e_true, (e_mode, e_true)
    assert not torch.equal(first, f32)


def test_split_family_refusals_hold_for_the_new_modes(hip_lib, cuda):
    """What the split family cannot run is refused with the new codes as with w_split = 1 -- never run on another kernel."""
    from deephar_amd import functional as F
    from deephar_amd._lib import DeepharHipError
    for mode in MODES:
        with pytest.raises(DeepharHipError):                             # Cin = 3: general implicit-GEMM kernel only
            F.conv2d(torch.randn(1, 16, 16, 3, device=cuda), np.zeros((3, 3, 3, 32), np.float32), precision=mode)
        with pytest.raises(DeepharHipError):                             # a skinny layer (8 x 8 map, 128 channels)
            F.conv2d(torch.randn(2, 8, 8, 288, device=cuda), np.zeros((1, 1, 288, 128), np.float32), precision=mode)
        with pytest.raises(DeepharHipError):                             # BN prologue
            F.conv2d(torch.randn(2, 32, 32, 64, device=cuda), np.zeros((1, 1, 64, 64), np.float32), precision=mode,
                     pre_scale=torch.ones(64, device=cuda), pre_shift=torch.zeros(64, device=cuda))
        with pytest.raises(ValueError):
            F.conv2d(torch.randn(1, 64, 64, 16, device=cuda), np.zeros((3, 3, 16, 32), np.float32), precision=mode, halo=True)
    with pytest.raises(ValueError):
        F.conv2d(torch.randn(2, 32, 32, 64, device=cuda), np.zeros((1, 1, 64, 64), np.float32), precision='bf16x4')
    x, k = torch.randn(2, 32, 32, 64, device=cuda), np.random.default_rng(0).standard_normal((1, 1, 64, 64)).astype(np.float32)
    assert torch.equal(F.conv2d(x, k, split=True), F.conv2d(x, k, precision='bf16x3'))
    assert torch.equal(F.conv2d(x, k), F.conv2d(x, k, precision='f32'))


# ---- 3. invariance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_batch_invariance_is_bit_exact(mode, hip_lib, cuda):
    """The mirror of test_gpu_bf16x3.test_bf16x3_batch_invariance_is_bit_exact: K ascends identically in every tiling, so
    the result depends on nothing but the layer's geometry."""
    from test_gpu_models import _build
    m, _ = _build(2, 4, 16, num_context_per_joint=2)
    m.gemm_precision = mode
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (32, 256, 256, 3)).astype(np.float32)
    a = m.predict(x, batch_size=32)
    perm = rng.permutation(32)
    b = m.predict(x[perm], batch_size=32)
    c = m.predict(x, batch_size=8)
    d = m.predict(x, batch_size=32)
    for k in range(len(a)):
        assert np.array_equal(a[k][perm], b[k]) and np.array_equal(a[k], c[k]) and np.array_equal(a[k], d[k])


# ---- 4. models against the fp64 oracle, bar from the CPU emulation of the mode -----------------------------------------
def _split_count(m):
    return sum(1 for s in m.plan.steps if s.kind == 'conv' and s.attrs.get('w_split')), \
        sum(1 for s in m.plan.steps if s.kind == 'conv')


@pytest.fixture(scope='module', autouse=True)
def _write_model_records():
    yield
    path = os.environ.get('DEEPHAR_PARITY_BF16_MODES')
    if MODEL_RECORDS and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            json.dump(dict(unit='px of the 256-px crop', bar='max(1e-3, 2 * emu_px)',
                           emu='fp64 oracle with every split-eligible convolution evaluated as E_P (tests/bf16_modes_ref.py)',
                           labels='arg-max action labels that differ from the fp64 oracle: reported, not asserted',
                           records=MODEL_RECORDS), fh, indent=1)


@pytest.mark.parametrize('name', ['mpii', 'h36m', 'penn', 'ntu'])
def test_models_within_the_emulated_bar(name, hip_lib, cuda, monkeypatch):
    """MPII 8 blocks, H36M 8 blocks, PennAction merge T = 16, SPNet-NTU T = 8 (builders, seeds and inputs of
    tests/test_gpu_bf16x3.py).  Per mode: emu_px = worst distance of the CPU emulation of the mode from the fp64 oracle; the
    engine must stay within max(1e-3 px, 2 x emu_px) of the fp64 oracle (engine and emulation are two draws of one error
    process -- the engine rounds a subset of the layers, in another summation order -- and adjacent rungs are ~2^8 apart, so
    the factor cannot hide a dropped part).  The mode must be engaged and differ from the fp32 path."""
    m, x, n, oracle, poses, actions = R.model_case(name)
    o64 = oracle(torch.float64)
    o32 = oracle(torch.float32)
    m.gemm_precision = 'f32'
    f32 = m.predict(x, batch_size=n)
    failures = []
    for mode in MODES:
        with monkeypatch.context() as mp:
            R.emulate(mp, R.PARTS[mode])
            emu = oracle(torch.float64)
        emu_px = R.px(poses(emu), poses(o64))
        m.gemm_precision = mode
        hip = m.predict(x, batch_size=n)
        nsplit, nconv = _split_count(m)
        hip_px, h32_px, vs_f32 = R.px(poses(hip), poses(o64)), R.px(poses(hip), poses(o32)), R.px(poses(hip), poses(f32))
        labels = sum(int((a.argmax(-1) != b.argmax(-1)).sum()) for a, b in zip(actions(hip), actions(o64)))
        nlab = sum(int(np.prod(a.shape[:-1])) for a in actions(o64))
        bar = max(1e-3, 2.0 * emu_px)
        rec = dict(case=name, mode=mode, emu_px=emu_px, bar_px=bar, hip_vs_o64_px=hip_px, hip_vs_o32_px=h32_px,
                   hip_vs_f32_path_px=vs_f32, o32_vs_o64_px=R.px(poses(o32), poses(o64)), labels_differ=labels,
                   labels=nlab, split_convs=nsplit, convs=nconv, within_bar=bool(hip_px <= bar))
        MODEL_RECORDS.append(rec)
        cat = lambda outs: np.concatenate([np.asarray(v, np.float64).ravel() for v in poses(outs)])
        paritylog.record('%s.%s.pose' % (name, mode), cat(hip), cat(o32), cat(o64), case='bf16_modes', mode=mode,
                         emu_px=emu_px, bar_px=bar, labels_differ=labels)
        print(json.dumps(rec))
        assert all(np.all(np.isfinite(v)) for v in hip)
        assert nsplit >= (100 if name == 'mpii' else 20), (nsplit, nconv)
        assert vs_f32 > 0, 'the %s plan returned the fp32 path\'s bits' % mode
        if hip_px > bar:
            failures.append('%s %s: %.3e px from the fp64 oracle, bar %.3e px (emulation %.3e px)' % (name, mode, hip_px, bar, emu_px))
    assert not failures, failures


# ---- 5. exported plan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind', ['reception2d', 'spnet'])
def test_c_plan_reproduces_predict_in_the_new_modes(kind, mode, hip_lib, cuda, tmp_path):
    """export_plan serialises bound calls and the weight image: the C executor runs the new modes without a format change."""
    from test_gpu_models import _build, _spnet
    rng = np.random.default_rng(17)
    if kind == 'spnet':
        m, _, _, _ = _spnet(8, 'pa16j2d', 15, 2, [1, 2], 160, replica=True, res=128)
        x = rng.uniform(-1, 1, (3, 8, 128, 128, 3)).astype(np.float32)
    else:
        m, _ = _build(2, 2, 16, num_context_per_joint=2, concat_pose_confidence=False)
        x = rng.uniform(-1, 1, (5, 256, 256, 3)).astype(np.float32)
    m.gemm_precision = mode
    n = len(x)
    ref = m.predict(x, batch_size=n)
    ref = ref if isinstance(ref, list) else [ref]
    code = {'bf16x2': 3, 'bf16': 4}[mode]
    assert sum(1 for s in m.plan.steps if s.kind == 'conv' and s.attrs.get('w_split') == code) >= 10
    path = str(tmp_path / 'model.dhplan')
    nbytes = m.export_plan(path, n)
    blob = open(path, 'rb').read()
    assert len(blob) == nbytes and blob[:4] == b'DHPL'
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
        outs_h = (C.c_void_p * len(host))(*[h.ctypes.data for h in host])
        assert hip_lib.dh_forward_host(plan, ins_h, n, outs_h) == 0
        for h, r in zip(host, ref):
            assert np.array_equal(h, r)
    finally:
        assert hip_lib.dh_plan_destroy(plan) == 0
