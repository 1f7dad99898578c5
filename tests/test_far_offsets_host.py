"""Host tests (no GPU) of the addressing limits: the rules that pick a 32-bit or a 64-bit kernel form, swept over their
thresholds on fake pointers, and the PROPERTY the rules are there for -- every launch a rule accepts forms offsets that
fit the type its kernel holds them in (the audit table of tests/farview.py, evaluated by farview.largest_offsets).

For each threshold: the last pitch (a multiple of 4 floats) the condition holds for, one step below, one and two steps
above, at two pixel counts.  Asserted: (a) the library's answer flips exactly where the constants say, (b) whatever it
accepts fits, (c) what it refuses it refuses with the documented code, and a pitch a 32-bit form cannot take never
reaches one.  tests/test_gpu_far_offsets.py runs the same launches on real memory."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convview as CV                              # noqa: E402
import farview as FV                               # noqa: E402

ALIGNED = {o: 'aligned' for o in CV.OPERANDS}


def _args(case, x='aligned', **ld):
    a = CV.fake_args(case, dict(ALIGNED, x=x), False)
    for k, v in ld.items():
        setattr(a, k, v)
    return a


def _fits(a, r, what):
    for name, value, bound, inclusive in FV.largest_offsets(a, r):
        assert (value <= bound) if inclusive else (value < bound), (what, name, hex(value), hex(bound))


def _two_batches(name, **kw):
    return [FV.with_batch(FV.CASES[name], n, **kw) for n in (2, 3)]


# ---- epi_with_direct: M * ld * 4 < 0x7fffffff for y and res1, (M / 4) * ldr2 * 4 < 0x7fffffff ------------------------------
def test_direct_epilogue_threshold(hip_lib):
    seen = set()
    for name, ops in (('direct', ('ldy', 'ldr1')), ('direct_down', ('ldy', 'ldr1', 'ldr2')), ('halo', ('ldy', 'ldr1'))):
        for case in _two_batches(name):
            cfg = case.cfgs[0]
            for field in ops:
                pixels = case.M // 4 if field == 'ldr2' else case.M
                for ld, holds in FV.steps_around(FV.INT31, 4 * pixels, False):
                    a = _args(case, **{field: ld})
                    r = CV.route(hip_lib, a, cfg)
                    what = (name, case.N, field, ld)
                    assert r.rc == 0 and CV.FAMILY_OF_KERNEL[r.kernel] == case.family_of(cfg) and r.tm == 1, what
                    assert bool(r.epi & 2) == holds, what                                   # (a)
                    _fits(a, r, what)                                                       # (b)
                    p = CV.paths(hip_lib, case, a, cfg)
                    assert ('direct' in p) == holds, (what, p)                              # (c): the staged form is 64-bit
                    if case.res2:
                        assert ('down_direct' in p) == holds and (holds or 'down_staged_pow2' in p), (what, p)
                    seen.add((name, field, holds))
    assert len(seen) == 2 * 7
    # the pitches around the bound at M = 2048 ("Addressing limits")
    assert [ld for ld, ok in FV.steps_around(FV.INT31, 4 * 2048, False)] == [262136, 262140, 262144, 262148]


# ---- x through a buffer descriptor: P * ldx * 4 <= 0xf0000000 --------------------------------------------------------------
X_FAMILIES = [('pw_ktail', None, 2), ('pw_bn', None, 2), ('kxk', None, 2), ('split1', None, 3), ('split1', 3, 3), ('split1', 4, 3),
              ('ext_pw', 5, 4), ('ext_pw', 6, 4), ('ext_pw', 7, 4), ('ext_kxk', 5, 4), ('ext_kxk', 6, 4), ('ext_kxk', 7, 4),
              ('halo', None, 5)]


def test_buffer_descriptor_threshold(hip_lib):
    assert [ld for ld, ok in FV.steps_around(FV.MAX_BUFFER_BYTES, 4 * 2048, True)] == [491516, 491520, 491524, 491528]
    for name, ws, kernel in X_FAMILIES:
        for case in _two_batches(name, w_split=ws):
            cfg = case.cfgs[0]
            P = case.N * case.H * case.W
            for ld, holds in FV.steps_around(FV.MAX_BUFFER_BYTES, 4 * P, True):
                a = _args(case, ldx=ld)
                r = CV.route(hip_lib, a, cfg)
                what = (name, ws, case.N, ld)
                if holds:
                    assert r.rc == 0 and r.kernel == kernel, (what, r.rc, r.kernel)         # (a)
                    _fits(a, r, what)                                                       # (b)
                else:
                    assert r.rc == CV.DH_EUNSUPPORTED and r.kernel == 0, (what, r.rc)       # (c)
                if case.w_split in (1, 3, 4):
                    assert hip_lib.dh_conv2d_split_eligible(C.byref(a)) == int(holds), what
                if case.w_split >= 5:
                    assert hip_lib.dh_conv2d_split_wide_eligible(C.byref(a)) == int(holds), what
                if case.w_split == 2:
                    assert hip_lib.dh_conv2d_halo_eligible(C.byref(a)) == int(holds), what
                if case.w_split == 0:               # the library's own pick: the DMA GEMM, or the register-gather kernel (64-bit)
                    r = CV.route(hip_lib, a, -1)
                    assert r.rc == 0 and r.kernel == (FV.CV_KERNEL['dma'] if holds else FV.CV_KERNEL['general']), (what, r.kernel)
                    _fits(a, r, what)
                    assert not (r.kernel in FV.THIRTYTWO_BIT and not holds)


# ---- first-layer kernel: N * OH * OW * ldy * 4 < 0x7fffffff (depends on N) -------------------------------------------------
def test_first_layer_threshold(hip_lib):
    assert [ld for ld, ok in FV.steps_around(FV.INT31, 4 * 512, False)] == [1048568, 1048572, 1048576, 1048580]
    for name in ('stem', 'stem_u8'):
        for case in _two_batches(name):
            for ld, holds in FV.steps_around(FV.INT31, 4 * case.M, False):
                a = _args(case, x='dense', ldy=ld)
                for cfg in (-1, 3):
                    r = CV.route(hip_lib, a, cfg)
                    what = (name, case.N, ld, cfg)
                    # above: the tap-major register-gather kernel (x is dense with 3 channels: no DMA form), 64-bit throughout
                    want = FV.CV_KERNEL['stem'] if holds else FV.CV_KERNEL['general']
                    assert r.rc == 0 and r.kernel == want, (what, r.rc, r.kernel)           # (a), (c)
                    assert hip_lib.dh_conv2d_uses_first_layer_kernel(C.byref(a)) == int(holds), what
                    _fits(a, r, what)                                                       # (b)


# ---- skinny kernel: H * W * ldx (4 x with x_resample >= 2) <= 0x7fffffff floats per frame ----------------------------------
def test_skinny_threshold(hip_lib):
    assert [ld for ld, ok in FV.steps_around(FV.INT31, 64, True)] == [33554424, 33554428, 33554432, 33554436]
    for name in ('skinny', 'skinny_rs2'):
        base = FV.CASES[name]
        for shape in ((1, 8, 8, 64), (3, 8, 16, 64)):          # a per-frame rule: N does not move it, the map does
            case = CV.Case(name, shape, 24, k=3, pre=base.pre, bn=True, res1=True, family='skinny', x_resample=base.x_resample)
            frame = case.H * case.W * (4 if case.x_resample >= 2 else 1)
            for ld, holds in FV.steps_around(FV.INT31, frame, True):
                a = _args(case, ldx=ld)
                assert hip_lib.dh_conv2d_uses_split_k(C.byref(a)) == 1              # the shape rule does not look at pitches
                for cfg in (-1, 3, 12):
                    r = CV.route(hip_lib, a, cfg)
                    what = (name, shape, ld, cfg)
                    if holds:
                        assert r.rc == 0 and r.kernel == FV.CV_KERNEL['skinny'] and r.vec4 == 1, (what, r.rc)   # (a)
                        _fits(a, r, what)                                                   # (b)
                    else:
                        assert r.rc == FV.DH_EINVAL and r.kernel == 0, (what, r.rc)         # (c): no other kernel takes it


# ---- depthwise, stride 1: H * W * ld * 4 < 0x7fffffff per frame, for x and for y -------------------------------------------
def _dw(h, w, c, k, ldx, ldy, n=2, pt=None, up_in=0):
    from deephar_amd import _lib
    g = _lib.DwArgs()
    g.x, g.w, g.y = 0x100000, 0x8000000, 0x200000
    g.N, g.H, g.W, g.C, g.ldx, g.ldy = n, h, w, c, ldx, ldy
    g.KH = g.KW = k
    g.PT = CV.same_pad(h, k, 1)[0] if pt is None else pt
    g.PL, g.up_in = CV.same_pad(w, k, 1)[0], up_in
    return g


def _dw_window_fits(g):
    """The LDS kernel's window rows above / behind the frame, as the 32-bit byte offsets it forms: inside [-2^31, 2^32)."""
    tw = 32 if g.W >= 32 else g.W
    rows = min((64 if tw == 8 else 256) // (8 * (tw // 8)), g.H)
    ush = 1 if g.up_in else 0
    row_bytes = (g.W >> ush) * g.ldx * 4
    last = -(-g.H // rows) * rows + g.KH - 2 - g.PT
    return ((last >> ush) + 1) * row_bytes <= 1 << 32 and ((g.PT + ush) >> ush) * row_bytes <= 1 << 31


def test_depthwise_lds_threshold(hip_lib):
    uses = lambda g: hip_lib.dh_dwconv2d_uses_lds_kernel(C.byref(g))
    assert uses(_dw(16, 16, 32, 5, 32, 32)) == 1 and uses(_dw(16, 16, 32, 5, 33, 32)) == 0 and uses(_dw(16, 16, 30, 5, 32, 32)) == 0
    assert hip_lib.dh_dwconv2d_uses_lds_kernel(None) == 0
    for h, w in ((16, 16), (32, 32)):
        for k in (5, 3):
            for ld, holds in FV.steps_around(FV.INT31, 4 * h * w, False):
                for gx in (_dw(h, w, 32, k, ld, 40), _dw(h, w, 32, k, 40, ld), _dw(h, w, 32, k, ld, ld, n=1)):
                    assert uses(gx) == int(holds), (h, w, k, ld)                            # (a); (c): 0 = the 64-bit register kernel
                    assert not holds or _dw_window_fits(gx), (h, w, k, ld)                  # (b)
    assert [ld for ld, ok in FV.steps_around(FV.INT31, 4 * 256, False)][1] == (1 << 21) - 4 and \
        [ld for ld, ok in FV.steps_around(FV.INT31, 4 * 1024, False)][1] == (1 << 19) - 4     # = (2^31 - 4 * H * W * 4) / (4 H W)


def test_depthwise_lds_window_rows_do_not_wrap(hip_lib):
    """What the audit found: on a ONE-row map the window's rows behind the frame lie up to 3 frames from its base; at a pitch
    near the frame bound the 32-bit offset wrapped past 2^32 into the frame.  Such a launch now takes the register kernel.
    Every map of two rows or more with 'same' padding keeps the LDS kernel up to the frame bound."""
    uses = lambda g: hip_lib.dh_dwconv2d_uses_lds_kernel(C.byref(g))
    for k in (5, 3):
        for w in (8, 16, 32):
            top = [ld for ld, ok in FV.steps_around(FV.INT31, 4 * w, False) if ok][-1]          # H = 1: the frame bound on the pitch
            seen = set()
            for ld in (64, top // 4 // 4 * 4, top // 2 // 4 * 4, top // 2 // 4 * 4 + 4, top):
                g = _dw(1, w, 32, k, ld, 32)
                assert uses(g) == int(_dw_window_fits(g)), (k, w, ld)
                seen.add(uses(g))
            assert seen == ({0, 1} if k == 5 else {1}), (k, w)      # (3 x 3: one row above, one behind -- 2 frames, no wrap)
            for h in (2, 3, 4, 7, 9, 15, 16, 17, 33):
                fit = [ld for ld, ok in FV.steps_around(FV.INT31, 4 * h * w, False) if ok][-1]
                g = _dw(h, w, 32, k, fit, 32)
                assert uses(g) == 1 and _dw_window_fits(g), (k, w, h)
    g = _dw(4, 8, 32, 5, (1 << 24) - 4, 32, pt=4)              # a caller's PT of KS - 1 rows above a short map
    assert uses(g) == int(_dw_window_fits(g))


# ---- transposed 2x2 convolution, split form: M * ldx * 4 <= 0xf0000000 --------------------------------------------------
def test_transposed_split_threshold(hip_lib):
    from deephar_amd import _lib
    n, h, w, cin = CV.CONVT_SHAPE
    for nn in (n, 2 * n):
        M = nn * h * w
        for ld, holds in FV.steps_around(FV.MAX_BUFFER_BYTES, 4 * M, True):
            a = _lib.ConvtArgs()
            a.x, a.y = 0x100000, 0x200000
            a.N, a.H, a.W, a.Cin, a.ldx, a.Cout, a.ldy, a.Kp, a.Np = nn, h, w, cin, ld, 20, 20, 32, 96
            assert hip_lib.dh_conv2d_transpose2x2_split_eligible(C.byref(a)) == int(holds), (nn, ld)
            if holds:
                assert ((M - 1) * ld + a.Kp) * 4 < FV.OOB and ((M - 1) * ld + cin) * 4 <= FV.MAX_BUFFER_BYTES
    assert [ld for ld, ok in FV.steps_around(FV.MAX_BUFFER_BYTES, 4 * 60, True)] == [16777212, 16777216, 16777220, 16777224]
    # (M <= 0x7fffffff / 4 cannot bite first: with Cin % 4 == 0 a pixel of x is 16 bytes, so the descriptor bound caps M at 0x0f000000)
