"""The geometry sweep of tests/convsweep.py on the GPU: dh_conv2d_f32 with rectangular kernels, SH != SW and explicit padding
in every kernel family, fused with the prologues, residuals, layouts and forced tilings that had only ever met square TF-SAME
kernels; dh_pool2d_f32, dh_dwconv2d_f32 and dh_dwconv2d_strided_f32 on the same windows.

Every launch the route accepts: canaries around y, then per element |y - fp64| <= ((K + 8) 2^-24 + split term) B (derived in
convsweep's docstring; operands with channel magnitudes spread over 2^+-3 / 2^+-6, so that a small channel counts), then the
family's existing max-norm bar (fp32 and halo: e_hip <= 4 e_cpu + 1e-6; bf16x3: e_split <= 2 e_f32 + 1e-6), and all fp32
launches of a case -- tile_cfg = -1, a forced general tiling, a forced LDS-DMA tiling, whatever is named on a skinny layer --
carry the same bits.  Every launch the route refuses answers the code the route gave and has written nothing.
tests/test_conv_sweep_host.py shows without a GPU what the table covers and that the bar separates a geometry mix-up from
the reference's own rounding.

With DEEPHAR_SWEEP_LOG=<file> every launch appends one JSON line (profiles/conv_sweep.md is made from such a run)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convsweep as S                               # noqa: E402
import convview as CV                               # noqa: E402
import slabview as SV                               # noqa: E402

pytestmark = pytest.mark.gpu

MODE = {0: 'fp32', 2: 'fp32 halo', 1: 'bf16x3', 3: 'bf16x2', 4: 'bf16', 5: 'bf16x3 ext', 6: 'bf16x2 ext', 7: 'bf16 ext'}


def _log(rows):
    path = os.environ.get('DEEPHAR_SWEEP_LOG')
    if path:
        with open(path, 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(a, b, what):
    assert SV.same_bits(a, b), '%s: differs in bits (max |d| = %.3e)' % (what, float(np.nanmax(np.abs(a - b))))


def _one(lib, case, rows):
    d = S.data(case)
    ref, B, cpu = S.truth(case)
    S.assert_signs(case, d, ref)
    e_cpu = float(np.abs(cpu - ref).max())
    packs, fp32, bits, e_f32 = {}, None, {}, None
    for ws, cfg in case.launches():
        what = '%s w_split %d tile_cfg %d' % (case.name, ws, cfg)
        if ws not in packs:
            packs[ws] = S.pack(case, d['w'], ws)
        rc, r, y = S.launch(lib, case, packs[ws], ws, cfg, what)
        row = dict(case=case.name, stratum=case.stratum, mode=MODE[ws], cfg=cfg, rc=rc)
        rows.append(row)
        if (ws, cfg) == (0, -1):                    # the default launch is refused for a listed reason or not at all
            why = S.refusal(lib, case)
            assert (rc != 0) == (why is not None), (what, rc, why)
            row['why'] = why
        if rc != 0:                                 # (S.launch: the code the route gave, nothing written)
            assert rc == CV.DH_EUNSUPPORTED, (what, rc)
            continue
        parts = S.PARTS_OF.get(ws, 0)
        err = np.abs(y.astype(np.float64) - ref)
        ratio, at = S.worst(err, S.bound(case, B, parts))
        e = float(err.max())
        row.update(family=CV.FAMILY_OF_KERNEL[r.kernel], tiling=r.tile_cfg, ratio=ratio, at=[int(i) for i in at], e=e, e_cpu=e_cpu)
        print('%s (%s, %s): err / bound %.3f at %s   |hip - fp64| = %.3e   |fp32 cpu - fp64| = %.3e' % (
            what, MODE[ws], row['family'], ratio, at, e, e_cpu))
        assert ratio <= 1.0, '%s: |y - fp64| = %.3e at %s is %.3f of the bar' % (what, float(err[at]), at, ratio)
        if ws in (0, 2):
            row['old'] = e / (4 * e_cpu + 1e-6)
            assert e <= 4 * e_cpu + 1e-6, (what, e, e_cpu)
        if ws == 0:
            if fp32 is None:
                fp32, e_f32 = (y, what), e
            else:
                _same(y, fp32[0], '%s against %s' % (what, fp32[1]))
        elif parts == 3:                            # bf16x3, both scopes: twice the shipped fp32 kernel's own error
            assert e_f32 is not None, what
            row['old'] = e / (2 * e_f32 + 1e-6)
            assert e <= 2 * e_f32 + 1e-6, (what, e, e_f32)
        if ws:                                      # one answer per mode whatever the tiling; 5 / 6 / 7 == 1 / 3 / 4 on the standard scope
            first = bits.setdefault(parts, (y, what))
            _same(y, first[0], '%s against %s' % (what, first[1]))


@pytest.mark.parametrize('stratum,first,last', [c for s, _ in S.STRATA for c in S.chunks(s)])
def test_conv2d_geometry_sweep(stratum, first, last, hip_lib, cuda):
    t0, rows = time.time(), []
    table = S.cases(hip_lib)
    try:
        for i in range(first, last):
            _one(hip_lib, table['%s_%02d' % (stratum, i)], rows)
    finally:
        _log(rows + [dict(test='conv %s %d-%d' % (stratum, first, last), seconds=time.time() - t0, launches=len(rows))])
    ran = sum(r['rc'] == 0 for r in rows)
    print('%s %d..%d: %d launches ran, %d refused' % (stratum, first, last - 1, ran, len(rows) - ran))
    assert ran >= 2 * (last - first)


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', S.pool_cases(), ids=repr)
def test_pool2d_windows(g, hip_lib, cuda):
    """Max and max + min pooling over rectangular windows, SH != SW, explicit PT / PL, on dense, aligned and odd views: the
    pixels of a window that lie inside the frame, bit for bit (NumPy)."""
    from deephar_amd import _lib
    t0 = time.time()
    x = S._gauss(np.random.default_rng(len(g.name) + g.H * g.W), (g.N, g.H, g.W, g.C)) * S.channel_scales(np.random.default_rng(g.C), g.C, 6)
    ref = S.pool_ref(x, g)
    for name in SV.LAYOUTS:
        (ldx, ox), (ldy, oy) = SV.layout(g.C, name, 0), SV.layout(g.C, name, 1)
        tx, px = SV.slab(x, ldx, ox, np.nan)
        ty, py = SV.out_slab(ref.shape, ldy, oy)
        a = _lib.PoolArgs()
        a.x, a.y = px, py
        a.N, a.H, a.W, a.C, a.ldx, a.OH, a.OW, a.ldy = g.N, g.H, g.W, g.C, ldx, g.OH, g.OW, ldy
        a.KH, a.KW, a.SH, a.SW, a.PT, a.PL, a.mode = g.KH, g.KW, g.SH, g.SW, g.PT, g.PL, g.mode
        assert hip_lib.dh_pool2d_f32(C.byref(a), _stream()) == 0
        torch.cuda.synchronize()
        SV.assert_untouched(ty, oy, g.C, what='%s %s' % (g, name))
        assert SV.same_bits(SV.view(ty, oy, g.C), ref), (g, name)
    _log([dict(test='pool %s' % g, seconds=time.time() - t0, launches=3)])


# ---- depthwise convolutions ------------------------------------------------------------------------------------------------------
def _dw_launch(lib, g, d, chans, layname, x=None, up_in=None, strided=False):
    """One depthwise launch on the first `chans` channels, on views of layout `layname` -> (y, took the LDS kernel)."""
    from deephar_amd import _lib
    x = d['x'] if x is None else x
    up_in = g.up_in if up_in is None else up_in
    (ldx, ox), (ldy, oy) = SV.layout(chans, layname, 0), SV.layout(chans, layname, 1)
    tx, px = SV.slab(x[..., :chans], ldx, ox, np.nan)
    ty, py = SV.out_slab((g.N, g.OH, g.OW, chans), ldy, oy)
    wt = torch.from_numpy(np.ascontiguousarray(d['w'][..., :chans].reshape(g.KH * g.KW, chans))).cuda()
    keep = [CV.table(d[n][:chans], False) for n in ('pre_scale', 'pre_shift')] if g.pre == 'bnrelu' else []
    a = _lib.DwsArgs() if strided else _lib.DwArgs()
    a.x, a.w, a.y = px, wt.data_ptr(), py
    if keep:
        a.pre_scale, a.pre_shift = keep[0][1], keep[1][1]
    a.N, a.H, a.W, a.C, a.ldx, a.ldy, a.KH, a.KW, a.PT, a.PL = g.N, g.H, g.W, chans, ldx, ldy, g.KH, g.KW, g.PT, g.PL
    a.pre_relu = int(g.pre != 'none')
    lds = False
    if strided:
        a.OH, a.OW, a.SH, a.SW = g.OH, g.OW, g.SH, g.SW
        rc = lib.dh_dwconv2d_strided_f32(C.byref(a), _stream())
    else:
        a.up_in = int(up_in)
        lds = bool(lib.dh_dwconv2d_uses_lds_kernel(C.byref(a)))
        rc = lib.dh_dwconv2d_f32(C.byref(a), _stream())
    torch.cuda.synchronize()
    assert rc == 0, (g, layname, rc)
    SV.assert_untouched(ty, oy, chans, what='%s %s' % (g, layname))
    return SV.view(ty, oy, chans), lds


def _dw_check(g, y, ref, B, what, rows):
    err = np.abs(y.astype(np.float64) - ref[..., :y.shape[-1]])
    ratio, at = S.worst(err, S.dw_bound(g, B[..., :y.shape[-1]]))
    print('%s: err / bound %.3f at %s' % (what, ratio, at))
    rows.append(dict(case=g.name, stratum='dw', mode=what.split()[-1], rc=0, ratio=ratio, at=[int(i) for i in at], family='depthwise'))
    assert ratio <= 1.0, '%s: |y - fp64| = %.3e at %s is %.3f of the bar' % (what, float(err[at]), at, ratio)


@pytest.mark.parametrize('k,width', [(k, w) for k in (1, 3, 5) for w in S.DW_WIDTHS])
def test_dwconv2d_windows(k, width, hip_lib, cuda):
    """dh_dwconv2d_f32 at the widths of the LDS kernel's column tilings and heights around its band, explicit PT / PL, the three
    prologues: the same geometry through the LDS-tiled, the strip and the generic kernel, each per element inside
    (k k + 4) 2^-24 B of the fp64 statement; the up-sampled form equals the explicit one in bits."""
    t0, rows = time.time(), []
    cases = [g for g in S.dw_cases() if (g.KH, g.W) == (k, width)]
    assert len(cases) == (3 if k == 1 else 5)
    try:
        for g in cases:
            d = S.dw_data(g)
            ref, B = S.dw_statement(g, d, torch.float64), S.dw_statement(g, d, torch.float64, mag=True)
            xup = np.repeat(np.repeat(d['x'], 2, axis=1), 2, axis=2) if g.up_in else None
            for kernel, less, layname in S.DW_VARIANTS:
                y, lds = _dw_launch(hip_lib, g, d, g.C - less, layname)
                assert lds == (kernel == 'lds' and k > 1), (g, kernel, lds)
                _dw_check(g, y, ref, B, '%s %s' % (g, kernel), rows)
                if g.up_in:
                    y2, lds2 = _dw_launch(hip_lib, g, d, g.C - less, layname, x=xup, up_in=False)
                    assert lds2 == lds and SV.same_bits(y, y2), '%s %s: up_in differs from the explicit up-sampling' % (g, kernel)
    finally:
        _log(rows + [dict(test='dw k%d W%d' % (k, width), seconds=time.time() - t0, launches=len(rows))])


def test_dwconv2d_strided_windows(hip_lib, cuda):
    """dh_dwconv2d_strided_f32 on odd H and W with explicit PT / PL: the float4 and the generic kernel."""
    t0, rows = time.time(), []
    try:
        for g in S.dws_cases():
            d = S.dw_data(g)
            ref, B = S.dw_statement(g, d, torch.float64), S.dw_statement(g, d, torch.float64, mag=True)
            for layname in ('aligned', 'odd'):
                y, _ = _dw_launch(hip_lib, g, d, g.C, layname, strided=True)
                _dw_check(g, y, ref, B, '%s %s' % (g, layname), rows)
    finally:
        _log(rows + [dict(test='dw strided', seconds=time.time() - t0, launches=len(rows))])
