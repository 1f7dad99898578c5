"""The clip boundary without a device (deephar_amd/csrc/cut_index.h behind the C ABI): dh_unpack_cut_host against NumPy's
moveaxis + reshape + slice, and dh_clip_inspect on 'DHCL' containers assembled around stub plan blobs
(engine/serialize.pack_clip).  Floats are moved, never computed on: every comparison is exact.  tools/clip_sweep.cpp runs the
same sweeps as a stand-alone program for a sanitizer build."""
import ctypes as C
import itertools
import struct
import subprocess

import numpy as np
import pytest

from deephar_amd import _lib
from deephar_amd.engine import serialize

EINVAL = -1
GUARD = np.float32(-7.0)
HEADER = 72                                            # bytes in front of the cut table


def segment_sets(cp):
    """[(coff, c, ld)] lists: c in {1, 2, 3, 4, 5, 16} then the remainder, from an aligned and from unaligned offsets, at pitches
    ld == c and ld > c"""
    sets = []
    for start, padded, wide_first in itertools.product((0, 1, 4), (False, True), (False, True)):
        segs, off = [], start
        for w in ((4, 16, 1, 2, 3, 5) if wide_first else (1, 2, 3, 4, 5, 16)):
            if off + w > cp:
                break
            segs.append((off, w, w + (4 if w % 4 == 0 else 3) if padded else w))
            off += w
        if off < cp:
            segs.append((off, cp - off, cp - off + 4 if padded else cp - off))
        sets.append(segs)
    return sets


def reference(gathered, segs):
    """gathered [G, m, Tl, P, Cp] -> per segment the dense [m, T, P, c] tensor"""
    g, m, tl, p, cp = gathered.shape
    frames = np.moveaxis(gathered, 0, 1).reshape(m, g * tl, p, cp)
    return [frames[..., off:off + c] for off, c, _ in segs]


def seg_table(dsts, segs):
    tab = (_lib.CutSeg * len(segs))()
    for k, ((off, c, ld), d) in enumerate(zip(segs, dsts)):
        tab[k].dst, tab[k].ld, tab[k].coff, tab[k].c = d.ctypes.data, ld, off, c
    return tab


@pytest.mark.parametrize('cp', [7, 24, 581])
def test_unpack_cut_host_equals_numpy(cp, hip_lib):
    rng = np.random.default_rng(cp)
    for g, m, tl, p in itertools.product((1, 2, 3), (1, 2), (1, 3), (1, 5, 16)):
        gathered = rng.standard_normal((g, m, tl, p, cp)).astype(np.float32)
        for segs in segment_sets(cp):
            dsts = [np.full((m, g * tl, p, ld), GUARD, np.float32) for _, _, ld in segs]
            tab = seg_table(dsts, segs)
            assert hip_lib.dh_unpack_cut_host(gathered.ctypes.data, g, m, tl, p, cp, tab, len(segs)) == 0
            for (off, c, ld), d, want in zip(segs, dsts, reference(gathered, segs)):
                assert np.array_equal(d[..., :c], want), (g, m, tl, p, cp, off, c, ld)
                assert np.all(d[..., c:] == GUARD), ('guard columns', g, m, tl, p, cp, off, c, ld)


def test_unpack_cut_host_refuses_bad_requests(hip_lib):
    src = np.zeros(7, np.float32)
    d = np.full(4, GUARD, np.float32)
    for off, c, ld in [(7, 1, 1), (6, 2, 2), (-1, 1, 1), (0, 0, 1), (0, 2, 1)]:
        tab = seg_table([d], [(off, c, ld)])
        assert hip_lib.dh_unpack_cut_host(src.ctypes.data, 1, 1, 1, 1, 7, tab, 1) == EINVAL
    tab = seg_table([d], [(0, 1, 1)])
    for geom in [(0, 1, 1, 1, 7), (1, 0, 1, 1, 7), (1, 1, 0, 1, 7), (1, 1, 1, 0, 7), (1, 1, 1, 1, 0), (1 << 20, 1 << 20, 1 << 20, 1, 7)]:
        assert hip_lib.dh_unpack_cut_host(src.ctypes.data, *geom, tab, 1) == EINVAL
    assert hip_lib.dh_unpack_cut_host(None, 1, 1, 1, 1, 7, tab, 1) == EINVAL
    assert np.all(d == GUARD)


def test_vec4_predicate(hip_lib):
    """16 bytes per lane exactly when Cp, coff, c, ld are multiples of 4 and both addresses are 16-byte aligned."""
    ok = (24, 4, 16, 16, 0x1000, 0x2000)
    assert hip_lib.dh_unpack_cut_vec4(*ok) == 1
    for k, bad in enumerate((22, 5, 15, 18, 0x1004, 0x2008)):
        args = list(ok)
        args[k] = bad
        assert hip_lib.dh_unpack_cut_vec4(*args) == 0, k


# ---- the container ---------------------------------------------------------------------------------------------------------

def stub_plan(nbytes, seed):
    return b'DHPL' + bytes(np.random.default_rng(seed).integers(0, 256, nbytes - 4, dtype=np.uint8))


CASES = {
    # name: world, T, Tl, Cp, P, cut [(offset, channels)], outputs [(kind, index)], frames bytes, head bytes
    'merge': (2, 8, 4, 581, 16, [(0, 2), (2, 1), (3, 576), (579, 2)], [(0, 0), (0, 1), (1, 0), (1, 1)], 300, 200),
    'pose_only': (1, 4, 4, 24, 1, [(0, 3), (3, 1)], [(0, 0), (0, 1)], 44, 0),
    'shared_cut': (3, 3, 1, 7, 5, [(0, 7)], [(1, 0), (0, 0), (0, 0)], 257, 44),
    'many': (4, 16, 4, 200, 34, [(2 * i, 2) for i in range(100)], [(i % 2, i // 2 if i % 2 else i) for i in range(100)], 512, 256),
}


def container(name):
    world, t, tl, cp, p, cut, outs, fb, hb = CASES[name]
    return serialize.pack_clip(world, t, tl, cp, p, cut, outs, stub_plan(fb, 1), stub_plan(hb, 2) if hb else b'')


def inspect(lib, blob, nbytes=None):
    info = _lib.ClipInfo()
    return lib.dh_clip_inspect(blob, len(blob) if nbytes is None else nbytes, C.byref(info)), info


@pytest.mark.parametrize('name', sorted(CASES))
def test_clip_inspect_round_trips_every_field(name, hip_lib):
    world, t, tl, cp, p, cut, outs, fb, hb = CASES[name]
    blob = container(name)
    rc, info = inspect(hip_lib, blob)
    assert rc == 0
    assert (info.version, info.world, info.T, info.Tl, info.packed_channels, info.P) == (1, world, t, tl, cp, p)
    assert (info.num_cut, info.num_outputs, info.num_head_outputs) == (len(cut), len(outs), sum(k for k, _ in outs))
    assert (info.frames_bytes, info.head_bytes) == (fb, hb)
    assert info.frames_offset % 256 == 0 and info.head_offset % 256 == 0 and info.frames_offset >= HEADER + 8 * (len(cut) + len(outs))
    assert info.head_offset >= info.frames_offset + fb and info.head_offset + hb == len(blob)
    assert blob[info.frames_offset:info.frames_offset + fb] == stub_plan(fb, 1)
    assert blob[info.head_offset:] == (stub_plan(hb, 2) if hb else b'')
    a, b = C.c_int32(), C.c_int32()
    for i, (off, c) in enumerate(cut):
        assert hip_lib.dh_clip_inspect_cut(blob, len(blob), i, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (off, c)
    for k, (kind, idx) in enumerate(outs):
        assert hip_lib.dh_clip_inspect_output(blob, len(blob), k, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (kind, idx)
    assert hip_lib.dh_clip_inspect_cut(blob, len(blob), len(cut), C.byref(a), C.byref(b)) == EINVAL
    assert hip_lib.dh_clip_inspect_output(blob, len(blob), -1, C.byref(a), C.byref(b)) == EINVAL


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_truncation_is_refused(name, hip_lib):
    blob = container(name)
    for n in range(len(blob)):
        assert inspect(hip_lib, blob[:n])[0] == EINVAL, n          # a copy of exactly n bytes
    assert inspect(hip_lib, blob + b'\0')[0] == EINVAL
    assert hip_lib.dh_clip_inspect(None, 100, C.byref(_lib.ClipInfo())) == EINVAL
    assert hip_lib.dh_clip_inspect(blob, len(blob), None) == EINVAL
    h = C.c_void_p()
    cb = _lib.ALLGATHER_FN()                                        # NULL callback
    assert hip_lib.dh_clip_create(blob[:len(blob) - 1], len(blob) - 1, 0, cb, None, C.byref(h)) == EINVAL and not h.value


def corrupt(blob, at, value, fmt='<I'):
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_corrupted_entry_is_refused(name, hip_lib):
    world, t, tl, cp, p, cut, outs, fb, hb = CASES[name]
    blob = container(name)
    nhead = sum(k for k, _ in outs)
    bad = [(0, 0x4c434845), (4, 2), (8, 0), (8, t + 1), (12, 0), (16, tl + 1), (20, 0), (24, 0), (28, 1 << 31), (32, 0), (32, 2 ** 32 - 1),
           (36, 0), (36, 2 ** 32 - 1)]
    if t % (world + 1):
        bad.append((8, world + 1))                                  # a world that does not divide T
    for i, (off, c) in enumerate(cut):
        at = HEADER + 8 * i
        bad += [(at, cp - c + 1), (at, 2 ** 32 - 1), (at + 4, cp - off + 1), (at + 4, 0), (at + 4, 2 ** 32 - 1)]
    for k, (kind, idx) in enumerate(outs):
        at = HEADER + 8 * len(cut) + 8 * k
        bad += [(at, 2), (at + 4, nhead if kind else len(cut)), (at + 4, 2 ** 32 - 1)]
    _, info = inspect(hip_lib, blob)
    bad += [(info.frames_offset, 0)] + ([(info.head_offset, 0)] if hb else [])       # the plan blobs' magic
    for at, value in bad:
        assert inspect(hip_lib, corrupt(blob, at, value))[0] == EINVAL, (at, value)
    for at in (40, 48, 56, 64):                                     # the four extents
        cur = struct.unpack_from('<Q', blob, at)[0]
        for d in (-256, 256) if at == 48 else (-256, -1, 1, 256):   # (a frames blob that ends inside its padding is well formed)
            assert inspect(hip_lib, corrupt(blob, at, (cur + d) % 2 ** 64, '<Q'))[0] == EINVAL, (at, d)
        for v in (2 ** 64 - 1, 2 ** 63):
            assert inspect(hip_lib, corrupt(blob, at, v, '<Q'))[0] == EINVAL, (at, v)
    # a head plan without a head output, and the reverse
    if hb:
        only_pass = serialize.pack_clip(world, t, tl, cp, p, cut, [(0, 0)], stub_plan(fb, 1), stub_plan(hb, 2))
    else:
        only_pass = serialize.pack_clip(world, t, tl, cp, p, cut, [(1, 0)], stub_plan(fb, 1))
    assert inspect(hip_lib, only_pass)[0] == EINVAL


def test_library_does_not_link_a_collective_library(hip_lib):
    """dh_clip_* take the collective as a callback and nowhere else: libdeephar_hip.so needs what it needed before."""
    from deephar_amd import _lib
    out = subprocess.run(['readelf', '-d', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = sorted(l.split('[')[1].split(']')[0] for l in out.splitlines() if '(NEEDED)' in l)
    assert not any('rccl' in n or 'nccl' in n or 'mpi' in n for n in needed), needed
    assert needed == sorted(['libamdhip64.so.7', 'libstdc++.so.6', 'libm.so.6', 'libgcc_s.so.1', 'libc.so.6']), needed
