"""The 'DHPL' plan blob without a device: the reader's step-record table (csrc/plan_blob.h behind dh_plan_record) against the ctypes
signatures the writer packs from; blobs packed on the host (serialize.pack_plan over binding.FakeEnv) through dh_plan_inspect;
every truncation, every broken step record and every broken tagged pointer refused; and tools/plan_blob_sweep.cpp built and
run on such a blob.  Nothing is computed on: every comparison is exact."""
import ctypes as C
import functools
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_binding_host as B                       # noqa: E402
import test_plan_streams_host as PS                 # noqa: E402

from deephar_amd import _lib                        # noqa: E402
from deephar_amd.engine import serialize as S       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
F_COUNT = len(S.ALL_FUNCTIONS)
HEAD = 4 + struct.calcsize('<IiQQIIIQ')            # bytes in front of the input table (version >= 2)
BASE = B.BASE                                      # the fake arena's address
TABLE_BYTES = 256                                  # every fake table is this many bytes of region 2


def inspect(lib, blob):
    """dh_plan_inspect -> (rc, PlanInfo); the library gets a buffer of exactly len(blob) bytes"""
    info = _lib.PlanInfo()
    buf = (C.c_char * max(len(blob), 1)).from_buffer_copy(blob or b'\0')
    return lib.dh_plan_inspect(buf, len(blob), C.byref(info)), info


def make_tag(base, arena_bytes, tables):
    """the test tagger: the fake arena is region 1, fake table k (at k << 20, binding.FakeEnv) is bytes [256 (k - 1), 256 k) of
    region 2; anything else is an error"""
    index = {addr: k for k, addr in enumerate(sorted(tables))}

    def tag(ptr):
        ptr = int(ptr or 0)
        if ptr == 0:
            return 0
        if base <= ptr < base + arena_bytes:
            return (S.ARENA << 60) | (ptr - base)
        return (S.WEIGHTS << 60) | (TABLE_BYTES * index[ptr])
    return tag


def host_blob(plan, n, section=b''):
    """-> (blob, expected PlanInfo fields, function ids) of `plan` bound for n items under binding.FakeEnv"""
    bound, env = B.launches(plan, n)
    launches = [(name, structs, scalars) for _, name, structs, scalars in bound]
    arena_bytes = 4 * plan.arena_items * n
    tables = sorted(env.tables.values())
    inputs = [(env.ptr(v), int(np.prod(v.shape)), 0) for v in plan.inputs]
    outputs = [(env.ptr(v) - env.base, v.npix, v.C, v.ld) for v in plan.outputs]
    blob = S.pack_plan(n, arena_bytes, inputs, outputs, launches, make_tag(env.base, arena_bytes, tables),
                       bytes(TABLE_BYTES * len(tables)), section=section)
    ids = [S.ALL_FUNCTIONS.index(name) for name, _, _ in launches]
    want = dict(version=S.plan_version(ids, section), batch=n, num_inputs=len(inputs), num_outputs=len(outputs), num_steps=len(launches),
                arena_bytes=arena_bytes, weight_bytes=TABLE_BYTES * len(tables), byte_bytes=0)
    return blob, want, ids


def hand_launch(fn):
    """function id -> a launch of that entry point from its ctypes signature: every pointer the arena's first byte, every
    integer 1, every float 0.5 (the parser looks at sizes and pointers only)"""
    name = S.ALL_FUNCTIONS[fn]
    sig = _lib.SIGNATURES[name][1][:-1]
    structs = []
    for t in sig:
        if not S._is_struct_ptr(t):
            break
        st = t._type_()
        for f, ft in st._fields_:
            setattr(st, f, BASE if ft is C.c_void_p else (0.5 if ft is C.c_float else 1))
        structs.append(st)
    scalars = [BASE if t is C.c_void_p else (0.5 if t is C.c_float else 1) for t in sig[len(structs):]]
    return name, structs, scalars


def hand_blob(fns, section=b'', u8=False):
    """a blob of these launches, one float input and one output in a 4096-byte arena (u8: a uint8 input in region 3)"""
    u8_base, u8_bytes = BASE << 1, 512 if u8 else 0

    def tag(ptr):
        if u8 and u8_base <= ptr < u8_base + u8_bytes:
            return (S.BYTES << 60) | (ptr - u8_base)
        return make_tag(BASE, 4096, [])(ptr)
    inputs = [(u8_base, 48, 1)] if u8 else [(BASE, 16, 0)]
    return S.pack_plan(2, 4096, inputs, [(64, 4, 2, 3)], [hand_launch(f) for f in fns], tag, u8_bytes=u8_bytes, section=section)


def steps_of(blob):
    """[(offset of the step record, function id, payload bytes)] and the offset behind the last one (versions >= 2)"""
    nin, nout, nsteps = struct.unpack_from('<III', blob, 28)
    at, out = HEAD + 24 * nin + 24 * nout, []
    for _ in range(nsteps):
        fn, nb = struct.unpack_from('<II', blob, at)
        out.append((at, fn, nb))
        at += 8 + nb
    return out, at


def put(blob, at, fmt, *values):
    raw = bytearray(blob)
    struct.pack_into(fmt, raw, at, *values)
    return bytes(raw)


def as_version_1(blob):
    """the same plan in the version-1 layout: no u8 region size in the header, inputs as bare arena offsets without a dtype"""
    ver, n, arena, wbytes, nin, nout, nsteps, u8b = struct.unpack_from('<IiQQIIIQ', blob, 4)
    assert ver == 2 and u8b == 0
    ins = b''
    for i in range(nin):
        tag, items, dtype, _ = struct.unpack_from('<QQII', blob, HEAD + 24 * i)
        assert tag >> 60 == 1 and dtype == 0
        ins += struct.pack('<QQ', tag & ((1 << 60) - 1), items)
    return blob[:4] + struct.pack('<IiQQIII', 1, n, arena, wbytes, nin, nout, nsteps) + ins + blob[HEAD + 24 * nin:]


@functools.lru_cache(maxsize=None)
def model_blobs():
    """{(model, batch): (blob, expected fields, function ids)} of every model of tests/test_binding_host.py, batch 1 and 3"""
    out = {}
    for name, make in B.models():
        plan = make().plan
        for n in (1, 3):
            out[name, n] = host_blob(plan, n)
    return out


def reference_blob():
    """the blob the refusal tests break: the host-built one with the most different step records (a ReceptionNet's: some
    30 KB, 60 steps)"""
    return max(model_blobs().values(), key=lambda e: (len(set(e[2])), -len(e[0])))[0]


# ---- the writer and the reader agree ---------------------------------------------------------------------------------------------

def test_record_table_equals_the_ctypes_signatures(hip_lib):
    for fn, name in enumerate(S.ALL_FUNCTIONS):
        got_name, first, size, offsets = _lib.plan_record(hip_lib, fn)
        assert got_name == name
        assert first == {2: 1, 3: 3, 4: 4}[S.blob_version([fn])], name
        sig = _lib.SIGNATURES[name][1][:-1]                    # without the stream
        at, want = 0, []
        for t in sig:
            if S._is_struct_ptr(t):
                want += [at + getattr(t._type_, f).offset for f, ft in t._type_._fields_ if ft is C.c_void_p]
                at += C.sizeof(t._type_)
            else:
                if t is C.c_void_p:
                    want.append(at)
                at += 8
        assert size == at, (name, size, at)
        assert sorted(offsets) == sorted(want) and len(set(offsets)) == len(offsets), (name, offsets, want)
        assert all(o % 8 == 0 and o + 8 <= size for o in offsets), name
    for fn in (-1, F_COUNT, 1 << 20):
        assert _lib.plan_record(hip_lib, fn) is None
    # the count is answered without a table; a table of four gets the first four offsets
    n, name, first, size = C.c_int(), C.c_char_p(), C.c_int(), C.c_size_t()
    assert hip_lib.dh_plan_record(0, C.byref(name), C.byref(first), C.byref(size), None, 0, C.byref(n)) == 0 and n.value == 11
    four = (C.c_int32 * 5)(*([-1] * 5))
    assert hip_lib.dh_plan_record(0, C.byref(name), C.byref(first), C.byref(size), four, 4, C.byref(n)) == 0 and n.value == 11
    assert list(four) == _lib.plan_record(hip_lib, 0)[3][:4] + [-1]
    assert hip_lib.dh_plan_record(0, C.byref(name), C.byref(first), C.byref(size), None, 4, C.byref(n)) == EINVAL
    assert hip_lib.dh_plan_record(0, None, C.byref(first), C.byref(size), None, 0, C.byref(n)) == EINVAL


# ---- host-built blobs parse ------------------------------------------------------------------------------------------------------

def check_info(info, want):
    for k, v in want.items():
        assert getattr(info, k) == v, (k, getattr(info, k), v)


def test_host_built_blobs_parse_and_cover_every_record(hip_lib):
    seen = set()
    for (name, n), (blob, want, ids) in model_blobs().items():
        rc, info = inspect(hip_lib, blob)
        assert rc == 0, (name, n)
        check_info(info, dict(want, nstreams=1, num_ops=0, num_events=0))
        assert blob[:4] == b'DHPL' and len(steps_of(blob)[0]) == len(ids) and steps_of(blob)[1] + want['weight_bytes'] == len(blob)
        seen |= set(ids)
    # ids no such model reaches: a one-step blob from the ctypes structs (grouped and paired launches come from the executor's
    # merge passes over a bound plan, never from binding a step)
    missing = sorted(set(range(F_COUNT)) - seen)
    assert {S.ALL_FUNCTIONS.index('dh_conv2d_dw_group_f32'), S.ALL_FUNCTIONS.index('dh_conv2d_pair_f32')} <= set(missing)
    for fn in range(F_COUNT):                                  # (every id by hand, the reached ones included)
        blob = hand_blob([fn])
        rc, info = inspect(hip_lib, blob)
        assert rc == 0, S.ALL_FUNCTIONS[fn]
        check_info(info, dict(version=S.blob_version([fn]), batch=2, num_inputs=1, num_outputs=1, num_steps=1, arena_bytes=4096,
                              weight_bytes=0, byte_bytes=0, nstreams=1, num_ops=0, num_events=0))
        seen.add(fn)
    assert seen == set(range(F_COUNT))                         # every record occurs in at least one accepted blob
    print('models reach ids %s; by hand only: %s' % (sorted(set(range(F_COUNT)) - set(missing)), missing))
    # a uint8 input in region 3
    rc, info = inspect(hip_lib, hand_blob([S.ALL_FUNCTIONS.index('dh_normalize_u8_f32')], u8=True))
    assert rc == 0 and info.byte_bytes == 512
    # a later version's stamp on a blob that does not need it: the same layout
    for v in (3, 4):
        assert inspect(hip_lib, put(hand_blob([0, 1]), 4, '<I', v))[0] == 0


def test_version_1_and_version_5_forms(hip_lib):
    blob = reference_blob()
    rc, info2 = inspect(hip_lib, blob)
    v1 = as_version_1(blob)
    rc, info = inspect(hip_lib, v1)
    assert rc == 0 and info.version == 1 and len(v1) == len(blob) - 8 - 8 * info.num_inputs
    for k in ('batch', 'num_inputs', 'num_outputs', 'num_steps', 'arena_bytes', 'weight_bytes', 'byte_bytes'):
        assert getattr(info, k) == getattr(info2, k), k
    assert inspect(hip_lib, put(v1, 4, '<I', 0))[0] == EINVAL and inspect(hip_lib, put(blob, 4, '<I', 6))[0] == EINVAL
    assert inspect(hip_lib, put(blob, 4, '<I', 1))[0] == EINVAL          # (a version-2 layout read as version 1: sizes do not add up)
    # version 5: the hand-made three-stream table of tests/test_plan_streams_host.py over seven launches
    copy = S.ALL_FUNCTIONS.index('dh_copy_channels_f32')
    section = S.pack_schedule(PS.HAND, 3, 1)
    v5 = hand_blob([copy] * len(PS.HAND), section=section)
    rc, ops, nev = PS.build_ops(hip_lib, PS.HAND, 3, 1)
    rc5, info = inspect(hip_lib, v5)
    assert rc == 0 and rc5 == 0
    check_info(info, dict(version=5, num_steps=7, nstreams=3, num_ops=len(ops), num_events=nev))
    at = steps_of(v5)[1]
    assert v5[at:at + len(section)] == section and at + len(section) == len(v5)
    for field, value in [(0, 5), (0, 2), (4, 8), (8, 6), (8, 8), (12, 3), (12, 5)]:      # nstreams, npre, #entries, #waits
        assert inspect(hip_lib, put(v5, at + field, '<I', value))[0] == EINVAL, (field, value)
    assert inspect(hip_lib, put(v5, 4, '<I', 4))[0] == EINVAL            # the section without the stamp: trailing bytes
    assert inspect(hip_lib, put(hand_blob([copy] * 7), 4, '<I', 5))[0] == EINVAL      # the stamp without the section
    # ... and the schedule of a real two-stream plan over its host-bound steps
    plan = PS.get_plan('reception', 2, 'list')
    section = S.schedule_section(plan.steps, plan.nstreams, multi_stream=True)
    blob, want, _ = host_blob(plan, 1, section)
    rc, ops, nev = PS.build_ops(hip_lib, PS.schedule.schedule_entries(plan.steps), 2, 0)
    rc5, info = inspect(hip_lib, blob)
    assert rc == 0 and rc5 == 0 and want['version'] == 5
    check_info(info, dict(want, nstreams=2, num_ops=len(ops), num_events=nev))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_every_prefix_and_any_other_length_is_refused(hip_lib):
    blob = reference_blob()
    assert inspect(hip_lib, blob)[0] == 0
    info = _lib.PlanInfo()
    buf = (C.c_char * (len(blob) + 1)).from_buffer_copy(blob + b'\0')
    for n in range(len(blob)):                                 # (one missing trailing byte is the longest of them)
        assert hip_lib.dh_plan_inspect(buf, n, C.byref(info)) == EINVAL, n
    assert inspect(hip_lib, blob[:-1])[0] == EINVAL
    assert inspect(hip_lib, blob + b'\0')[0] == EINVAL          # one extra trailing byte
    assert hip_lib.dh_plan_inspect(None, len(blob), C.byref(info)) == EINVAL and hip_lib.dh_plan_inspect(buf, len(blob), None) == EINVAL
    assert inspect(hip_lib, b'XXXX' + blob[4:])[0] == EINVAL


def test_broken_step_records_are_refused(hip_lib):
    blob = reference_blob()
    steps, _ = steps_of(blob)
    assert len(steps) >= 4
    for at, fn, nb in steps:
        assert inspect(hip_lib, put(blob, at, '<I', F_COUNT))[0] == EINVAL, (at, 'id')
        assert inspect(hip_lib, put(blob, at, '<I', 0xffffffff))[0] == EINVAL, (at, 'id')
        for d in (-8, 8):
            assert inspect(hip_lib, put(blob, at + 4, '<I', nb + d))[0] == EINVAL, (at, 'payload bytes', d)
            grown = blob[:at + 4] + struct.pack('<I', nb + d) + (blob[at + 8:at + 8 + nb] + bytes(8))[:nb + d] + blob[at + 8 + nb:]
            assert inspect(hip_lib, grown)[0] == EINVAL, (at, 'payload resized', d)
    # the id gate per version: 19 and 20 need version 3, 21 needs version 4
    for fn, first in [(19, 3), (20, 3), (21, 4)]:
        good = hand_blob([0, fn])
        assert struct.unpack_from('<I', good, 4)[0] == first and inspect(hip_lib, good)[0] == 0
        assert inspect(hip_lib, put(good, 4, '<I', first - 1))[0] == EINVAL, fn
        if first < 4:
            assert inspect(hip_lib, put(good, 4, '<I', first + 1))[0] == 0, fn


def test_broken_tagged_pointers_are_refused(hip_lib):
    """every pointer slot the table names -- of a one-step blob per function id and of every step of a model's blob -- with
    region 1 at offset = arena bytes, region 4, and region 0 with an offset"""
    cases = [(hand_blob([fn]), 4096) for fn in range(F_COUNT)]
    ref = reference_blob()
    cases.append((ref, inspect(hip_lib, ref)[1].arena_bytes))
    slots = 0
    for blob, arena_bytes in cases:
        for at, fn, nb in steps_of(blob)[0]:
            _, _, size, offsets = _lib.plan_record(hip_lib, fn)
            assert size == nb
            for off in offsets:
                slot = at + 8 + off
                for bad in ((1 << 60) | arena_bytes, (4 << 60) | 16, 16, (15 << 60), (2 << 60) | (1 << 59)):
                    assert inspect(hip_lib, put(blob, slot, '<Q', bad))[0] == EINVAL, (fn, off, hex(bad))
                for good in (0, (1 << 60) | (arena_bytes - 1)):
                    assert inspect(hip_lib, put(blob, slot, '<Q', good))[0] == 0, (fn, off, hex(good))
                slots += 1
    assert slots >= sum(len(_lib.plan_record(hip_lib, fn)[3]) for fn in range(F_COUNT))
    # region 3 only exists in a uint8 plan
    norm = S.ALL_FUNCTIONS.index('dh_normalize_u8_f32')
    at = steps_of(hand_blob([norm]))[0][0][0] + 8
    assert inspect(hip_lib, put(hand_blob([norm]), at, '<Q', 3 << 60 | 0))[0] == EINVAL
    assert inspect(hip_lib, put(hand_blob([norm], u8=True), at, '<Q', 3 << 60 | 511))[0] == 0
    assert inspect(hip_lib, put(hand_blob([norm], u8=True), at, '<Q', 3 << 60 | 512))[0] == EINVAL


def test_broken_headers_and_tables_are_refused(hip_lib):
    blob = hand_blob([0, 4])
    assert inspect(hip_lib, blob)[0] == 0
    for at, fmt, value, what in [(8, '<i', 0, 'batch 0'), (8, '<i', -1, 'batch < 0'), (28, '<I', 0, 'no input'), (28, '<I', 65, 'inputs'),
                                 (32, '<I', 0, 'no output'), (32, '<I', 4097, 'outputs'), (36, '<I', (1 << 20) + 1, 'steps'),
                                 (36, '<I', 3, 'one step too many'), (36, '<I', 1, 'one step too few'), (40, '<Q', (1 << 40) + 1, 'u8 bytes'),
                                 (20, '<Q', 1, 'weight bytes'), (12, '<Q', 64, 'an arena too small for the output'),
                                 (HEAD, '<Q', (1 << 60) | 4095, 'misaligned input'), (HEAD, '<Q', (2 << 60), 'input in the weights'),
                                 (HEAD, '<Q', (1 << 60) | 4096 - 2 * 64 + 4, 'input leaves the arena'), (HEAD + 8, '<Q', 0, 'no items'),
                                 (HEAD + 16, '<I', 2, 'dtype'), (HEAD + 16, '<I', 1, 'uint8 without region 3'),
                                 (HEAD + 24, '<Q', 4096, 'output offset'), (HEAD + 24 + 8, '<Q', 0, 'no pixels'),
                                 (HEAD + 24 + 16, '<I', 0, 'no channels'), (HEAD + 24 + 16, '<I', 4, 'channels above the pitch'),
                                 (HEAD + 24 + 8, '<Q', 1 << 62, 'pixels overflow')]:
        assert inspect(hip_lib, put(blob, at, fmt, value))[0] == EINVAL, what


# ---- the stand-alone sweep -----------------------------------------------------------------------------------------------------------

def test_plan_blob_sweep_builds_and_passes(tmp_path):
    """tools/plan_blob_sweep.cpp, the stand-alone sweep of the header (its own main(), nothing loaded into Python), built plainly
    and run on a host-built blob: every prefix and every single-byte change in front of the image, each in a heap block of
    exactly its length.  Its sanitizer build (the command in the file's head) is run by hand on a CPU host; this keeps the sweep
    compiling and passing."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe, path = str(tmp_path / 'plan_blob_sweep'), str(tmp_path / 'model.dhplan')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'deephar_amd', 'csrc'),
                        os.path.join(ROOT, 'tools', 'plan_blob_sweep.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    open(path, 'wb').write(reference_blob())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'plan_blob_sweep: ok' in r.stdout, r.stdout + r.stderr
    print(r.stdout.strip())
