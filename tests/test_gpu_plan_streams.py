"""Multi-stream plans behind the C ABI, and one launch for all outputs (include/deephar_hip.h: dh_pack_outputs_f32, blob
version 5, dh_plan_num_streams): the pack kernel against NumPy slicing on NaN-guarded buffers; Model.export_plan(...,
multi_stream=True) -> dh_plan_create / dh_forward / dh_forward_host must return the bits of a ONE-stream Model.predict, also
with one stream delayed against the other; malformed schedule sections are refused; a clip container with a two-stream frame
stage equals ShardedClipModel.  The feature moves no bit: every comparison is exact."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_plan_streams_host import GUARD_FLOATS, PACK_SEGMENTS, check_packed, out_table, pack_case      # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1


# ---- 1. the pack kernel --------------------------------------------------------------------------------------------------------

def _pack_on_device(lib, cuda, case, null=()):
    """slabs and NaN-guarded destinations on the device, ONE dh_pack_outputs_f32 call, everything read back into the case's host
    arrays; -> (host copies of the destinations, the 16-byte answer per segment)"""
    slabs = [torch.from_numpy(np.ascontiguousarray(c[0])).to(cuda) for c in case]
    dsts = [torch.full((c[2].size + 2 * GUARD_FLOATS + 4,), float('nan'), device=cuda) for c in case]
    assert all(t.data_ptr() % 16 == 0 for t in slabs + dsts)
    ptrs = [None if k in null else d.data_ptr() + 4 * (GUARD_FLOATS + c[3]) for k, (c, d) in enumerate(zip(case, dsts))]
    tab = out_table(case, [s.data_ptr() for s in slabs], ptrs)
    assert lib.dh_pack_outputs_f32(tab, len(case), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for c, s in zip(case, slabs):
        c[0][...] = s.cpu().numpy()                                 # (the slab as the kernel left it: check_packed looks at it)
    vec = [lib.dh_pack_outputs_vec4(t.C, t.ld, t.src, t.dst) for t in tab]
    return [d.cpu().numpy() for d in dsts], vec


@pytest.mark.parametrize('m', [1, 3])
def test_pack_kernel_equals_numpy(m, hip_lib, cuda):
    case = pack_case(PACK_SEGMENTS, m, 60 + m)
    null = (3,)                                                     # one NULL dst in the middle
    dsts, vec = _pack_on_device(hip_lib, cuda, case, null)
    check_packed(case, dsts, null)
    # the two 48-pitch segments move 16 bytes per lane, the misaligned and the 6-pitch one do not (nor C = 1, 2, 3)
    assert vec == [0, 0, 0, 0, 1, 1, 0, 0]
    dsts, _ = _pack_on_device(hip_lib, cuda, case)                  # ... and with every output wanted
    check_packed(case, dsts)
    # 70 one-channel segments of 4 pixels: crosses the 64-segment chunk of one launch
    many = pack_case([(4, 1, 1 + k % 3, 0, 0) for k in range(70)], m, 70 + m)
    dsts, _ = _pack_on_device(hip_lib, cuda, many, null=(0, 63, 64))
    check_packed(many, dsts, null=(0, 63, 64))


def test_pack_kernel_refuses_bad_tables(hip_lib, cuda):
    from deephar_amd import _lib
    t = torch.full((64,), float('nan'), device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    tab = (_lib.OutSeg * 2)()
    for k in range(2):
        tab[k].src, tab[k].dst, tab[k].npix, tab[k].C, tab[k].ld = t.data_ptr(), t.data_ptr() + 128, 4, 2, 2
    tab[1].ld = 1                                                    # a pitch below the channels: nothing is launched
    assert hip_lib.dh_pack_outputs_f32(tab, 2, st) == EINVAL
    assert hip_lib.dh_pack_outputs_f32(None, 1, st) == EINVAL and hip_lib.dh_pack_outputs_f32(None, 0, st) == 0
    tab[0].dst = tab[1].dst = None                                   # all outputs unwanted: nothing to do
    assert hip_lib.dh_pack_outputs_f32(tab, 2, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all())


# ---- whole models --------------------------------------------------------------------------------------------------------------

def _spnet_model(streams=1, policy='list'):
    from test_gpu_models import _spnet
    m, cfg, _, _ = _spnet(8, 'pa16j2d', 15, 2, [1, 2], 160, replica=True, res=128)
    m.num_streams, m.stream_policy = streams, policy
    return m, cfg


def _reception_model(streams=1, policy='list'):
    from test_gpu_models import _build
    m, _ = _build(2, 2, 16, num_context_per_joint=2)
    m.num_streams, m.stream_policy = streams, policy
    return m


class _Ref:
    """a one-stream model, inputs and its Model.predict -- built once per module, never changed"""

    def __init__(self, model, x):
        self.model, self.x = model, x
        ref = model.predict(x, batch_size=len(x))
        self.ref = [np.array(r, copy=True) for r in (ref if isinstance(ref, list) else [ref])]
        for r in self.ref:
            r.setflags(write=False)


@pytest.fixture(scope='module')
def spnet_ref(hip_lib, cuda):
    m, _ = _spnet_model()
    return _Ref(m, np.random.default_rng(41).uniform(-1, 1, (2, 8, 128, 128, 3)).astype(np.float32))


@pytest.fixture(scope='module')
def reception_ref(hip_lib, cuda):
    return _Ref(_reception_model(), np.random.default_rng(42).uniform(-1, 1, (3, 256, 256, 3)).astype(np.float32))


def _export(m, n, tmp_path, name, **kw):
    path = str(tmp_path / name)
    nbytes = m.export_plan(path, n, **kw)
    blob = open(path, 'rb').read()
    assert len(blob) == nbytes and blob[:4] == b'DHPL'
    return blob


def _version(blob):
    return struct.unpack_from('<I', blob, 4)[0]


def _create(lib, blob):
    h = C.c_void_p()
    rc = lib.dh_plan_create(blob, len(blob), C.byref(h))
    assert rc == 0, rc
    return h


def _forward_device(lib, cuda, plan, x, ref, before=None):
    """dh_forward on torch's current stream into NaN-filled outputs; `before(stream)` may enqueue something first"""
    xd = torch.from_numpy(x).to(cuda)
    outs = [torch.full(r.shape, float('nan'), device=cuda) for r in ref]
    outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    if before is not None:
        before(st)
    assert lib.dh_forward(plan, (C.c_void_p * 1)(xd.data_ptr()), len(x), outs_p, st) == 0
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _forward_host(lib, plan, x, ref, m):
    host = [np.full((m,) + r.shape[1:], np.nan, np.float32) for r in ref]
    xin = np.ascontiguousarray(x[:m])
    outs_h = (C.c_void_p * len(host))(*[h.ctypes.data for h in host])
    assert lib.dh_forward_host(plan, (C.c_void_p * 1)(xin.ctypes.data), m, outs_h) == 0
    return host


def _same(got, ref, m=None):
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r if m is None else r[:m]), ('output', k)


def _exports_reproduce_one_stream_predict(lib, cuda, tmp_path, case, m):
    """`m`: the multi-stream twin of case.model (same synthetic weights).  The version-5 export and the default export of it
    both return the bits of the one-stream predict, through device pointers on the caller's stream and host pointers, m = 1."""
    n = len(case.x)
    m.executor.tune_table = case.model.executor.tune_table          # (tilings never move a bit; this only spares the timing)
    assert m.plan.nstreams == m.num_streams
    v5 = _export(m, n, tmp_path, 'multi.dhplan', multi_stream=True)
    plain = _export(m, n, tmp_path, 'plain.dhplan')
    assert _version(v5) == 5 and _version(plain) <= 4 and len(v5) > len(plain)
    # both executors run the same list: the program of the exported blob is the bound plan's own
    from deephar_amd import _lib
    info = _lib.PlanInfo()
    assert lib.dh_plan_inspect(v5, len(v5), C.byref(info)) == 0
    ops, nevents = m.executor.bound[n].program()
    assert (info.nstreams, info.num_ops, info.num_events) == (m.plan.nstreams, len(ops), nevents)
    for graph in (False, True):                                     # ... and what Python enqueues from it returns the same bits
        m.executor.use_graph = graph
        got = m.predict(case.x, batch_size=n)
        _same(got if isinstance(got, list) else [got], case.ref)
    for blob, streams in [(v5, m.plan.nstreams), (plain, 1)]:
        plan = _create(lib, blob)
        try:
            assert lib.dh_plan_num_streams(plan) == streams
            assert bool(lib.dh_plan_side_stream(plan, 1)) == (streams > 1)
            assert lib.dh_plan_side_stream(plan, 0) is None and lib.dh_plan_side_stream(plan, streams) is None
            for _ in range(2):
                _same(_forward_device(lib, cuda, plan, case.x, case.ref), case.ref)
            _same(_forward_host(lib, plan, case.x, case.ref, 1), case.ref, 1)
            _same(_forward_host(lib, plan, case.x, case.ref, n), case.ref)
        finally:
            assert lib.dh_plan_destroy(plan) == 0
    return v5, plain


@pytest.mark.parametrize('streams', [2, 3])
def test_spnet_tail_plans_reproduce_one_stream_predict(streams, spnet_ref, hip_lib, cuda, tmp_path):
    m, _ = _spnet_model(streams, 'tail')
    v5, plain = _exports_reproduce_one_stream_predict(hip_lib, cuda, tmp_path, spnet_ref, m)
    # the version-5 blob is the plain one with the schedule section in front of the weight image
    at, end = _section(v5)
    assert v5[:4] + struct.pack('<I', _version(plain)) + v5[8:at] + v5[end:] == plain


@pytest.mark.parametrize('streams', [2, 3])
def test_reception_list_plans_reproduce_one_stream_predict(streams, reception_ref, hip_lib, cuda, tmp_path):
    _exports_reproduce_one_stream_predict(hip_lib, cuda, tmp_path, reception_ref, _reception_model(streams, 'list'))


def test_single_stream_export_is_unchanged_by_the_keyword(reception_ref, hip_lib, cuda, tmp_path):
    """one stream: multi_stream=True writes the ordinary blob, byte for byte"""
    n = len(reception_ref.x)
    a = _export(reception_ref.model, n, tmp_path, 'a.dhplan')
    b = _export(reception_ref.model, n, tmp_path, 'b.dhplan', multi_stream=True)
    assert a == b and _version(a) == 2


# ---- 4. one stream delayed against the other ------------------------------------------------------------------------------------

def test_tail_plan_under_stream_delays(spnet_ref, hip_lib, cuda, tmp_path):
    """6 eager passes; before each a few bounded idle waves of 20-300 us go on the caller's stream (the side stream races ahead
    to its waits) or on the plan's side stream (the caller's stream runs ahead and re-uses arena space as early as the schedule
    lets it).  Every pass returns the bits of the one-stream predict."""
    m, _ = _spnet_model(2, 'tail')
    m.executor.tune_table = spnet_ref.model.executor.tune_table
    plan = _create(hip_lib, _export(m, len(spnet_ref.x), tmp_path, 'multi.dhplan', multi_stream=True))
    rng = np.random.default_rng(43)
    try:
        side = hip_lib.dh_plan_side_stream(plan, 1)
        assert side and hip_lib.dh_plan_num_streams(plan) == 2
        for it in range(6):
            delays = [int(d) for d in rng.integers(20, 300, size=3)]

            def before(st, it=it, delays=delays):
                for us in delays:
                    assert hip_lib.dh_stream_spin_us(st if it % 2 == 0 else side, us) == 0
            _same(_forward_device(hip_lib, cuda, plan, spnet_ref.x, spnet_ref.ref, before), spnet_ref.ref)
    finally:
        assert hip_lib.dh_plan_destroy(plan) == 0


# ---- 5. malformed version-5 blobs -----------------------------------------------------------------------------------------------

def _section(blob):
    """-> (offset, end) of the schedule section of a version-5 blob"""
    ver, n, arena, wbytes, nin, nout, nsteps, u8b = struct.unpack_from('<IiQQIIIQ', blob, 4)
    at = 4 + struct.calcsize('<IiQQIIIQ') + 24 * nin + 24 * nout
    for _ in range(nsteps):
        at += 8 + struct.unpack_from('<II', blob, at)[1]
    ns, npre, nent, nwaits = struct.unpack_from('<IIII', blob, at)
    end = at + 16 + 16 * nent + 4 * nwaits
    assert ver == 5 and len(blob) - end == wbytes
    return at, end


def test_malformed_schedule_sections_are_refused(reception_ref, hip_lib, cuda, tmp_path):
    m = _reception_model(2, 'list')
    m.executor.tune_table = reception_ref.model.executor.tune_table
    blob = _export(m, 2, tmp_path, 'multi.dhplan', multi_stream=True)
    at, end = _section(blob)
    ns, npre, nent, nwaits = struct.unpack_from('<IIII', blob, at)
    assert ns == 2 and nent >= 8 and nwaits >= 1

    def patched(off, value):
        b = bytearray(blob)
        struct.pack_into('<I', b, off, value)
        return bytes(b)

    bad = {'truncated section': blob[:end - 4] + blob[end:],
           'section cut off': blob[:at + 20],
           'nstreams 5': patched(at, 5),
           'nstreams 0': patched(at, 0),
           'wait beyond the table': patched(at + 16 + 16 * nent, nent + 5),
           'wait count off': patched(at + 12, nwaits + 1),
           'stream out of range': patched(at + 16 + 4, 2)}
    for what, b in bad.items():
        h = C.c_void_p()
        assert hip_lib.dh_plan_create(b, len(b), C.byref(h)) == EINVAL and not h.value, what
    plan = _create(hip_lib, blob)                                    # the blob itself is fine
    assert hip_lib.dh_plan_destroy(plan) == 0


# ---- 6. a clip container with a two-stream frame stage ---------------------------------------------------------------------------

def test_clip_container_with_a_two_stream_frame_stage(spnet_ref, hip_lib, cuda, tmp_path):
    from deephar_amd import _lib, parallel
    m, _ = _spnet_model()
    scm = parallel.ShardedClipModel(m, rank=0, world=1)
    scm.frame_model.num_streams, scm.frame_model.stream_policy = 2, 'tail'
    want = scm.predict(spnet_ref.x)
    _same(want, spnet_ref.ref)
    path = str(tmp_path / 'model.dhclip')
    n = len(spnet_ref.x)
    nbytes = scm.export_clip_plan(path, n, multi_stream=True)
    blob = open(path, 'rb').read()
    info = _lib.ClipInfo()
    assert len(blob) == nbytes and hip_lib.dh_clip_inspect(blob, len(blob), C.byref(info)) == 0
    assert scm.frame_model.plan.nstreams == 2 and _version(blob[info.frames_offset:]) == 5
    clip = C.c_void_p()
    assert hip_lib.dh_clip_create(blob, len(blob), 0, _lib.ALLGATHER_FN(), None, C.byref(clip)) == 0
    try:
        host = [np.full(r.shape, np.nan, np.float32) for r in want]
        outs = (C.c_void_p * len(host))(*[h.ctypes.data for h in host])
        for _ in range(2):
            assert hip_lib.dh_clip_forward_host(clip, spnet_ref.x.ctypes.data, n, outs) == 0
            _same(host, want)
    finally:
        assert hip_lib.dh_clip_destroy(clip) == 0
