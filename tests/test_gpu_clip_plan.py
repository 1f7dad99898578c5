"""Frame-sharded clip models behind the C ABI (include/deephar_hip.h: dh_clip_* and dh_unpack_cut_f32):
ShardedClipModel.export_clip_plan -> dh_clip_create / dh_clip_forward_host must return the bits of Model.predict, for a world
of one (no collective), for a world of two driven through the all-gather callback inside one process, for an SPNet with
many cut tensors and for a pose-only clip model without a head plan; the unpack launch alone must equal the host loop that
shares its index arithmetic; tools/c_host/predict_clip.c runs a container as a process with no Python in it.  Floats are moved,
never computed on, between the stages: every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -7.0


# ---- the unpack launch ------------------------------------------------------------------------------------------------------

def _segments(cp, start, padded, wide_first=False):
    """c in {1, 2, 3, 4, 5, 16} from channel `start` on, then the remainder; wide_first puts the widths of 4 and 16 in front, where
    an aligned `start` makes them 16-byte segments"""
    segs, off = [], start
    for w in ((4, 16, 1, 2, 3, 5) if wide_first else (1, 2, 3, 4, 5, 16)):
        if off + w > cp:
            break
        segs.append((off, w, w + (4 if w % 4 == 0 else 3) if padded else w))
        off += w
    if off < cp:
        segs.append((off, cp - off, cp - off + 4 if padded else cp - off))
    return segs


def _table(lib_mod, ptrs, segs):
    tab = (lib_mod.CutSeg * len(segs))()
    for k, ((off, c, ld), p) in enumerate(zip(segs, ptrs)):
        tab[k].dst, tab[k].ld, tab[k].coff, tab[k].c = p, ld, off, c
    return tab


def _unpack_both(lib, cuda, g, m, tl, p, cp, segs, src_shift=0, dst_shift=0):
    """Runs the segment set through dh_unpack_cut_f32 and dh_unpack_cut_host (destinations pre-filled with a guard value) and
    holds the device result to the host's, guards included.  *_shift: floats by which the base addresses are moved off their
    16-byte alignment.  Returns whether any segment took the 16-byte path."""
    from deephar_amd import _lib
    rng = np.random.default_rng(g * 1000 + cp + len(segs))
    gathered = rng.standard_normal(g * m * tl * p * cp + src_shift).astype(np.float32)
    rows = m * g * tl * p
    host = [np.full(rows * ld + dst_shift, GUARD, np.float32) for _, _, ld in segs]
    tab_h = _table(_lib, [h.ctypes.data + 4 * dst_shift for h in host], segs)
    assert lib.dh_unpack_cut_host(gathered.ctypes.data + 4 * src_shift, g, m, tl, p, cp, tab_h, len(segs)) == 0
    src_d = torch.from_numpy(gathered).to(cuda)
    dev = [torch.full((rows * ld + dst_shift,), GUARD, device=cuda) for _, _, ld in segs]
    tab_d = _table(_lib, [d.data_ptr() + 4 * dst_shift for d in dev], segs)
    tab_dev = torch.frombuffer(bytearray(bytes(tab_d)), dtype=torch.uint8).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.dh_unpack_cut_f32(src_d.data_ptr() + 4 * src_shift, g, m, tl, p, cp, tab_dev.data_ptr(), len(segs), st) == 0
    torch.cuda.synchronize()
    for (off, c, ld), h, d in zip(segs, host, dev):
        assert np.array_equal(d.cpu().numpy(), h), (g, m, tl, p, cp, off, c, ld, src_shift, dst_shift)
    return any(lib.dh_unpack_cut_vec4(cp, off, c, ld, src_d.data_ptr() + 4 * src_shift, d.data_ptr() + 4 * dst_shift)
               for (off, c, ld), d in zip(segs, dev))


def test_unpack_launch_equals_host_loop(hip_lib, cuda):
    """The three G, chunks of one row and of more rows than one work-group's tile (Cp = 581: 14 rows; 7 and 24: 64 rows), packed
    widths that do and do not allow 16-byte accesses, aligned and unaligned channel offsets, pitches ld == c and ld > c."""
    took = set()
    for g, (m, tl, p), cp in [(1, (1, 1, 1), 7), (2, (2, 3, 5), 7), (3, (1, 3, 16), 7), (1, (2, 3, 16), 24), (2, (1, 1, 1), 24),
                              (3, (2, 3, 5), 24), (2, (2, 5, 16), 24), (1, (1, 3, 5), 581), (2, (2, 1, 16), 581), (3, (2, 3, 16), 581),
                              (2, (1, 4, 16), 580)]:
        for start, padded, wide_first in [(0, False, False), (0, True, True), (1, False, True), (4, True, False), (4, False, True)]:
            took.add(_unpack_both(hip_lib, cuda, g, m, tl, p, cp, _segments(cp, start, padded, wide_first)))
    assert took == {False, True}                  # both sides of the 16-byte predicate ran
    # the same segments with one base address off its 16-byte alignment: the scalar path must serve them
    segs = _segments(24, 0, False, wide_first=True)
    assert _unpack_both(hip_lib, cuda, 2, 2, 3, 5, 24, segs) is True
    assert _unpack_both(hip_lib, cuda, 2, 2, 3, 5, 24, segs, src_shift=1) is False
    assert _unpack_both(hip_lib, cuda, 2, 2, 3, 5, 24, segs, dst_shift=1) is False


def test_unpack_launch_with_more_than_64_segments(hip_lib, cuda):
    """100 segments in one launch (an SPNet with actions on several pyramids has dozens): one-channel confidences next to
    four-channel groups, every other one at a padded pitch."""
    segs, off = [], 0
    for k in range(100):
        c = 1 if k % 3 else 4
        segs.append((off, c, c + (4 if k % 2 else 0)))
        off += c + (k % 5 == 0)                    # (a few channels of the packed axis belong to nobody)
    assert off <= 256
    assert _unpack_both(hip_lib, cuda, 2, 2, 3, 16, 256, segs) is True
    assert _unpack_both(hip_lib, cuda, 3, 1, 2, 5, 255, segs) is False


def test_unpack_launch_refuses_bad_requests(hip_lib, cuda):
    t = torch.zeros(64, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    assert hip_lib.dh_unpack_cut_f32(None, 1, 1, 1, 1, 7, t.data_ptr(), 1, st) == -1
    assert hip_lib.dh_unpack_cut_f32(t.data_ptr(), 1, 1, 1, 1, 7, None, 1, st) == -1
    assert hip_lib.dh_unpack_cut_f32(t.data_ptr(), 0, 1, 1, 1, 7, t.data_ptr(), 1, st) == -1
    assert hip_lib.dh_unpack_cut_f32(t.data_ptr(), 1, 1, 1, 1, 8193, t.data_ptr(), 1, st) == -2      # wider than the LDS tile


# ---- whole clip models -------------------------------------------------------------------------------------------------------

class _Case:
    """A clip model, clips, Model.predict of them, and its containers by (world, uint8) -- built once per module."""

    def __init__(self, model, clips):
        self.model, self.clips = model, clips
        ref = model.predict(clips, batch_size=len(clips))
        self.ref = ref if isinstance(ref, list) else [ref]
        self.sharded, self.blobs = {}, {}

    def scm(self, world):
        from deephar_amd import parallel
        if world not in self.sharded:
            self.sharded[world] = parallel.ShardedClipModel(self.model, rank=0, world=world)
        return self.sharded[world]

    def blob(self, world, tmp_path, uint8=False):
        if (world, uint8) not in self.blobs:
            path = str(tmp_path / 'model.dhclip')
            nbytes = self.scm(world).export_clip_plan(path, len(self.clips), uint8=uint8)
            self.blobs[(world, uint8)] = open(path, 'rb').read()
            assert len(self.blobs[(world, uint8)]) == nbytes
        return self.blobs[(world, uint8)]


@pytest.fixture(scope='module')
def merge(hip_lib, cuda):
    from test_gpu_models import _merge
    m, _ = _merge(2, 8, 16, 2, num_actions=15)
    return _Case(m, np.random.default_rng(31).uniform(-1, 1, (2, 8, 256, 256, 3)).astype(np.float32))


@pytest.fixture(scope='module')
def spnet(hip_lib, cuda):
    from test_gpu_models import _spnet
    m, cfg, _, _ = _spnet(8, 'pa16j2d', 15, 2, [1, 2], 160, replica=True, res=128)
    case = _Case(m, np.random.default_rng(32).uniform(-1, 1, (2, 8, 128, 128, 3)).astype(np.float32))
    case.cfg = cfg
    return case


def _create(lib, blob, rank=0, cb=None):
    from deephar_amd import _lib
    h = C.c_void_p()
    rc = lib.dh_clip_create(blob, len(blob), rank, cb if cb is not None else _lib.ALLGATHER_FN(), None, C.byref(h))
    assert rc == 0, rc
    return h


def _forward_host(lib, clip, frames, ref, m, skip=()):
    """dh_clip_forward_host on `frames` -> host arrays shaped like ref[:m]; outputs in `skip` get a NULL pointer and stay NaN"""
    frames = np.ascontiguousarray(frames[:m])
    host = [np.full((m,) + r.shape[1:], np.nan, np.float32) for r in ref]
    outs = (C.c_void_p * len(host))(*[None if k in skip else h.ctypes.data for k, h in enumerate(host)])
    assert lib.dh_clip_forward_host(clip, frames.ctypes.data, m, outs) == 0
    return host


def _same(host, ref, m, skip=()):
    for k, (h, r) in enumerate(zip(host, ref)):
        if k in skip:
            assert np.all(np.isnan(h)), ('unwanted output written', k)
        else:
            assert np.array_equal(h, r[:m]), ('output', k)


def test_world_1_container_reproduces_predict(merge, hip_lib, tmp_path):
    """No collective (NULL callback): the packed tensor is read where the frame plan left it.  Also fewer clips than the plans
    hold, and one pass-through and one head output not wanted."""
    blob = merge.blob(1, tmp_path)
    info = merge.scm(1).info
    assert blob[:4] == b'DHCL' and info['packed_channels'] == 581
    n = len(merge.clips)
    clip = _create(hip_lib, blob)
    try:
        assert hip_lib.dh_clip_world(clip) == 1 and hip_lib.dh_clip_batch(clip) == n and hip_lib.dh_clip_input_is_u8(clip) == 0
        assert hip_lib.dh_clip_num_outputs(clip) == len(merge.ref) == 11
        assert hip_lib.dh_clip_frame_items(clip) == merge.clips[0].size
        assert [hip_lib.dh_clip_output_items(clip, k) for k in range(11)] == [r[0].size for r in merge.ref]
        assert hip_lib.dh_clip_output_items(clip, 11) == -1
        _same(_forward_host(hip_lib, clip, merge.clips, merge.ref, n), merge.ref, n)
        _same(_forward_host(hip_lib, clip, merge.clips, merge.ref, 1), merge.ref, 1)
        for skip in [(0,), (5,), (1, 10)]:         # outputs 0, 1 pass through the cut, 2..10 come from the head
            _same(_forward_host(hip_lib, clip, merge.clips, merge.ref, n, skip), merge.ref, n, skip)
        _same(_forward_host(hip_lib, clip, merge.clips, merge.ref, n), merge.ref, n)
        outs = (C.c_void_p * 11)()
        assert hip_lib.dh_clip_forward_host(clip, merge.clips.ctypes.data, n + 1, outs) == -1
        assert hip_lib.dh_clip_forward_host(clip, None, n, outs) == -1
    finally:
        assert hip_lib.dh_clip_destroy(clip) == 0
    # launches between the last frame-stage step and the first head step: one, against one torch copy per cut tensor plus one
    # per pass-through output on the Python path (parallel.ShardedClipModel.forward_device)
    print('merge model: %d cut tensors + %d pass-through outputs -> %d copies on the Python path, 1 unpack launch here'
          % (len(info['cut']), len(info['passthrough']), len(info['cut']) + len(info['passthrough'])))


def test_world_1_device_pointers_on_the_callers_stream(merge, hip_lib, cuda, tmp_path):
    """dh_clip_forward with device pointers on torch's stream; the head plan's inputs are written in place, so dh_forward of
    the head must not have copied them: dh_plan_input_ptr is what dh_clip hands it."""
    blob = merge.blob(1, tmp_path)
    n = len(merge.clips)
    clip = _create(hip_lib, blob)
    try:
        xd = torch.from_numpy(merge.clips).to(cuda)
        outs = [torch.full(r.shape, float('nan'), device=cuda) for r in merge.ref]
        outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(2):                          # the second call re-uses the uploaded segment table
            assert hip_lib.dh_clip_forward(clip, xd.data_ptr(), n, outs_p, st) == 0
        torch.cuda.synchronize()
        for o, r in zip(outs, merge.ref):
            assert np.array_equal(o.cpu().numpy(), r)
    finally:
        hip_lib.dh_clip_destroy(clip)


def test_plan_input_written_in_place_skips_the_copy(hip_lib, cuda, tmp_path):
    """dh_plan_input_ptr: a caller that writes a plan's input where the plan reads it passes that address to dh_forward."""
    from test_gpu_models import _build
    m, _ = _build(2, 1, 16, num_context_per_joint=2, concat_pose_confidence=True)
    x = np.random.default_rng(33).uniform(-1, 1, (2, 256, 256, 3)).astype(np.float32)
    ref = m.predict(x, batch_size=2)
    ref = ref if isinstance(ref, list) else [ref]
    path = str(tmp_path / 'm.dhplan')
    m.export_plan(path, 2)
    blob = open(path, 'rb').read()
    plan = C.c_void_p()
    assert hip_lib.dh_plan_create(blob, len(blob), C.byref(plan)) == 0
    try:
        p = hip_lib.dh_plan_input_ptr(plan, 0)
        assert p and hip_lib.dh_plan_input_ptr(plan, 1) is None and hip_lib.dh_plan_input_ptr(plan, -1) is None
        xd = torch.from_numpy(x).to(cuda)
        st = torch.cuda.current_stream().cuda_stream
        assert hip_lib.dh_copy_channels_f32(xd.data_ptr(), 3, p, 3, x.size // 3, 3, st) == 0      # "written in place"
        outs = [torch.full(r.shape, float('nan'), device=cuda) for r in ref]
        outs_p = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        assert hip_lib.dh_forward(plan, (C.c_void_p * 1)(p), 2, outs_p, st) == 0
        torch.cuda.synchronize()
        for o, r in zip(outs, ref):
            assert np.array_equal(o.cpu().numpy(), r)
        assert hip_lib.dh_forward(plan, (C.c_void_p * 1)(None), 2, outs_p, st) == -1             # a NULL input stays an error
    finally:
        hip_lib.dh_plan_destroy(plan)


def test_world_1_with_uint8_frames(merge, hip_lib, tmp_path):
    x = np.random.default_rng(34).integers(0, 256, merge.clips.shape, dtype=np.uint8)
    ref = merge.model.predict(x, batch_size=len(x))
    clip = _create(hip_lib, merge.blob(1, tmp_path, uint8=True))
    try:
        assert hip_lib.dh_clip_input_is_u8(clip) == 1 and hip_lib.dh_clip_frame_items(clip) == x[0].size
        _same(_forward_host(hip_lib, clip, x, ref, len(x)), ref, len(x))
        _same(_forward_host(hip_lib, clip, x, ref, 1), ref, 1)
    finally:
        hip_lib.dh_clip_destroy(clip)


def _two_ranks(lib, cuda, case, tmp_path):
    """World 2 inside one process: the other rank's packed tensor comes from the frame stage first; this rank's dh_clip gets a
    callback that places its own `send` and that tensor rank-major into `recv`, ordered on the stream it is given."""
    from deephar_amd import _lib
    world, n = 2, len(case.clips)
    scm = case.scm(world)
    tl = scm.info['Tl']
    blob = case.blob(world, tmp_path)
    packed = [torch.from_numpy(np.ascontiguousarray(scm.frame_model.predict(case.clips[:, r * tl:(r + 1) * tl], batch_size=n))).to(cuda)
              for r in range(world)]
    torch.cuda.synchronize()
    for rank in range(world):
        other, calls = packed[1 - rank], []

        def gather(ctx, send, recv, count, stream):
            calls.append(count)
            if count != other.numel():
                return 1
            rc = lib.dh_copy_channels_f32(send, count, recv + 4 * count * rank, count, 1, count, stream)
            return rc or lib.dh_copy_channels_f32(other.data_ptr(), count, recv + 4 * count * (1 - rank), count, 1, count, stream)

        cb = _lib.ALLGATHER_FN(gather)
        bad = C.c_void_p()
        assert lib.dh_clip_create(blob, len(blob), rank, _lib.ALLGATHER_FN(), None, C.byref(bad)) == -1     # world 2 needs a collective
        assert lib.dh_clip_create(blob, len(blob), world, cb, None, C.byref(bad)) == -1                     # no such rank
        clip = _create(lib, blob, rank, cb)
        try:
            assert lib.dh_clip_world(clip) == world and lib.dh_clip_frame_items(clip) == case.clips[0].size // world
            host = _forward_host(lib, clip, case.clips[:, rank * tl:(rank + 1) * tl], case.ref, n)
            assert calls == [other.numel()]
            _same(host, case.ref, n)
        finally:
            lib.dh_clip_destroy(clip)
    return scm.info


def test_world_2_through_the_callback(merge, hip_lib, cuda, tmp_path):
    _two_ranks(hip_lib, cuda, merge, tmp_path)


def test_spnet_with_many_cut_tensors(spnet, hip_lib, cuda, tmp_path):
    """Actions on two pyramids at 128 px: every pose output passes through the cut and every action block reads its own
    pose / visibility / feature tensors.  World 2 through the callback, then world 1."""
    info = _two_ranks(hip_lib, cuda, spnet, tmp_path)
    assert len(info['cut']) > 8 and len(info['passthrough']) >= 2 and info['head_outputs']
    n = len(spnet.clips)
    clip = _create(hip_lib, spnet.blob(1, tmp_path))
    try:
        _same(_forward_host(hip_lib, clip, spnet.clips, spnet.ref, n), spnet.ref, n)
    finally:
        hip_lib.dh_clip_destroy(clip)
    print('spnet: %d cut tensors + %d pass-through outputs -> %d copies on the Python path, 1 unpack launch here'
          % (len(info['cut']), len(info['passthrough']), len(info['cut']) + len(info['passthrough'])))


def test_pose_only_clip_model_has_no_head_blob(spnet, hip_lib, cuda, tmp_path):
    """The pose half of the SPNet as a clip model: every output passes through the cut, the container's head blob is empty and
    the unpack launch writes the caller's outputs directly."""
    from deephar_amd import _lib
    from deephar_amd.models import split_model
    pose_model, _ = split_model(spnet.model, spnet.cfg)
    case = _Case(pose_model, spnet.clips)
    blob = case.blob(2, tmp_path)
    info = _lib.ClipInfo()
    assert hip_lib.dh_clip_inspect(blob, len(blob), C.byref(info)) == 0
    assert info.head_bytes == 0 and info.num_head_outputs == 0 and info.num_outputs == len(case.ref) and info.world == 2
    assert case.scm(2).head_model is None
    _two_ranks(hip_lib, cuda, case, tmp_path)
    for k, r in enumerate(case.ref):               # the same bits as the pose outputs of the whole SPNet
        assert np.array_equal(r, spnet.ref[k])


# ---- a host with no Python in it ---------------------------------------------------------------------------------------------

def _run_c_host(case, tmp_path, extra, exe_name):
    libdir = os.path.join(ROOT, 'deephar_amd', 'csrc')
    exe = str(tmp_path / exe_name)
    cmd = ['gcc', '-O2', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tools', 'c_host', 'predict_clip.c'),
           '-L' + libdir, '-ldeephar_hip', '-Wl,-rpath,' + libdir, '-o', exe] + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return r
    open(str(tmp_path / 'model.dhclip'), 'wb').write(case.blob(1, tmp_path))
    case.clips.tofile(str(tmp_path / 'x.f32'))
    run = subprocess.run([exe, str(tmp_path / 'model.dhclip'), str(tmp_path / 'x.f32'), str(tmp_path / 'out')],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    print(run.stdout.strip())
    for k, want in enumerate(case.ref):
        got = np.fromfile(str(tmp_path / ('out.%d.f32' % k)), np.float32).reshape(want.shape)
        assert np.array_equal(got, want), k
    return r


def test_pure_c_host_runs_a_clip_container(merge, hip_lib, tmp_path):
    """gcc-compiled host, no HIP headers, world 1 with a NULL callback: container + raw frames in, raw outputs out."""
    r = _run_c_host(merge, tmp_path, [], 'predict_clip')
    assert r.returncode == 0, r.stderr


def test_pure_c_host_with_an_rccl_callback(merge, hip_lib, tmp_path):
    """-DDH_WITH_RCCL: the callback is ncclAllGather on a communicator of one rank; the host links RCCL itself.  Skipped, with
    the reason printed, where rccl.h or librccl is not installed or does not link."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    if not os.path.exists(os.path.join(rocm, 'include', 'rccl', 'rccl.h')):
        print('no rccl/rccl.h under %s' % rocm)
        pytest.skip('rccl/rccl.h not found under %s' % rocm)
    extra = ['-DDH_WITH_RCCL', '-D__HIP_PLATFORM_AMD__', '-I' + os.path.join(rocm, 'include'), '-L' + os.path.join(rocm, 'lib'),
             '-lrccl', '-lamdhip64', '-Wl,-rpath,' + os.path.join(rocm, 'lib')]
    r = _run_c_host(merge, tmp_path, extra, 'predict_clip_rccl')
    if r.returncode != 0:
        print('the RCCL variant does not build here:\n' + r.stderr)
        pytest.skip('librccl does not link')
