"""Serialise a bound plan for the C-level executor of the library (include/deephar_hip.h: dh_plan_create / dh_forward /
dh_plan_destroy -- SURVEY.md 8b's plan / execute pair): a host written in C or C++ runs the model without Python.

Blob (little endian), version 2 (version 1 = float inputs only, no `u8 bytes` / `dtype`, still read by the library);
a plan with a strided depthwise or a transposed-convolution step (downsampling_type='conv') is written as version 3: the
same layout with the two further function ids -- every other plan stays version 2, byte for byte what it was; a plan with
a split-bf16 transposed convolution (downsampling_type='conv' under a gemm_precision other than 'f32') is version 4, again
the same layout with one more function id (V4_FUNCTIONS) -- every other plan keeps its version 2 or 3:
    header   'DHPL' u32 version | i32 batch n | u64 arena bytes | u64 weight bytes | u32 #inputs | u32 #outputs | u32 #steps
             | u64 u8 bytes (size of region 3: the byte staging buffers of a uint8-input plan, 0 otherwise)
    inputs   per input : u64 tagged pointer of the buffer dh_forward copies the caller's data into (region 1: the plan's
             float input inside the arena; region 3: the byte staging buffer of a uint8 plan) | u64 elements per batch
             item | u32 dtype (0 float32, 1 uint8) | u32 0
    outputs  per output: u64 arena byte offset | u64 pixels per batch item | u32 channels | u32 pixel pitch (floats)
    steps    per launch: u32 function id | u32 payload bytes | payload
               struct functions: the argument struct, byte for byte, then one u64 per further argument
               scalar functions: one u64 per argument (ints sign-extended, floats as their bit pattern in the low half)
             every device pointer (struct field or scalar) is written as 0 (NULL) or (region << 60) | byte offset,
             region 1 = the activation arena, 2 = the weight image, 3 = the uint8 input staging
    weights  the weight image (packed conv / depthwise kernels, BN affines, grids), every tensor 256-byte aligned
Launch order is the plan's step order, a valid single-stream schedule of the graph; tilings are the bound plan's
(autotuned) ones, so dh_forward reproduces Model.predict bit for bit.

Version 5 (dump_plan(..., multi_stream=True) of a plan with more than one stream -- Model.num_streams > 1; every other export,
a several-stream plan under the default keyword included, stays the version 2 - 4 blob it was, byte for byte): the same layout
with a schedule section between the steps and the weight image, the engine's multi-stream schedule for dh_forward:
    schedule u32 nstreams | u32 npre (leading entries that stage the inputs: launched on stream 0 in front of the fork)
             | u32 #entries | u32 #waits (of all entries)
             per entry (one per bound call of the exporter, absorbed no-ops included, in launch order):
               u32 step (index into `steps`, or 0xffffffff: no launch -- the call's work moved into an earlier grouped /
               paired launch; it keeps its entry so that it still records its event at its own place)
               | u32 stream | u32 flags (bit 0: an event is recorded behind it) | u32 #waits of this entry
             waits   u32 entry index per wait, entry by entry: an EARLIER entry on another stream that records
The table is schedule.schedule_entries of the bound calls, the one BoundPlan.launch_all runs from.  The library turns it into
the enqueue program both executors run (csrc/plan_sched.h: fork, per-entry waits / launch / record, the relay rule, join) and
refuses a table that breaks one of the rules above, more than 4 streams, or sizes that do not add up.

Clip container (little endian), version 1: a frame-sharded clip model (parallel.ShardedClipModel) as ONE file for
dh_clip_inspect / dh_clip_create / dh_clip_forward -- the two stage plans and the cut table between them:
    header   'DHCL' u32 version | u32 world (ranks G) | u32 T (frames per clip) | u32 Tl (= T / world, frames per rank)
             | u32 packed channels Cp | u64 P (pixels per frame of every cut tensor: prod(shape[:-1])) | u32 #cut | u32 #outputs
             | u64 frames plan offset | u64 frames plan bytes | u64 head plan offset | u64 head plan bytes (0: no head)
    cut      per cut tensor, in the order of the head plan's inputs: u32 channel offset in the packed axis | u32 channels
    outputs  per model output, in model order: u32 kind (0: cut tensor passed through, 1: output of the head plan) | u32 index
             (of the cut tensor / of the head plan's output)
    plans    the frames plan blob ('DHPL', above) at the next 256-byte boundary behind the tables, the head plan blob at the
             next 256-byte boundary behind it; the container ends with the head plan (without one: at that boundary, zero filled)
"""
import ctypes as C
import struct

import numpy as np

from .. import _lib
from .schedule import schedule_entries      # (its home is the scheduler: the table BoundPlan runs from)

MAGIC, VERSION = b'DHPL', 2
FUNCTIONS = ['dh_conv2d_f32', 'dh_dwconv2d_f32', 'dh_pool2d_f32', 'dh_upsample2x_add_f32', 'dh_eltwise_f32',
             'dh_softargmax2d_f32', 'dh_context_aggregation_f32', 'dh_depth_means_f32', 'dh_softargmax1d_f32',
             'dh_kronecker_f32', 'dh_global_maxmin_softmax_f32', 'dh_copy_channels_f32', 'dh_zeropad2d_f32',
             'dh_depth_from_maps_f32', 'dh_softargmax2d_context_f32', 'dh_normalize_u8_f32', 'dh_conv2d_dw_group_f32',
             'dh_conv2d_pair_f32', 'dh_conv2d_seg_f32', 'dh_dwconv2d_strided_f32', 'dh_conv2d_transpose2x2_f32']
V3_FUNCTIONS = FUNCTIONS.index('dh_dwconv2d_strided_f32')     # function ids from here on make a blob version 3
# appended behind FUNCTIONS (the ids of versions 1 - 3 do not move): function ids from len(FUNCTIONS) on make a blob version 4
V4_FUNCTIONS = ['dh_conv2d_transpose2x2_split_f32']
ALL_FUNCTIONS = FUNCTIONS + V4_FUNCTIONS
ARENA, WEIGHTS, BYTES = 1, 2, 3


class _Regions:
    def __init__(self, bp):
        self.base = bp.base
        self.end = bp.base + bp.arena.numel() * 4
        st = bp.store
        tensors = [e[0] for e in st.conv.values()] + [e[0] for e in st.dw.values()] + list(st.const.values())
        for e in st.bn.values():
            tensors += [e[0], e[1]]
        self.known = sorted(((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), t) for t in tensors),
                            key=lambda r: r[0])
        self.offset = {}          # tensor data_ptr -> byte offset in the weight image
        self.image = []
        self.size = 0
        # uint8-input plans: the byte staging buffers (one per model input) form region 3, 256-byte aligned each
        self.u8 = []              # (lo, hi, region offset)
        self.u8_size = 0
        for buf, _, _ in (bp.u8 or {}).values():
            self.u8.append((buf.data_ptr(), buf.data_ptr() + buf.numel(), self.u8_size))
            self.u8_size = (self.u8_size + buf.numel() + 255) & ~255

    def tag(self, ptr):
        ptr = int(ptr or 0)
        if ptr == 0:
            return 0
        if self.base <= ptr < self.end:
            return (ARENA << 60) | (ptr - self.base)
        for lo, hi, off in self.u8:
            if lo <= ptr < hi:
                return (BYTES << 60) | (off + ptr - lo)
        for lo, hi, t in self.known:
            if lo <= ptr < hi:
                if lo not in self.offset:
                    self.size = (self.size + 255) & ~255
                    self.offset[lo] = self.size
                    self.image.append((self.size, t))
                    self.size += hi - lo
                return (WEIGHTS << 60) | (self.offset[lo] + ptr - lo)
        raise ValueError('pointer 0x%x belongs neither to the arena nor to the weight store' % ptr)


def _is_ptr_type(t):
    return t is C.c_void_p


def _is_struct_ptr(t):
    return isinstance(getattr(t, '_type_', None), type) and issubclass(t._type_, C.Structure)


def _scalars(sig, args, tag):
    assert len(sig) == len(args), (len(sig), len(args))
    parts = []
    for t, a in zip(sig, args):
        if _is_ptr_type(t):
            parts.append(struct.pack('<Q', tag(a)))
        elif t is C.c_float:
            parts.append(struct.pack('<fI', float(a), 0))
        else:
            parts.append(struct.pack('<q', int(a)))
    return b''.join(parts)


def pack_steps(launches, tag):
    """-> [bytes]: the step record of every launch (module docstring).  launches: [(entry point name, [argument structs],
    [the arguments behind them, without the stream])], as engine/binding.py binds them; tag(ptr) -> the tagged pointer
    (region << 60) | byte offset of a non-null address.  Pointer fields and pointer arguments are the c_void_p ones of the
    ctypes structs and of _lib.SIGNATURES (csrc/plan_blob.h holds the reader's table; tests/test_plan_blob_host.py compares
    the two).  No device needed."""
    names = {n: i for i, n in enumerate(ALL_FUNCTIONS)}
    steps = []
    for name, structs, scalars in launches:
        if name not in names:
            raise ValueError('%s has no serialised form' % name)
        payload = b''
        for obj in structs:                                   # (dh_conv2d_dw_group_f32 takes two structs)
            raw = bytearray(bytes(obj))
            for fname, ftype in obj._fields_:
                if _is_ptr_type(ftype):
                    off = getattr(type(obj), fname).offset
                    raw[off:off + 8] = struct.pack('<Q', tag(getattr(obj, fname) or 0))
            payload += bytes(raw)
        sig = _lib.SIGNATURES[name][1][len(structs):-1]      # without the structs in front and the stream behind
        payload += _scalars(sig, scalars, lambda p: tag(p or 0))
        steps.append(struct.pack('<II', names[name], len(payload)) + payload)
    return steps


def pack_plan(batch, arena_bytes, inputs, outputs, launches, tag, weights=b'', u8_bytes=0, section=b''):
    """-> bytes: a plan blob (module docstring).  inputs: [(address of the buffer dh_forward copies to, elements per batch
    item, dtype 0 float32 / 1 uint8)]; outputs: [(arena byte offset, pixels per batch item, channels, pixel pitch)];
    launches, tag: as for pack_steps; weights: the weight image, or a callable that returns it once every pointer has gone
    through `tag` (the exporter lays the image out as `tag` meets its tensors); section: the schedule section (pack_schedule)
    of a version-5 blob.  No device needed."""
    steps = pack_steps(launches, tag)
    ins = b''.join(struct.pack('<QQII', tag(ptr), int(items), int(dtype), 0) for ptr, items, dtype in inputs)
    outs = b''.join(struct.pack('<QQII', int(off), int(npix), int(c), int(ld)) for off, npix, c, ld in outputs)
    image = bytes(weights() if callable(weights) else weights)
    version = plan_version((struct.unpack_from('<I', st)[0] for st in steps), section)
    head = MAGIC + struct.pack('<IiQQIIIQ', version, int(batch), int(arena_bytes), len(image), len(inputs), len(outputs),
                               len(steps), int(u8_bytes))
    return head + ins + outs + b''.join(steps) + section + image


def blob_version(function_ids):
    """The blob version a plan with these step function ids is written as: the lowest that knows them all."""
    top = max(function_ids, default=0)
    return 4 if top >= len(FUNCTIONS) else (3 if top >= V3_FUNCTIONS else VERSION)


SCHEDULE_VERSION = 5            # blob version of a plan written with its multi-stream schedule
NO_LAUNCH = 0xffffffff          # schedule entry whose work moved into an earlier grouped / paired launch


def pack_schedule(entries, nstreams, npre=0):
    """-> bytes: the schedule section of a version-5 blob (module docstring).  No device needed."""
    waits = [w for e in entries for w in e[3]]
    head = struct.pack('<IIII', int(nstreams), int(npre), len(entries), len(waits))
    body = b''.join(struct.pack('<IIII', NO_LAUNCH if idx is None else idx, stream, 1 if record else 0, len(ws))
                    for idx, stream, record, ws in entries)
    return head + body + struct.pack('<%dI' % len(waits), *waits)


def schedule_section(steps, nstreams, npre=0, noop=(), multi_stream=False):
    """-> the schedule section dump_plan writes: b'' (the blob keeps its version) unless the caller asked for the multi-stream
    schedule AND the plan has more than one stream.  No device needed."""
    if not multi_stream or nstreams <= 1:
        return b''
    return pack_schedule(schedule_entries(steps, npre, noop), nstreams, npre)


def plan_version(function_ids, section=b''):
    """The version dump_plan writes: SCHEDULE_VERSION with a schedule section, blob_version otherwise."""
    return SCHEDULE_VERSION if section else blob_version(function_ids)


def dump_plan(model, batch, u8_norm=None, multi_stream=False):
    """-> bytes.  `model`'s plan bound (and autotuned) for `batch`; needs a HIP device (the weight image is read back).
    u8_norm: None for float inputs; a channel_power (as for Executor.bind) for a plan that takes raw uint8 frames and
    normalises them on the GPU (inside the first convolution where the planner could fuse it).
    multi_stream: write the plan's stream schedule too (version 5) when it has more than one stream; False (the default) and
    one-stream plans give the blob of versions 2 - 4, byte for byte."""
    ex = model.executor
    torch = __import__('torch')
    with torch.cuda.device(ex.device), torch.cuda.stream(ex.stream):
        if ex.bound:
            ex.sync_weights()
        bp = ex.bind(batch, u8_norm=u8_norm)
    ex.stream.synchronize()
    # the device half: the bound calls as (entry point, structs, scalars), the three regions, the weight image read back
    lib = _lib.load()
    by_addr = {C.cast(getattr(lib, n), C.c_void_p).value: n for n in ALL_FUNCTIONS}
    reg = _Regions(bp)
    launches = []
    for idx, (fn, args, step) in enumerate(bp.calls):
        if idx in bp.noop_calls:                              # merged into an earlier launch (BoundPlan.group_launches)
            continue
        name = by_addr.get(C.cast(fn, C.c_void_p).value)
        if name is None:
            raise ValueError('step %s (%s) has no serialised form' % (step.kind, step.name))
        nstruct = sum(1 for t in _lib.SIGNATURES[name][1] if _is_struct_ptr(t))     # (the argument structs come first, by reference)
        launches.append((name, [a._obj for a in args[:nstruct]], args[nstruct:]))
    plan = bp.plan
    if bp.u8 is not None:
        inputs = [(bp.u8[id(v.buf)][0].data_ptr(), int(np.prod(v.shape)), 1) for v in plan.inputs]
    else:
        inputs = [(bp.ptr(v), int(np.prod(v.shape)), 0) for v in plan.inputs]
    if any(v.coff % 1 or v.ld < v.C for v in plan.outputs):
        raise ValueError('output view not serialisable')
    outputs = [(bp.ptr(v) - bp.base, v.npix, v.C, v.ld) for v in plan.outputs]

    def image():
        raw = bytearray((reg.size + 255) & ~255)
        for off, t in reg.image:
            b = t.detach().cpu().contiguous().numpy().tobytes()
            raw[off:off + len(b)] = b
        return raw

    section = schedule_section([c[2] for c in bp.calls], plan.nstreams, bp.npre, bp.noop_calls, multi_stream)
    # the pure half
    return pack_plan(bp.n, bp.arena.numel() * 4, inputs, outputs, launches, reg.tag, image, reg.u8_size, section)


CLIP_MAGIC, CLIP_VERSION = b'DHCL', 1


def pack_clip(world, T, Tl, packed_channels, pixels, cut, outputs, frames_blob, head_blob=b''):
    """-> bytes: the clip container (module docstring) around two plan blobs.  cut: [(channel offset, channels)];
    outputs: [(kind, index)] in model order, kind 0 = cut tensor passed through, 1 = head output.  No device needed."""
    align = lambda v: (v + 255) & ~255
    tables = b''.join(struct.pack('<II', int(o), int(c)) for o, c in cut) + \
        b''.join(struct.pack('<II', int(k), int(i)) for k, i in outputs)
    head_size = 4 + struct.calcsize('<IIIIIQIIQQQQ')
    f_off = align(head_size + len(tables))
    h_off = align(f_off + len(frames_blob))
    head = CLIP_MAGIC + struct.pack('<IIIIIQIIQQQQ', CLIP_VERSION, int(world), int(T), int(Tl), int(packed_channels), int(pixels),
                                    len(cut), len(outputs), f_off, len(frames_blob), h_off, len(head_blob))
    body = head + tables
    body += bytes(f_off - len(body)) + frames_blob
    body += bytes(h_off - len(body)) + head_blob
    return body


def dump_clip_plan(sharded, clips, uint8=False, multi_stream=False):
    """-> bytes.  The frame stage and the head stage of `sharded` (a parallel.ShardedClipModel) bound for `clips` clips per
    step, with the cut table, as one clip container.  Needs a HIP device (dump_plan, once per stage).  multi_stream goes to
    both stage plans (dump_plan): a stage whose model has num_streams > 1 is written with its schedule."""
    info = sharded.info
    fm, hm = sharded.frame_model, sharded.head_model
    frames = dump_plan(fm, int(clips), u8_norm=fm.channel_power if uint8 else None, multi_stream=multi_stream)
    head = dump_plan(hm, int(clips), multi_stream=multi_stream) if hm is not None else b''
    pixels = {int(np.prod(shape[:-1])) for (shape, _, _) in info['cut']}
    assert len(pixels) == 1, pixels                          # parallel.split_frames refuses anything else
    outputs = []
    for k in range(len(sharded.model.outputs)):
        if k in info['passthrough']:
            outputs.append((0, info['passthrough'][k]))
        else:
            outputs.append((1, info['head_outputs'].index(k)))
    return pack_clip(sharded.world, info['T'], info['Tl'], info['packed_channels'], pixels.pop(),
                     [(off, c) for (_, off, c) in info['cut']], outputs, frames, head)
