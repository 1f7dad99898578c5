"""Bind a Plan to device memory for a batch size and run it through the C-ABI on one HIP stream.

PyTorch-ROCm is used for exactly three things: the activation arena / weight tensors (device memory),
the stream handle, and host<->device copies.  Every kernel is a libdeephar_hip.so entry point; there is no
torch compute and no CPU fallback.  The launch sequence of a bound plan is captured once into a hipGraph
(dh_graph_*), so steady-state `predict` costs one graph launch per batch instead of ~300 kernel launches.
"""
import ctypes as C
import itertools
import os

import numpy as np

from .. import _lib, frontend
from . import binding, packing, schedule
from .binding import grid_x, grid_depth      # noqa: F401  (their home is the binder; functional.py and the tests look here)

SPLIT_CODES = packing.LAYOUT_CODES['standard']        # Plan.gemm_precision -> dh_conv_args.w_split (packing.LAYOUTS)
WIDE_SPLIT_CODES = packing.LAYOUT_CODES['extended']   # the same under Plan.gemm_scope == 'extended'

BN_EPS = 1e-3  # keras BatchNormalization default epsilon


def _torch():
    import torch
    return torch


class WeightStore:
    """Device copies of the model weights in kernel-ready layout; refreshed in place when Params change."""

    def __init__(self, device):
        self.device = device
        self.conv = {}    # id(param) -> (tensor, Kp, Np, version)
        self.dw = {}      # id(param) -> (tensor, version)
        self.bn = {}      # id(layer) -> (scale, shift, versions)
        self.const = {}   # key -> tensor

    def _dev(self, arr):
        torch = _torch()
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(self.device)

    @staticmethod
    def _require(p):
        if p.value is None:
            raise RuntimeError('weight %s is not set: call model.load_weights(...) or '
                               'deephar_amd.weights.init_synthetic(model) before predict' % p.key)
        return p.value

    def _entry(self, table, key, version, make):
        """table[key] = (device tensors..., further fields..., version): created from make() -> (host arrays, further fields),
        or -- when the version moved -- copied into the tensors already there (pointers stay valid)."""
        ent = table.get(key)
        if ent is None or ent[-1] != version:
            arrays, extra = make()
            if ent is None:
                tensors = tuple(self._dev(a) for a in arrays)
            else:
                tensors = ent[:len(arrays)]
                for t, a in zip(tensors, arrays):
                    t.copy_(self._dev(a))
            ent = table[key] = tensors + tuple(extra) + (version,)
        return ent

    def _packed(self, key, p, pack):
        def make():
            w, kp, np_ = pack(self._require(p))
            return (w,), (kp, np_)
        return self._entry(self.conv, key, p.version, make)[:3]

    def conv_weight(self, p, split=0):
        """split = dh_conv_args.w_split (packing.LAYOUTS): 0 fp32 tap-major, 1 / 3 / 4 the split-bf16 packing with three / two /
        one part, 2 fp32 chunk-major (halo-resident K x K kernel); different packings of one Param are kept side by side when
        several are in use.  5 / 6 / 7 (the extended scope) are the bytes of 1 / 3 / 4 and share their tensor."""
        split = packing.LAYOUTS[int(split)].base
        parts = packing.LAYOUTS[split].parts
        if parts:
            return self._packed((id(p), split), p, lambda w: packing.pack_conv_split(w, parts=parts))
        return self._packed((id(p), split), p, packing.pack_conv_halo if split == 2 else packing.pack_conv)

    CONVT = 'convt'       # packing key of a Conv2DTranspose kernel in `conv` (beside the dh_conv_args.w_split codes)

    def convt_weight(self, p, split=0):
        """Keras Conv2DTranspose kernel [2, 2, Cout, Cin] as the packed [Cin, 4 * Cout] B operand of the depth-to-space
        GEMM (packing.pack_convt); kept in `conv` like every packed GEMM weight.  split = 0: fp32; 1 / 3 / 4 (the codes of
        dh_conv_args.w_split): the split-bf16 packing with three / two / one part, kept beside the fp32 one."""
        key = (id(p), self.CONVT if not split else (self.CONVT, int(split)))
        return self._packed(key, p, lambda w: packing.pack_convt(w, parts=packing.LAYOUTS[int(split)].parts))

    def dw_weight(self, p):
        def flat():
            w = self._require(p)
            return (np.ascontiguousarray(w.reshape(w.shape[0] * w.shape[1], w.shape[2])),), ()
        return self._entry(self.dw, id(p), p.version, flat)[0]

    def _bn_host(self, layer):
        byrole = {p.role: self._require(p) for p in layer.params}
        inv = (np.float32(1.0) / np.sqrt(byrole['var'].astype(np.float32) + np.float32(BN_EPS))).astype(np.float32)
        if 'gamma' in byrole:
            inv = (inv * byrole['gamma']).astype(np.float32)
        return inv, (byrole['beta'] - byrole['mean'] * inv).astype(np.float32)

    def bn_affine(self, layer):
        """BatchNormalization inference as y = x*scale + shift (fp32, like tf.nn.batch_normalization).  A
        planner.ConcatAffine (the affine behind a horizontally merged convolution, rule R10c) gives the per-column scale /
        shift of its parts side by side, identity (1, 0) for a part without a BatchNormalization."""
        def host():
            if not hasattr(layer, 'parts'):
                return self._bn_host(layer), ()
            pieces = [self._bn_host(l) if l is not None else (np.ones(c, np.float32), np.zeros(c, np.float32))
                      for c, l in layer.parts]
            return (np.concatenate([a for a, _ in pieces]).astype(np.float32),
                    np.concatenate([b for _, b in pieces]).astype(np.float32)), ()
        return self._entry(self.bn, id(layer), tuple(p.version for p in layer.params), host)[:2]

    def constant(self, key, make):
        t = self.const.get(key)
        if t is None:
            t = self._dev(make())
            self.const[key] = t
        return t


def normalization_lut(channels, channel_power=1):
    """utils/transform.normalize_channels (transform.py:212-231) tabulated for every byte value, per channel:
    the reference runs it in float32 in place (T.asarray() yields float32, transform.py:122-124), so the same
    NumPy float32 operations on 0..255 give bit-identical values.  Returns float32 [channels, 256]."""
    powers = [channel_power] * channels if isinstance(channel_power, int) else list(channel_power)
    if len(powers) != channels:
        raise ValueError('channel_power expected to be int or a list with one entry per channel')
    lut = np.empty((channels, 256), np.float32)
    for c, pw in enumerate(powers):
        v = np.arange(256, dtype=np.float32)
        v /= 255.
        if pw != 1:
            v = np.power(v, pw)
        v -= .5
        v *= 2.
        lut[c] = v
    return lut


class _InputStep:
    """Pseudo-step for the stand-alone uint8 normalisation launch (first on stream 0, nothing to wait for)."""
    kind, name, stream, wait, record, deps, params = 'normalize_u8', 'input', 0, (), False, (), {}

    def __init__(self, v):
        self.outs = {'y': v}
        self.ins = {}
        self.attrs = {}

    def flops(self, n):
        return 0

    def bytes(self, n):
        v = self.outs['y']
        return 5 * n * int(np.prod(v.shape))


from .planner import split_k_rule      # noqa: E402  (the rule is stated once, next to the planner rule that uses it)


def value_view(flat, v, n):
    """torch view [n, *shape] of a Value (strided when it lives inside a wider buffer) in `flat`: the arena of a plan bound at n,
    or a copy of its head (OutputRing: the packed output region arena[0 : out_items * n])."""
    shape = (n,) + v.shape
    strides = [1] * len(shape)
    if len(shape) >= 2:
        strides[-2] = v.ld
        for i in range(len(shape) - 3, -1, -1):
            strides[i] = strides[i + 1] * shape[i + 1]
    return _torch().as_strided(flat, shape, strides, v.buf.offset * n + v.coff)


class BoundPlan:
    """A Plan with concrete device pointers for batch size n."""

    def __init__(self, plan, n, store, device, u8_norm=None):
        torch = _torch()
        self.plan, self.n, self.store, self.device = plan, n, store, device
        self.lib = _lib.load()
        self.arena = torch.empty(max(plan.arena_items * n, 4), dtype=torch.float32, device=device)
        self.base = self.arena.data_ptr()
        self.calls = []       # (fn, args tuple without stream, step)
        self._keep = []       # ctypes structs kept alive
        self.graph = None
        # test hook (schedule stress tests): perturb(call index, step, stream of the step, [all streams]), once per call in order,
        # no later than the call's launch / record (schedule.run_program: before) -- e.g. dh_stream_spin_us delays on one stream
        self.perturb = None
        # uint8 frames: every model input gets a byte staging buffer; convolutions that read an input directly
        # normalise on load (dh_conv_args.x_u8), anything else is fed by a stand-alone normalisation launch
        self.u8 = None
        self.npre = 0         # launches in front of plan.steps[0] (step indices in `wait` lists are offset by it)
        if u8_norm is not None:
            self.u8 = {}
            for v in plan.inputs:
                lut = store.constant(('u8lut', v.C, repr(u8_norm)), lambda v=v: normalization_lut(v.C, u8_norm))
                buf = torch.zeros((n,) + v.shape, dtype=torch.uint8, device=device)
                users = [s for s in plan.steps for w in s.ins.values() if w is not None and w.buf is v.buf]
                fused = all(s.kind == 'conv' and s.ins['x'].buf is v.buf and s.ins['x'].C == v.C and
                            s.ins['x'].coff == v.coff and v.C % 4 != 0 and 'pre_bn' not in s.params and
                            s.ins.get('res1') is None and s.ins.get('res2') is None for s in users)
                self.u8[id(v.buf)] = (buf, lut, fused)
                if not fused:
                    self.calls.append((self.lib.dh_normalize_u8_f32,
                                       (buf.data_ptr(), lut.data_ptr(), self.ptr(v), n * int(np.prod(v.shape[:-1])),
                                        v.C), _InputStep(v)))
                    self.npre += 1
        for step in plan.steps:
            self._bind(step)
        self.grouped = 0      # pairs of launches merged into one (group_launches: latency regime only)
        self.noop_calls = set()   # indices of `calls` whose work moved into an earlier, grouped launch
        self.paired = []          # (index of the paired launch, index of the launch it absorbed): _pair_skinny_convs
        self.absorbed = {}        # index of a grouped / paired launch -> the Step whose work it also does
        # what the Executor's chunk loops keep per bound plan, across calls: all of it only grows (pinned allocation costs
        # milliseconds, and a warm second call must allocate nothing)
        self.ring = OutputRing(plan, n, self.arena)   # pinned slots for the packed outputs
        self.h2d = []             # per slot: the event that orders the slot's upload (copy stream) before the compute stream
        self.array_slots = []     # ArrayFeed: per slot (pinned staging per input, their device twins)
        self.byte_slots = []      # frontend.CropFeed: per slot (pinned uint8, device uint8): a crop program or a job table
        # the ONE device crop program of this plan (Executor.crop_room / crop_step).  One buffer is enough for every slot and
        # every loop: its only reader is the crop launch right behind the builder on the compute stream, and the next builder is
        # enqueued on that stream behind the forward's join -- what run_refine, run_frame_boxes and plan.hip (pl->crop_prog) rely on
        self.crop_prog = None
        self.boxes_host = None    # run_frame_boxes: the pinned result tables
        self.votes_host = None    # run_votes: the pinned result tables

    # ---- views -------------------------------------------------------------------------------------------
    def ptr(self, v):
        return self.base + 4 * (v.buf.offset * self.n + v.coff)

    def tensor(self, v):
        """torch view [n, *shape] of a Value (strided when it lives inside a wider buffer)."""
        return value_view(self.arena, v, self.n)

    def input_bytes(self):
        """The uint8 staging tensor [n, ...] of the first input of a uint8-bound plan: what a crop launch fills."""
        return self.u8[id(self.plan.inputs[0].buf)][0]

    # ---- binding: the env of engine/binding.py over the arena and the WeightStore, and the part that needs a device ----------
    def affine(self, layer):
        sc, sh = self.store.bn_affine(layer)
        return sc.data_ptr(), sh.data_ptr()

    def constant(self, key, make):
        return self.store.constant(key, make).data_ptr()

    def dw_weight(self, p):
        return self.store.dw_weight(p).data_ptr()

    def u8_input(self, buf):
        ent = (self.u8 or {}).get(id(buf))
        return (ent[0].data_ptr(), ent[1].data_ptr()) if ent is not None and ent[2] else None

    def _bind(self, s):
        """binding.bind fills the launch; here the library picks the weight's packing and the store supplies it."""
        name, structs, scalars = binding.bind(s, self.n, self)
        if s.kind in ('conv', 'convtranspose'):
            args = structs[0]                          # every field but w / w_split is final here
            if s.kind == 'conv':
                s.attrs['x_u8'] = int(args.x_u8)       # (read by bench.py to name the kernel)
                split = binding.weight_layout(self.lib, self.plan, args)
                wt, kp, np_ = self.store.conv_weight(s.params['w'], split=split)
                args.w_split = int(split)
            else:
                split = binding.convt_weight_layout(self.lib, self.plan, args)
                wt, kp, np_ = self.store.convt_weight(s.params['w'], split=split)
                if split:
                    name, scalars = 'dh_conv2d_transpose2x2_split_f32', [packing.SPLIT_PARTS[split]] + scalars
            assert (kp, np_) == (args.Kp, args.Np)
            args.w = wt.data_ptr()
            s.attrs['w_split'] = int(split)            # (read by bench.py to name the kernel; convtranspose: 0 = the fp32 kernel)
        self._keep.extend(structs)
        self.calls.append((getattr(self.lib, name), tuple(C.byref(st) for st in structs) + tuple(scalars), s))

    # ---- execution -----------------------------------------------------------------------------------------
    _streams = _program = _sync = None      # made on first use: side streams | (ops, number of events) | the sync events by id

    def _side_streams(self, main_ptr=None):
        """The extra HIP streams for the parallel branches of the plan.  [r06] They are the engine's role streams other than
        the one this plan is launched on (shared_stream below: every stream the package creates costs one of ROCm's four hardware
        queues, and a side stream that shares a queue with its plan's main stream is slow); only a plan with more branches than
        those creates streams of its own."""
        if self._streams is None:
            roles = [shared_stream(self.device, r) for r in ('head', 'comm', 'copy')] if self.plan.nstreams > 1 else []
            spare = [st for st in roles if main_ptr is None or st.cuda_stream != main_ptr]
            self._streams = [C.c_void_p(st.cuda_stream) for st in spare[:self.plan.nstreams - 1]]
            while len(self._streams) < self.plan.nstreams - 1:
                self._streams.append(C.c_void_p())
                _lib.check(self.lib.dh_stream_create(C.byref(self._streams[-1])), 'stream create')
        return self._streams

    def program(self):
        """-> (ops, number of events) of `calls`, from the scheduler dh_forward runs too (csrc/plan_sched.h); built on first use"""
        if self._program is None:
            entries = schedule.schedule_entries([c[2] for c in self.calls], self.npre, self.noop_calls)
            self._program = _lib.sched_program(self.lib, entries, self.plan.nstreams, self.npre)
        return self._program

    def launch_all(self, stream_ptr):
        """Enqueue the whole plan: walk program() with `stream_ptr` as stream 0.  One stream: the launches in order.  Several:
        steps go to their scheduled stream, cross-stream dependencies are event waits, and the side streams fork from / join
        back into `stream_ptr` (so the sequence is capturable into one hipGraph)."""
        lib, calls, (ops, nevents) = self.lib, self.calls, self.program()
        ptrs = [stream_ptr] + self._side_streams(stream_ptr)
        if self._sync is None and len(ptrs) > 1:
            self._sync = [C.c_void_p() for _ in range(nevents)]
            for ev in self._sync:
                _lib.check(lib.dh_event_create_sync(C.byref(ev)), 'event create')
        sync = self._sync
        def launch(i, s):
            fn, args, step = calls[i]                  # (looked up now: bench.py assigns into `calls` after binding)
            rc = fn(*args, ptrs[s])
            if rc != 0:
                _lib.check(rc, 'step %s (%s)' % (step.kind, step.name))

        record = lambda ev, s: _lib.check(lib.dh_event_record(sync[ev], ptrs[s]), 'event record')
        wait = lambda ev, s: _lib.check(lib.dh_stream_wait_event(ptrs[s], sync[ev]), 'event wait')
        before = self.perturb and (lambda i: self.perturb(i, calls[i][2], ptrs[calls[i][2].stream], ptrs))
        schedule.run_program(ops, launch, record, wait, before, len(calls))

    # ---- grouped launches (latency regime) ------------------------------------------------------------------------
    GROUP_MAX_ROWS = 8192           # conv rows (pixels of the bound batch) up to which a pair is merged
    GROUP_MAX_DW_ELEMS = 1 << 23    # ... and depthwise elements

    def group_launches(self, stream_ptr):
        """[r06] Merge every (1x1 shortcut convolution, depthwise convolution) pair of a pre-activation residual unit that is
        launched back to back on one stream, reads the same tensor and is small enough to be bound by the cost of a node
        rather than by its work into ONE launch (dh_conv2d_dw_group_f32: bit-identical, the work-groups of one grid run
        either kernel's code).  The depthwise entry of `calls` stays as a no-op so that step indices (event waits, per-step
        profiles) keep their meaning.  Switch: plan.rules.group_launches.  Returns the number of pairs merged."""
        if not self.plan.rules.group_launches or self.grouped or self.paired:
            return self.grouped
        lib = self.lib
        for i in range(self.npre, len(self.calls) - 1):
            fc, ac, sc = self.calls[i]
            # the next launch ON THE SAME STREAM (a multi-stream plan interleaves the streams in launch order): the pair is
            # consecutive there, so running the depthwise conv at the shortcut's place moves it past nothing it is ordered
            # with -- it waits for no event of its own (checked), and what it writes was planned to be free from here on
            j = next((k for k in range(i + 1, len(self.calls)) if self.calls[k][2].stream == sc.stream), None)
            if j is None:
                continue
            fd, ad, sd = self.calls[j]
            if sc.kind != 'conv' or sd.kind != 'dwconv' or sd.wait or i in self.noop_calls or fc is lib.dh_conv2d_dw_group_f32:
                continue
            if fd is not lib.dh_dwconv2d_f32:          # (a strided depthwise step has its own entry point and no grouped form)
                continue
            # which pairs: the two halves of one unit, both reading its input.  Whether they may run as one grid is the pair
            # path's test: neither reads or overwrites what the other writes (the memory plan re-uses space: the depthwise
            # result must not lie over the convolution's residuals either)
            if sc.ins['x'].buf is not sd.ins['x'].buf or not self._independent(sc, sd):
                continue
            ca, da = ac[0]._obj, ad[0]._obj
            if ca.N * ca.OH * ca.OW > self.GROUP_MAX_ROWS or da.N * da.H * da.W * da.C > self.GROUP_MAX_DW_ELEMS:
                continue
            if lib.dh_conv2d_dw_group_f32(ac[0], ad[0], stream_ptr) != 0:      # (a real launch: the pair's own outputs)
                continue
            sc.attrs['grouped'] = True                 # (for bench.py's kernel names: the plan's steps are shared by every batch
            self._absorb(i, j, lib.dh_conv2d_dw_group_f32)     # size it is bound to -- `calls` / `noop_calls` count for execution)
            self.grouped += 1
        self._pair_skinny_convs(stream_ptr)
        if self.grouped or self.paired:
            self._drop_graph()
            self._program = None                       # noop_calls changed
        return self.grouped

    def _absorb(self, i, k, fn):
        """Launch i becomes the two-struct launch `fn` over its own and launch k's arguments; k stays as a no-op."""
        (_, ai, si), (_, ak, sk) = self.calls[i], self.calls[k]
        self.calls[i] = (fn, (ai[0], ak[0]), si)
        self.calls[k] = (_noop_launch, (), sk)
        self.noop_calls.add(k)
        self.absorbed[i] = sk

    PAIR_LOOKAHEAD = 3              # launches of the same stream a partner may be pulled forward past

    @staticmethod
    def _values_overlap(v, w):
        """May the two views touch the same floats?  Same buffer: unless they are disjoint channel runs of one pitch;
        different buffers: if their arena ranges meet (the memory plan re-uses space)."""
        if v is None or w is None:
            return False
        if v.buf is w.buf:
            return not (v.ld == w.ld and (v.coff + v.C <= w.coff or w.coff + w.C <= v.coff))
        a, b = v.buf, w.buf
        return not (a.offset + a.items <= b.offset or b.offset + b.items <= a.offset)

    @classmethod
    def _independent(cls, s, t):
        """neither step reads or overwrites what the other writes"""
        for o in s.outs.values():
            if any(cls._values_overlap(o, v) for v in list(t.ins.values()) + list(t.outs.values())):
                return False
        for o in t.outs.values():
            if any(cls._values_overlap(o, v) for v in s.ins.values()):
                return False
        return True

    def _pair_skinny_convs(self, stream_ptr):
        """[r06] Two independent convolutions of the skinny-conv kernel that follow each other on one stream -- the residual unit
        on the action head's pose features beside `v_conv0` on its appearance features (spnet.py:113-133), the pointwise half of
        the separable unit on the previous head's features beside this head's conv2 -- become ONE launch (dh_conv2d_pair_f32:
        work-groups of one grid run either convolution's own code: bit-identical).  The partner is the next launch of the same
        stream, or one up to PAIR_LOOKAHEAD launches further down that is independent of everything it is pulled past; it must
        wait for no event itself and pass no launch that does (an event a launch waits for may be the one that orders the
        partner's inputs too).  Switch: plan.rules.pair_convs."""
        if not self.plan.rules.pair_convs:
            return
        lib = self.lib

        def skinny(k):
            fn, args, st = self.calls[k]
            if fn is not lib.dh_conv2d_f32 or k in self.noop_calls or st.kind != 'conv':
                return False
            ca = args[0]._obj                          # (the latency regime only, like the conv + depthwise groups)
            return not ca.x_resample and ca.N * ca.OH * ca.OW <= self.GROUP_MAX_ROWS and lib.dh_conv2d_uses_split_k(args[0]) == 1

        i = self.npre
        while i < len(self.calls) - 1:
            if not skinny(i):
                i += 1
                continue
            fa, aa, sa = self.calls[i]
            passed, npassed = [], 0
            for k in range(i + 1, len(self.calls)):
                fk, ak, sk = self.calls[k]
                if sk.stream != sa.stream or k in self.noop_calls:
                    continue                           # (a no-op's work runs where its group / pair is: see `absorbed` below)
                if sk.wait or npassed > self.PAIR_LOOKAHEAD:
                    break
                if skinny(k) and self._independent(sa, sk) and all(self._independent(q, sk) for q in passed) and \
                        lib.dh_conv2d_pair_f32(aa[0], ak[0], stream_ptr) == 0:
                    self._absorb(i, k, lib.dh_conv2d_pair_f32)
                    self.paired.append((i, k))
                    break
                passed.append(sk)
                npassed += 1
                if k in self.absorbed:                 # a grouped / paired launch does a second step's work at this place
                    passed.append(self.absorbed[k])
            i += 1

    def capture(self, stream_ptr):
        """Capture the launch sequence into a hipGraph.  -> False (nothing captured; the caller launches eagerly) when
        this is a multi-stream plan and the process already holds MAX_MULTISTREAM_GRAPHS such graph execs: they can only
        be parked, never destroyed (__del__), so their number is what bounds the leak of a long-lived multi-model process."""
        global _MULTISTREAM_GRAPHS
        lib = self.lib
        if self.plan.nstreams > 1:
            if _MULTISTREAM_GRAPHS >= MAX_MULTISTREAM_GRAPHS:
                return False
        _lib.check(lib.dh_graph_begin_capture(stream_ptr), 'graph capture begin')
        try:
            self.launch_all(stream_ptr)
        finally:
            g = C.c_void_p()
            rc = lib.dh_graph_end_capture(stream_ptr, C.byref(g))
        _lib.check(rc, 'graph capture end')
        self.graph = g
        if self.plan.nstreams > 1:
            _MULTISTREAM_GRAPHS += 1      # counted only once a graph exec exists (a failed capture holds no slot: ADVICE r04)
        return True

    def replay(self, stream_ptr):
        _lib.check(self.lib.dh_graph_launch(self.graph, stream_ptr), 'graph launch')

    # ---- autotuning of the conv tiling -------------------------------------------------------------------
    def autotune(self, stream_ptr, table=None, reps=3):
        """Time every tile configuration of dh_conv2d_f32 for each distinct conv shape of this bound plan
        (HIP events on the launch stream) and keep the fastest.  All configurations sum K in the same order,
        so the choice never changes a result bit.  `table` (signature -> cfg) is filled / reused."""
        lib = self.lib
        table = {} if table is None else table
        ncfgs = {'conv': lib.dh_conv2d_num_tile_cfgs()}
        e0, e1 = C.c_void_p(), C.c_void_p()
        _lib.check(lib.dh_event_create(C.byref(e0)))
        _lib.check(lib.dh_event_create(C.byref(e1)))
        for i, (fn, args, step) in enumerate(self.calls):
            if step.kind not in ncfgs:
                continue
            if fn is lib.dh_conv2d_seg_f32:                      # (skinny-conv kernel by its own entry point: nothing to choose)
                step.attrs['tile_cfg'] = -1
                step.attrs['split_k'] = True
                continue
            ncfg = ncfgs[step.kind]
            cargs = args[0]._obj
            sig = (self.n, step.kind) + binding.conv_signature(step) + ((('u8',) if cargs.x_u8 else ())) + \
                (((packing.LAYOUT_MODE[cargs.w_split],) if cargs.w_split else ()))
            if cargs.w_split:
                ncfg = lib.dh_conv2d_num_halo_tile_cfgs() if cargs.w_split == 2 else lib.dh_conv2d_num_split_tile_cfgs()
            if step.kind == 'conv' and lib.dh_conv2d_uses_split_k(args[0]):
                step.attrs['tile_cfg'] = -1                      # shape rule: split-K kernel, no tilings to choose from
                step.attrs['split_k'] = True
                self.calls[i] = (fn, (args[0], -1), step)
                continue
            if step.kind == 'conv' and lib.dh_conv2d_uses_first_layer_kernel(args[0]):
                step.attrs['tile_cfg'] = -1                      # shape rule: first-layer kernel (conv_stem.hip)
                step.attrs['first_layer'] = True
                self.calls[i] = (fn, (args[0], -1), step)
                continue
            shape_key = ('shape', int(cargs.w_split), self.n, cargs.N * cargs.OH * cargs.OW, cargs.K, cargs.Cout, cargs.KH,
                         cargs.KW, cargs.up2)
            if sig not in table:
                def time_cfg(cfg, nrep, trials):
                    t_cfg = float('inf')
                    for _trial in range(trials):         # best of several trials: one noisy sample must not pick the tiling
                        _lib.check(lib.dh_event_record(e0, stream_ptr))
                        for _ in range(nrep):
                            fn(args[0], cfg, stream_ptr)
                        _lib.check(lib.dh_event_record(e1, stream_ptr))
                        _lib.check(lib.dh_event_synchronize(e1))
                        ms = C.c_float()
                        _lib.check(lib.dh_event_elapsed_ms(e0, e1, C.byref(ms)))
                        t_cfg = min(t_cfg, ms.value / nrep)
                    return t_cfg
                timed = {}
                for cfg in range(ncfg):
                    if fn(args[0], cfg, stream_ptr) != 0:     # unsupported combination (warm-up launch)
                        continue
                    timed[cfg] = time_cfg(cfg, reps, 2)
                best = -1
                if timed:
                    lo = min(timed.values())
                    # candidates within 8 % of the fastest are timed again, longer: a 3-4 % difference between two
                    # tilings of the dominant GEMM is worth more than the first pass can resolve
                    close = [c for c, t in timed.items() if t <= 1.08 * lo]
                    if len(close) > 1:
                        for c in close:
                            timed[c] = time_cfg(c, 4 * reps, 3)
                        best = min(close, key=lambda c: timed[c])
                        # tilings within 1 % of each other are the same speed as far as this timing can tell: the same
                        # GEMM (M x K x N, taps) under another epilogue signature keeps the tiling chosen first, so one
                        # layer family runs ONE instantiation (per-kernel profiles stay readable, PMC look-ups hit)
                        pref = table.get(shape_key)
                        if pref in close and timed[pref] <= 1.01 * timed[best]:
                            best = pref
                    else:
                        best = close[0]
                table[sig] = best
                table.setdefault(shape_key, best)
            step.attrs['tile_cfg'] = table[sig]
            self.calls[i] = (fn, (args[0], table[sig]), step)
        lib.dh_event_destroy(e0)
        lib.dh_event_destroy(e1)
        self._drop_graph()
        return table

    def profile(self, stream_ptr, reps=1):
        """Per-step device time (ms, mean over reps) with HIP events recorded on the launch stream."""
        lib = self.lib
        evs = []
        for _ in range(len(self.calls) + 1):
            e = C.c_void_p()
            _lib.check(lib.dh_event_create(C.byref(e)))
            evs.append(e)
        times = np.zeros(len(self.calls))
        for _ in range(reps):
            _lib.check(lib.dh_event_record(evs[0], stream_ptr))
            for i, (fn, args, step) in enumerate(self.calls):
                _lib.check(fn(*args, stream_ptr), step.kind)
                _lib.check(lib.dh_event_record(evs[i + 1], stream_ptr))
            _lib.check(lib.dh_event_synchronize(evs[-1]))
            for i in range(len(self.calls)):
                ms = C.c_float()
                _lib.check(lib.dh_event_elapsed_ms(evs[i], evs[i + 1], C.byref(ms)))
                times[i] += ms.value
        for e in evs:
            lib.dh_event_destroy(e)
        return times / reps

    def _drop_graph(self):
        # ROCm 7.2: hipGraphExecDestroy of a graph captured across several streams (event fork/join nodes) leaves
        # the runtime in a state where a LATER capture + launch of another multi-stream graph segfaults
        # (tools/repro_seg.py: two bound plans of one model destroyed, next model's first replay crashes; the
        # same sequence with one stream, or without the destroy, is fine).  Multi-stream graph execs are therefore
        # parked until process exit instead of destroyed -- a few KB of kernel-node parameters each.
        if self.graph is not None:
            if self.plan.nstreams > 1:
                _GRAPH_GRAVEYARD.append(self.graph)
            else:
                self.lib.dh_graph_destroy(self.graph)
            self.graph = None

    def __del__(self):
        try:
            self._drop_graph()
        except Exception:
            pass


def _noop_launch(*_args):
    """Placeholder of a launch that was merged into the one before it (BoundPlan.group_launches)."""
    return 0


_GRAPH_GRAVEYARD = []
# multi-stream graph execs ever created by this process (live + parked): capped, see BoundPlan.capture.  One-stream
# plans (the default, Model.num_streams = 1) destroy their graphs and are not counted.
_MULTISTREAM_GRAPHS = 0
MAX_MULTISTREAM_GRAPHS = max(0, int(os.environ.get('DEEPHAR_MAX_MULTISTREAM_GRAPHS', '64')))
# ---- the package's HIP streams, one per ROLE and device ----------------------------------------------------------------
# ROCm maps every HIP stream onto one of GPU_MAX_HW_QUEUES (default 4) hardware queues when it is created.  Until round 6 every
# Model owned a compute stream, every predict() a copy stream, every frame-sharded clip model a collective stream: the fourth
# or fifth stream of a process landed on a hardware queue another one already used, and two streams that order each other with
# events through ONE hardware queue cost the frame-sharded SPNet / merge models 4.7 % of their step (22.0 -> 23.0 ms, 7.85 ->
# 8.24 ms) -- in any process that had called Model.predict on another model before (profiles/r06_hw_queue_collision.md).
# Now: ONE stream per role -- 'compute' (every Model's launches; models of a process run one after the other anyway), 'copy'
# (predict's host-device staging), 'head' (the head stage of a frame-sharded clip model), 'comm' (its collective) -- four
# streams, four hardware queues, whatever the process did before.
_ROLE_STREAMS = {}
_ROLE_LOCKS = {}        # (device index, role) -> RLock: the models of a process share a stream, so ONE thread at a time enqueues on it
                        # (a hipGraph capture on the stream would otherwise swallow another thread's launches)


def stream_lock(device, role):
    import threading
    torch = _torch()
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), role)
    lk = _ROLE_LOCKS.get(key)
    if lk is None:
        lk = _ROLE_LOCKS.setdefault(key, threading.RLock())
    return lk


def shared_stream(device, role):
    torch = _torch()
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), role)
    st = _ROLE_STREAMS.get(key)
    if st is None:
        with torch.cuda.device(device):
            for r in ('compute', 'copy', 'head', 'comm'):           # a fixed creation order: the mapping does not depend on
                k = (key[0], r)                                      # which role a process happens to need first
                if k not in _ROLE_STREAMS:
                    _ROLE_STREAMS[k] = torch.cuda.Stream(device=device)
        st = _ROLE_STREAMS.get(key)
        if st is None:
            with torch.cuda.device(device):
                st = _ROLE_STREAMS[key] = torch.cuda.Stream(device=device)
    return st


_STAGING_THREADS = max(1, min(8, (os.cpu_count() or 2) // 2, int(os.environ.get('DEEPHAR_STAGING_THREADS', '6'))))
_POOL = None


def _staging_pool():
    """Threads that copy / cast host arrays into pinned staging for Model.predict (run_pipelined); orchestration only."""
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=_STAGING_THREADS, thread_name_prefix='deephar-staging')
    return _POOL


# ---- the chunk loops of the Executor: their arithmetic, their output ring, the host-array feed ----------------------------------
def chunk_steps(total, bs, depth, passes=1):
    """The chunk-steps of `passes` passes over rows 0 .. total - 1 in chunks of `bs`, on a ring of `depth` slots, pass-major:
    yields (step, pass t, chunk ci, slot = step % depth, start = ci * bs, m = min(bs, total - start)).  GPU-free."""
    nchunks = -(-total // bs)
    for step in range(passes * nchunks):
        t, ci = divmod(step, nchunks)
        yield step, t, ci, step % depth, ci * bs, min(bs, total - ci * bs)


def ring_depth(steps, slot_bytes=0):
    """Slots for `steps` chunk-steps: one per step, at most DEEPHAR_PREDICT_DEPTH (8) and -- where every slot stages
    `slot_bytes` of input in pinned memory -- at most 512 MB of staging per bound plan; never fewer than 2.  GPU-free."""
    cap = max(2, (512 << 20) // slot_bytes) if slot_bytes else steps
    return max(2, min(steps, int(os.environ.get('DEEPHAR_PREDICT_DEPTH', '8')), cap))


class OutputRing:
    """Per bound plan: slots of pinned host memory for the packed outputs of a forward (arena[0 : out_items * n]), the event
    behind each slot's D2H and the rows pending in it.  The chunk loops submit a slot behind every forward and reclaim it --
    the one host wait -- only when they need the slot again or drain."""

    def __init__(self, plan, n, arena):
        self.plan, self.n, self.arena = plan, n, arena
        self.host, self.done, self.pending = [], [], []

    def grow(self, depth):
        torch = _torch()
        while len(self.host) < depth:
            self.host.append(torch.empty(max(self.plan.out_items * self.n, 4), dtype=torch.float32, pin_memory=True))
            self.done.append(torch.cuda.Event())
            self.pending.append(None)

    def submit(self, slot, m, stream):
        """Behind a forward of m rows on `stream`: ONE D2H of the packed outputs of the whole model into the slot."""
        self.host[slot].copy_(self.arena[:self.host[slot].numel()], non_blocking=True)
        self.done[slot].record(stream)
        self.pending[slot] = m

    def reclaim(self, slot, results, only=None):
        """If the slot holds rows: wait for its D2H and append to `results` one fresh array per output (a list), or the
        array of output `only` alone, sliced out of the packed region."""
        m = self.pending[slot]
        if m is not None:
            self.done[slot].synchronize()
            outs = self.plan.outputs
            fresh = [np.array(value_view(self.host[slot], v, self.n)[:m].numpy(), dtype=np.float32, copy=True, order='C')
                     for v in (outs if only is None else [outs[only]])]
            results.append(fresh if only is None else fresh[0])
            self.pending[slot] = None

    def drain(self, step, depth, results, only=None):
        """Reclaim every slot of a ring of `depth` whose next chunk-step would be `step`: the oldest pending one first."""
        for k in range(depth):
            self.reclaim((step + k) % depth, results, only)

    def abandon(self, stream):
        """A call that died mid-loop must not leak rows into the next one: wait for whatever is in flight, forget it."""
        if any(p is not None for p in self.pending):
            stream.synchronize()
            self.pending = [None] * len(self.pending)


class ArrayFeed:
    """Executor.run_pipelined's feed of host arrays (equal leading dim; an array may also be a device tensor).  Per slot:
    pinned host staging in the dtype that crosses PCIe (uint8 frames or float32 -- float64 loader arrays are cast on the HOST
    while being copied into the pinned buffer) and its device twin.
    A feed is driven through three calls per chunk: stage_chunk (start the host-side staging into a slot on the pool, return the
    futures), upload (enqueue the slot's upload; the copy stream is current), fill (enqueue what fills the plan's input; the
    compute stream is current) -- after slot_bytes (what a slot pins, for ring_depth) and open (the slots, grown only)."""

    def __init__(self, plan, arrays):
        self.plan, self.arrays, self.total = plan, arrays, arrays[0].shape[0]

    def slot_bytes(self, bs, u8):
        return sum(bs * int(np.prod(v.shape)) for v in self.plan.inputs) * (1 if u8 else 4)

    def open(self, ex, bp, bs, depth):
        torch = _torch()
        self.bp, self.want, self.dev_src = bp, torch.uint8 if bp.u8 is not None else torch.float32, {}

        def alloc(**where):
            return [torch.empty((bp.n,) + v.shape, dtype=self.want, **where) for v in self.plan.inputs]
        while len(bp.array_slots) < depth:
            bp.array_slots.append((alloc(pin_memory=True), alloc(device=ex.device)))

    def stage_chunk(self, pool, slot, start, m):
        torch = _torch()
        dev_src, futs = [], []
        for k, (v, arr) in enumerate(zip(self.plan.inputs, self.arrays)):
            part = arr[start:start + m]
            if tuple(part.shape[1:]) != tuple(v.shape):
                raise ValueError('input has shape %s, model expects [N, %s]' % (tuple(arr.shape), tuple(v.shape)))
            src = torch.from_numpy(np.ascontiguousarray(part)) if isinstance(part, np.ndarray) else part
            if (src.dtype == torch.uint8) != (self.want == torch.uint8):
                raise ValueError('plan bound for %s inputs, got %s' % (self.want, src.dtype))
            dev_src.append(src if src.is_cuda else None)
            if not src.is_cuda:                         # host-side cast (f64 -> f32) + pin, row slices in parallel
                dst = self.bp.array_slots[slot][0][k]
                nsl = max(1, min(_STAGING_THREADS, src.numel() * src.element_size() >> 22, m))
                step = -(-m // nsl)
                for a0 in range(0, m, step):
                    a1 = min(a0 + step, m)              # a ragged last chunk: both slices stop at m
                    futs.append(pool.submit(dst[a0:a1].copy_, src[a0:a1]))
        self.dev_src[slot] = dev_src                    # (until the slot's upload: a slot is staged again only behind it)
        return futs

    def upload(self, slot, m, staged, copy_stream):
        host, dev = self.bp.array_slots[slot]
        dev_src = self.dev_src.pop(slot)
        if any(s is not None for s in dev_src):         # the caller's device data may still be in flight on ITS stream
            copy_stream.wait_stream(_torch().cuda.current_stream())
        for k, s in enumerate(dev_src):
            dev[k][:m].copy_(host[k][:m] if s is None else s, non_blocking=True)

    def fill(self, slot, m):
        for k, v in enumerate(self.plan.inputs):
            dst = self.bp.u8[id(v.buf)][0] if self.bp.u8 is not None else self.bp.tensor(v)
            dst[:m].copy_(self.bp.array_slots[slot][1][k][:m], non_blocking=True)


class Executor:
    def __init__(self, plan, device=None, use_graph=True, autotune=True, stream_role='compute'):
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.DeepharHipError('no HIP device visible: deephar_amd runs only on an AMD GPU (gfx950); '
                                       'there is no CPU execution path')
        _lib.load()
        self.device = torch.device(device or 'cuda:%d' % torch.cuda.current_device())
        self.plan = plan
        self.use_graph = use_graph
        self.autotune = autotune
        self.tune_table = {}
        self.store = WeightStore(self.device)
        self.bound = {}            # key -> BoundPlan, most recently used last; at most `max_bound` are kept
        self.max_bound = max(1, int(os.environ.get('DEEPHAR_MAX_BOUND_PLANS', '4')))
        self._wstamp = None        # sum of Param.version over plan.params at the last refresh / first bind
        self.stream = shared_stream(self.device, stream_role)
        self._lock = stream_lock(self.device, stream_role)

    @property
    def stream_ptr(self):
        return self.stream.cuda_stream

    def bind(self, n, u8_norm=None):
        with self._lock:          # one thread at a time on the shared stream (engine/executor.py: stream_lock)
            return self._bind_locked(n, u8_norm)

    def _bind_locked(self, n, u8_norm=None):
        """u8_norm: None for float inputs; a channel_power (1 or a per-channel list) when the inputs are raw uint8
        frames to be normalised on the GPU like utils/transform.normalize_channels."""
        key = n if u8_norm is None else (n, repr(u8_norm))
        bp = self.bound.get(key)
        if bp is None:
            torch = _torch()
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                bp = BoundPlan(self.plan, n, self.store, self.device, u8_norm=u8_norm)
                if self.autotune:
                    bp.autotune(self.stream_ptr, self.tune_table)
                bp.group_launches(self.stream_ptr)
            self.bound[key] = bp
            while len(self.bound) > self.max_bound:         # dataset tails / box-refinement loops bind many sizes:
                old = next(iter(self.bound))                # drop the least recently used arena + graph
                if old == key:
                    break
                del self.bound[old]
        else:
            self.bound[key] = self.bound.pop(key)           # mark as most recently used
        return bp

    def _weight_stamp(self):
        return sum(p.version for p in self.plan.params)

    def sync_weights(self):
        """Device weights follow the host Params: any Param.set since the last forward (Model.set_weights,
        Layer.set_weights, load_weights through ANOTHER model that shares these layers, init_synthetic ...) bumps
        its version; the sum over the plan's params is compared before every forward and changed tensors are
        re-packed and copied in place (pointers stay valid, captured graphs need no re-capture)."""
        stamp = self._weight_stamp()
        if self._wstamp is None:
            self._wstamp = stamp
        elif stamp != self._wstamp:
            self.refresh_weights()

    def refresh_weights(self):
        """Push changed Params to their (already bound) device tensors in place."""
        torch = _torch()
        self._wstamp = self._weight_stamp()
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            for s in self.plan.steps:
                for role, p in s.params.items():
                    if role == 'w' and s.kind == 'convtranspose':   # every packing in use: fp32 and / or the modes'
                        for (pid, key) in [k_ for k_ in self.store.conv if k_[0] == id(p)]:
                            self.store.convt_weight(p, split=key[1] if isinstance(key, tuple) else 0)
                    elif role == 'w' and s.kind != 'dwconv':
                        for (pid, split) in [k_ for k_ in self.store.conv if k_[0] == id(p)]:
                            self.store.conv_weight(p, split=split)
                    elif role == 'w':
                        self.store.dw_weight(p)
                    elif role == 'dw':
                        self.store.dw_weight(p)
                    else:
                        self.store.bn_affine(p)
        self.stream.synchronize()

    def set_inputs(self, bp, arrays):
        """Copy host (or device) arrays [m<=n, ...] into the input buffers (fp32, or the byte staging buffers of
        a uint8-bound plan)."""
        torch = _torch()
        for v, arr in zip(self.plan.inputs, arrays):
            if bp.u8 is not None:
                dst = bp.u8[id(v.buf)][0]
                src = torch.from_numpy(np.ascontiguousarray(arr)) if isinstance(arr, np.ndarray) else arr
                if src.dtype != torch.uint8 or tuple(src.shape[1:]) != tuple(dst.shape[1:]) or src.shape[0] > bp.n:
                    raise ValueError('uint8-bound plan expects uint8 input [<=%d, %s], got %s %s' %
                                     (bp.n, tuple(dst.shape[1:]), src.dtype, tuple(src.shape)))
                dst[:src.shape[0]].copy_(src.to(self.device, non_blocking=True))
                continue
            dst = bp.tensor(v)
            if isinstance(arr, np.ndarray):
                src = torch.from_numpy(np.ascontiguousarray(arr))
            else:
                src = arr
            m = src.shape[0]
            if tuple(src.shape[1:]) != tuple(dst.shape[1:]) or m > bp.n:
                raise ValueError('input has shape %s, model expects [<=%d, %s]' % (tuple(src.shape), bp.n,
                                                                                  tuple(dst.shape[1:])))
            dst[:m].copy_(src.to(self.device, non_blocking=True).to(torch.float32))

    def forward(self, bp):
        with self._lock:          # one thread at a time on the shared stream (engine/executor.py: stream_lock)
            return self._forward_locked(bp)

    def _forward_locked(self, bp):
        """Enqueue one forward pass of the bound plan on the executor stream."""
        if self.use_graph and (bp.graph is not None or bp.capture(self.stream_ptr)):
            bp.replay(self.stream_ptr)
        else:
            bp.launch_all(self.stream_ptr)

    def run(self, arrays, n=None, u8_norm=None):
        """arrays: list of host arrays with equal leading dim m <= n.  Returns list of np.float32 outputs."""
        return self.run_pipelined(arrays, n or arrays[0].shape[0], u8_norm=u8_norm)

    # ---- the chunk loops: what they share ----------------------------------------------------------------------------
    def _begin(self, bs, u8_norm=None):
        """What every run_* does first (under the lock, on this device): the device weights follow the host Params if
        anything is bound, the plan is bound at `bs` on the executor stream, the weight stamp is taken on first use."""
        if self.bound:
            self.sync_weights()
        with _torch().cuda.stream(self.stream):
            bp = self.bind(bs, u8_norm=u8_norm)
        if self._wstamp is None:
            self._wstamp = self._weight_stamp()
        return bp

    def crop_room(self, bp, store, njobs, OH, OW):
        """bp.crop_prog (one per bound plan, grown only) takes the device program of `njobs` crops out of `store`."""
        nbytes = frontend.crop_program_max_bytes(bp.lib, njobs, len(store), OH, OW)
        if bp.crop_prog is None or bp.crop_prog.numel() < nbytes:
            bp.crop_prog = _torch().empty(nbytes, dtype=_torch().uint8, device=self.device)
        store.srcs_dev                    # (uploaded on first use, with a device-wide wait: here, in front of the loop)

    def crop_step(self, bp, store, jobs_ptr, njobs, OH, OW, status_ptr=None):
        """Enqueue on the compute stream: dh_crop_program_build_dev from `njobs` resident jobs into bp.crop_prog (per-job
        status to `status_ptr` if given), then ONE dh_crop_resize_u8 launch that writes the crops straight into the plan's
        uint8 input -- no intermediate tensor."""
        prog, dst = bp.crop_prog, bp.input_bytes()
        _lib.check(bp.lib.dh_crop_program_build_dev(store.srcs_dev.data_ptr(), len(store), jobs_ptr, njobs, OH, OW, prog.data_ptr(),
                                                    prog.numel(), status_ptr, self.stream_ptr), 'dh_crop_program_build_dev')
        _lib.check(bp.lib.dh_crop_resize_u8(prog.data_ptr(), njobs, OH, OW, dst.data_ptr(), OH * OW * 3, self.stream_ptr),
                   'dh_crop_resize_u8')

    # ---- the Model.predict boundary: host arrays in, host arrays out ---------------------------------------------
    def run_pipelined(self, arrays, bs, u8_norm=None, verbose=0, crop=None):
        with self._lock:          # one thread at a time on the shared stream (engine/executor.py: stream_lock)
            return self._run_pipelined_locked(arrays, bs, u8_norm, verbose, crop)

    def _run_pipelined_locked(self, arrays, bs, u8_norm=None, verbose=0, crop=None):
        """Forward over all rows of `arrays` (host arrays, equal leading dim) in chunks of `bs`, as a 3-stage pipeline:
             host   : cast / copy chunk i+2 into pinned staging on a small THREAD POOL (row slices in parallel; the
                      copy releases the GIL) while the main thread enqueues chunk i -- a float32 batch of 64 frames is
                      50 MB, and one core writing pinned (fine-grained) host memory was the serial stage of the float32
                      boundary (66 % of the device-resident rate over 2 048 frames before the pool)
             copy   : pinned -> device staging on a copy stream      (overlaps the graph replay of chunk i)
             compute: staging -> plan input (D2D), hipGraph replay, ONE D2H of the packed outputs of the whole model
                      (arena[0 : out_items * n]) into pinned memory.
           The ring of staging slots is DEEP (up to DEEPHAR_PREDICT_DEPTH = 8 chunks in flight, capped at 512 MB of
           pinned staging per bound plan: ring_depth): on this stack every host-side wait that actually has to block is
           followed by a 40-70 ms hole in the GPU's timeline, even though later chunks are already queued
           (profiles/r02_predict_boundary.md) -- so the host enqueues ahead and waits as late as it can.
           The three stages are a FEED's (ArrayFeed above); the loop does not know which one it drives.
           crop (frontend.CropFeed; `arrays` is None): the input is cropped out of device-resident full frames instead of
           copied in.  host: chunk i+2's crop program (source table, jobs, coefficient tables) is built into pinned memory
           on the pool; copy: the program goes to the device; compute: ONE dh_crop_resize_u8 launch writes the chunk's
           crops straight into the plan's uint8 input, then the same forward and D2H.  Same slots, same events, no host
           synchronisation between chunks.  crop.program == 'device': host: chunk i+2's JOB table (24 bytes per crop) goes
           into pinned memory; copy: the jobs go to the device; compute: crop_step builds the program on the GPU from the
           store's resident source table, then the same crop launch, forward and D2H.
           Returns one np.float32 array per model output, rows in input order (keras Model.predict semantics:
           exp/common/*_tools.py; timing method of exp/pennaction/eval_speed2d.py:70-77)."""
        torch = _torch()
        feed = crop if crop is not None else ArrayFeed(self.plan, arrays)
        total = feed.total
        bs = int(min(bs, total))
        nchunks = -(-total // bs)
        with torch.cuda.device(self.device):
            bp = self._begin(bs, u8_norm)
            if getattr(self, 'copy_stream', None) is None:
                self.copy_stream = shared_stream(self.device, 'copy')
            depth = ring_depth(nchunks, feed.slot_bytes(bs, u8_norm is not None))
            feed.open(self, bp, bs, depth)
            ring = bp.ring
            ring.grow(depth)
            ring.abandon(self.stream)
            while len(bp.h2d) < depth:
                bp.h2d.append(torch.cuda.Event())
            results, staged = [], {}
            pool = _staging_pool()
            ahead = chunk_steps(total, bs, depth)               # the same sequence, read min(2, depth - 1) chunks ahead of
                                                                # the one being enqueued: the chunks staged by then

            def stage(step):
                """Start the host-side staging of a chunk into its slot; staged[ci] = the futures."""
                _, _, ci, slot, start, m = step
                ring.reclaim(slot, results)                     # chunk ci - depth used this slot (its H2D is long done)
                staged[ci] = feed.stage_chunk(pool, slot, start, m)

            try:
                for step in itertools.islice(ahead, min(2, depth - 1)):
                    stage(step)
                for _, _, ci, slot, _, m in chunk_steps(total, bs, depth):
                    for step in itertools.islice(ahead, 1):
                        stage(step)
                    done = [fu.result() for fu in staged.pop(ci)]
                    with torch.cuda.stream(self.copy_stream):
                        feed.upload(slot, m, done, self.copy_stream)
                        bp.h2d[slot].record(self.copy_stream)
                    with torch.cuda.stream(self.stream):
                        self.stream.wait_event(bp.h2d[slot])                          # GPU-side wait
                        feed.fill(slot, m)
                        self.forward(bp)
                        ring.submit(slot, m, self.stream)
                    if verbose:
                        print('%d/%d' % (min((ci + 1) * bs, total), total))
                ring.drain(nchunks, depth, results)
            finally:
                for futs in staged.values():                            # (an exception mid-loop: let the copies finish)
                    for fu in futs:
                        fu.cancel() or fu.exception()
                ring.abandon(self.stream)
        nres = len(self.plan.outputs)
        return [np.concatenate([r[k] for r in results], axis=0) if len(results) > 1 else results[0][k]
                for k in range(nres)]

    def run_refine(self, store, index, bbox0, out_hw, outidx, num_iter, winsize_scale, momentum, bs, u8_norm):
        with self._lock:          # one thread at a time on the shared stream (engine/executor.py: stream_lock)
            return self._run_refine_locked(store, index, bbox0, out_hw, outidx, num_iter, winsize_scale, momentum, bs, u8_norm)

    def _run_refine_locked(self, store, index, bbox0, out_hw, outidx, num_iter, winsize_scale, momentum, bs, u8_norm):
        """The box-refinement loop (evaltools.refine_pred_frames) with the boxes resident on the device: `num_iter` passes over
        all N samples as num_iter x nchunks chunk-steps on the compute stream, iteration-major, with no host wait between the
        first launch and the final drain other than the recycling of output slots.
          once      : bbox0 (float64 [N, 4]) and the frame indices go to the device; dh_jobs_from_boxes_f64 makes iteration 0's
                      slice of the job table int32 [num_iter, N, 6].
          chunk-step: crop_step from the resident slice of the job table (per-job status into int32 [num_iter, N]) into the
                      plan's uint8 input, the forward, the packed-output D2H into the slot; then, but for the last iteration,
                      dh_refine_boxes_f64 reads output `outidx` where it lies in the arena and writes the chunk's rows of the
                      box table and of the next iteration's job table.
          Iteration t + 1 of a chunk depends only on iteration t of the same chunk, and both are on this stream: no event.
        Returns (raw output `outidx` per iteration: list of float32 [N, J, D]; the job tables int32 [num_iter, N, 6]; the
        builder's status int32 [num_iter, N]).  A refused job leaves its input frame as the previous chunk-step left it."""
        torch = _torch()
        lib = _lib.load()
        OH, OW, _ = frontend.image_io(self.plan.inputs, u8_norm is not None, self.plan.outputs, outidx, clips=False,
                                      out_hw=out_hw, who='the device refinement loop')
        index = np.ascontiguousarray(index, np.int32)
        bbox0 = np.ascontiguousarray(bbox0, np.float64)
        total = index.shape[0]
        if bbox0.shape != (total, 4) or total < 1 or num_iter < 1:
            raise ValueError('bbox0 %s does not give one box for each of %d samples' % (bbox0.shape, total))
        if index.min() < 0 or index.max() >= len(store):
            raise ValueError('frame index outside the %d stored frames' % len(store))
        bs = int(min(bs, total))
        nchunks = -(-total // bs)
        J = self.plan.outputs[outidx].shape[0]
        with torch.cuda.device(self.device):
            bp = self._begin(bs, u8_norm)
            depth = ring_depth(num_iter * nchunks)
            self.crop_room(bp, store, bs, OH, OW)
            ring = bp.ring
            ring.grow(depth)
            ring.abandon(self.stream)
            results = []
            pose = bp.tensor(self.plan.outputs[outidx])
            try:
                with torch.cuda.stream(self.stream):
                    boxes = torch.from_numpy(bbox0).to(self.device, non_blocking=True)
                    src = torch.from_numpy(index).to(self.device, non_blocking=True)
                    jobs = torch.empty((num_iter, total, 6), dtype=torch.int32, device=self.device)
                    status = torch.empty((num_iter, total), dtype=torch.int32, device=self.device)
                    _lib.check(lib.dh_jobs_from_boxes_f64(boxes.data_ptr(), src.data_ptr(), total, jobs.data_ptr(), self.stream_ptr),
                               'dh_jobs_from_boxes_f64')
                    for _, t, _, slot, start, m in chunk_steps(total, bs, depth, num_iter):
                        ring.reclaim(slot, results, outidx)     # chunk-step `step - depth` used this slot
                        self.crop_step(bp, store, jobs[t, start].data_ptr(), m, OH, OW, status[t, start:].data_ptr())
                        self.forward(bp)
                        ring.submit(slot, m, self.stream)
                        if t + 1 < num_iter:                    # the chunk's next windows, from the poses in the arena
                            _lib.check(lib.dh_refine_boxes_f64(
                                pose.data_ptr(), pose.stride(0), pose.stride(1), J, jobs[t, start].data_ptr(),
                                boxes[start].data_ptr(), m, float(winsize_scale), float(momentum), boxes[start].data_ptr(),
                                jobs[t + 1, start].data_ptr(), self.stream_ptr), 'dh_refine_boxes_f64')
                    jobs_host = jobs.cpu().numpy()              # one copy each, behind everything on the stream
                    status_host = status.cpu().numpy()
                ring.drain(num_iter * nchunks, depth, results, outidx)
            finally:
                ring.abandon(self.stream)
        raw = [np.concatenate(results[t * nchunks:(t + 1) * nchunks], axis=0) if nchunks > 1 else results[t * nchunks]
               for t in range(num_iter)]
        return raw, jobs_host, status_host

    def run_frame_boxes(self, store, index, windows, out_hw, outidx, relsize, bs, u8_norm):
        with self._lock:          # one thread at a time on the shared stream (engine/executor.py: stream_lock)
            return self._run_frame_boxes_locked(store, index, windows, out_hw, outidx, relsize, bs, u8_norm)

    def _run_frame_boxes_locked(self, store, index, windows, out_hw, outidx, relsize, bs, u8_norm):
        """The per-frame person-box pass (evaltools.bbox.predict_frame_bboxes_frames) with the pose -> box step on the device:
        all N items as nchunks chunks on the compute stream, ONE stream of launches without a host wait in between and no
        packed-output transfer -- 52 bytes per item leave the device, once, at the end.
          once     : the job table int32 [N * per_item, 6] goes to the device (index [N]: per_item = 1; index [N, T] of a clip
                     model: per_item = T, the item's window broadcast over its frames).
          per chunk: crop_step from the resident slice of the job table (per-job status kept) into the plan's uint8 input, the
                     forward, then dh_pose_boxes_f64 reads output `outidx` where it lies in the arena (confidence channel
                     D - 2) and the item's window at jobs[i * per_item], and writes the chunk's rows of the box and status
                     tables.  The forward joins its side streams before it returns, so output `outidx` is complete on this
                     stream: no event, as in run_refine.
          at the end: one copy each of the int32 boxes, the float64 boxes, the statuses and the builder's statuses into pinned
                     memory, behind everything on the stream, and ONE drain.
        Returns (boxes int32 [N, 4], boxes float64 [N, 4], status int32 [N], the builder's status int32 [N, per_item]).  A
        refused job leaves its input frame as the previous chunk left it; the caller raises for it."""
        torch = _torch()
        lib = _lib.load()
        OH, OW, per_item = frontend.image_io(self.plan.inputs, u8_norm is not None, self.plan.outputs, outidx, out_hw=out_hw,
                                             who='the device box pass')
        vout = self.plan.outputs[outidx]
        index = np.ascontiguousarray(index, np.int32)
        windows = np.ascontiguousarray(windows, np.int32)
        total = index.shape[0]
        if total < 1 or index.shape != ((total,) if per_item == 1 else (total, per_item)) or windows.shape != (total, 4):
            raise ValueError('index %s and windows %s do not describe items of %d frame(s)' % (index.shape, windows.shape, per_item))
        if index.min() < 0 or index.max() >= len(store):
            raise ValueError('frame index outside the %d stored frames' % len(store))
        table = np.zeros((total, per_item, 6), np.int32)
        table[:, :, 0] = index.reshape(total, per_item)
        table[:, :, 1:5] = windows[:, None, :]
        bs = int(min(bs, total))
        J, D = int(vout.shape[-2]), int(vout.shape[-1])
        with torch.cuda.device(self.device):
            bp = self._begin(bs, u8_norm)
            self.crop_room(bp, store, bs * per_item, OH, OW)
            if bp.boxes_host is None or bp.boxes_host[0].shape[0] < total:               # pinned result tables, grown only
                bp.boxes_host = [torch.empty(shape, dtype=dt, pin_memory=True) for shape, dt in
                                 (((total, 4), torch.int32), ((total, 4), torch.float64), ((total,), torch.int32),
                                  ((total, per_item), torch.int32))]
            host = [h[:total] for h in bp.boxes_host]
            pose = bp.tensor(vout)                                  # [bs, (T,) J, D] where the forward leaves it
            item_stride = pose.stride(0)
            frame_stride = pose.stride(1) if per_item > 1 else item_stride
            try:
                with torch.cuda.stream(self.stream):
                    jobs = torch.from_numpy(table).to(self.device, non_blocking=True)
                    boxes = torch.empty((total, 4), dtype=torch.int32, device=self.device)
                    boxes_f = torch.empty((total, 4), dtype=torch.float64, device=self.device)
                    status = torch.empty((total,), dtype=torch.int32, device=self.device)
                    built = torch.zeros((total, per_item), dtype=torch.int32, device=self.device)
                    for _, _, _, _, start, m in chunk_steps(total, bs, 1):
                        self.crop_step(bp, store, jobs[start].data_ptr(), m * per_item, OH, OW, built[start].data_ptr())
                        self.forward(bp)
                        _lib.check(lib.dh_pose_boxes_f64(
                            pose.data_ptr(), item_stride, frame_stride, pose.stride(-2), per_item, J, D - 2,
                            jobs[start].data_ptr(), per_item, m, float(relsize), boxes[start].data_ptr(),
                            boxes_f[start].data_ptr(), status[start:].data_ptr(), self.stream_ptr), 'dh_pose_boxes_f64')
                    for h, d in zip(host, (boxes, boxes_f, status, built)):      # behind everything on the stream
                        h.copy_(d, non_blocking=True)
            finally:
                self.stream.synchronize()                           # the one drain (and nothing in flight behind an exception)
        return tuple(h.numpy().copy() for h in host)

    def run_votes(self, store, index, windows, hflip, seq, nseq, outidx_list, keep_scores, bs, u8_norm):
        with self._lock:          # one thread at a time on the shared stream (engine/executor.py: stream_lock)
            return self._run_votes_locked(store, index, windows, hflip, seq, nseq, outidx_list, keep_scores, bs, u8_norm)

    def _run_votes_locked(self, store, index, windows, hflip, seq, nseq, outidx_list, keep_scores, bs, u8_norm):
        """The multi-clip action vote (evaltools.action.multiclip_votes_frames) on the device: all N items (clips, as they are
        or mirrored) as nchunks chunks on the compute stream, ONE stream of launches without a host wait in between and no
        packed-output transfer.
          once     : the job table int32 [N, per_item, 6] goes to the device (the item's window broadcast over its frames, its
                     mirror flag in every job's hflip field), and so does seq; acc float64 [nb, nseq, C] is set to ones.
          per chunk: crop_step from the resident slice of the job table (per-job status kept) into the plan's uint8 input, the
                     forward, then ONE dh_vote_products_f64 call that reads the action outputs `outidx_list` where they lie in
                     the arena and multiplies the chunk's rows into acc, with seq[start:].  Its label and score tables are dense
                     per CALL, so the chunk's block [nb, m(, C)] lies at nb * start (* C) of a flat table and is put in place
                     on the host.  The forward joins its side streams before it returns, so the outputs are complete on this
                     stream: no event, as in run_frame_boxes.  A sequence may straddle chunks: the products stay in acc.
          at the end: one copy each of acc, the labels, the builder's statuses and the optional scores into pinned memory,
                     behind everything on the stream, and ONE drain.
        Returns (a_pred float64 [nb, nseq, C], labels int32 [nb, N], scores float32 [nb, N, C] or None, the builder's status
        int32 [N, per_item]).  A refused job leaves its input frame as the previous chunk left it; the caller raises for it."""
        torch = _torch()
        lib = _lib.load()
        OH, OW, per_item = frontend.image_io(self.plan.inputs, u8_norm is not None, who='the device vote')
        outs = [self.plan.outputs[k] for k in outidx_list]
        if not outs or any(len(v.shape) != 1 or tuple(v.shape) != tuple(outs[0].shape) for v in outs):
            raise ValueError('outputs %s are not action outputs of one shape (C,): %s' %
                             (list(outidx_list), [tuple(v.shape) for v in outs]))
        nb, C, nseq = len(outs), int(outs[0].shape[0]), int(nseq)
        index = np.ascontiguousarray(index, np.int32)
        windows = np.ascontiguousarray(windows, np.int32)
        hflip = np.asarray(hflip).astype(bool)
        seq = np.ascontiguousarray(seq, np.int32)
        total = index.shape[0]
        if total < 1 or index.shape != ((total,) if per_item == 1 else (total, per_item)) or windows.shape != (total, 4) or \
                hflip.shape != (total,) or seq.shape != (total,):
            raise ValueError('index %s, windows %s, hflip %s and seq %s do not describe items of %d frame(s)' %
                             (index.shape, windows.shape, hflip.shape, seq.shape, per_item))
        if index.min() < 0 or index.max() >= len(store):
            raise ValueError('frame index outside the %d stored frames' % len(store))
        if nseq < 1 or seq.min() < 0 or seq.max() >= nseq:
            raise ValueError('seq outside [0, %d)' % nseq)
        table = np.zeros((total, per_item, 6), np.int32)
        table[:, :, 0] = index.reshape(total, per_item)
        table[:, :, 1:5] = windows[:, None, :]
        table[:, :, 5] = hflip[:, None]
        bs = int(min(bs, total))
        sizes = [(nb * nseq * C, torch.float64), (nb * total, torch.int32), (total * per_item, torch.int32)] + \
            ([(nb * total * C, torch.float32)] if keep_scores else [])
        with torch.cuda.device(self.device):
            bp = self._begin(bs, u8_norm)
            self.crop_room(bp, store, bs * per_item, OH, OW)
            if bp.votes_host is None or len(bp.votes_host) < len(sizes) or \
                    any(h.numel() < size for h, (size, _) in zip(bp.votes_host, sizes)):           # pinned result tables
                bp.votes_host = [torch.empty(size, dtype=dt, pin_memory=True) for size, dt in sizes]
            host = [h[:size] for h, (size, _) in zip(bp.votes_host, sizes)]
            probs = [bp.tensor(v) for v in outs]                    # [bs, C] each, where the forward leaves them
            srcs = (_lib.VoteSrc * nb)(*[_lib.VoteSrc(p.data_ptr(), max(p.stride(0), C)) for p in probs])
            try:
                with torch.cuda.stream(self.stream):
                    jobs = torch.from_numpy(table).to(self.device, non_blocking=True)
                    seq_dev = torch.from_numpy(seq).to(self.device, non_blocking=True)
                    acc = torch.ones(nb * nseq * C, dtype=torch.float64, device=self.device)
                    label = torch.empty(nb * total, dtype=torch.int32, device=self.device)
                    built = torch.zeros(total * per_item, dtype=torch.int32, device=self.device)
                    scores = torch.empty(nb * total * C, dtype=torch.float32, device=self.device) if keep_scores else None
                    for _, _, _, _, start, m in chunk_steps(total, bs, 1):
                        self.crop_step(bp, store, jobs[start].data_ptr(), m * per_item, OH, OW,
                                       built[start * per_item:].data_ptr())
                        self.forward(bp)
                        _lib.check(lib.dh_vote_products_f64(
                            srcs, nb, C, seq_dev[start:].data_ptr(), m, nseq, acc.data_ptr(), label[nb * start:].data_ptr(),
                            scores[nb * start * C:].data_ptr() if keep_scores else None, self.stream_ptr), 'dh_vote_products_f64')
                    for h, d in zip(host, (acc, label, built) + ((scores,) if keep_scores else ())):
                        h.copy_(d, non_blocking=True)               # behind everything on the stream
            finally:
                self.stream.synchronize()                           # the one drain (and nothing in flight behind an exception)
        a_pred = host[0].numpy().reshape(nb, nseq, C).copy()
        labels = np.empty((nb, total), np.int32)
        out_scores = np.empty((nb, total, C), np.float32) if keep_scores else None
        for _, _, _, _, start, m in chunk_steps(total, bs, 1):      # every call's dense block into its columns
            labels[:, start:start + m] = host[1].numpy()[nb * start:nb * (start + m)].reshape(nb, m)
            if keep_scores:
                out_scores[:, start:start + m] = host[3].numpy()[nb * start * C:nb * (start + m) * C].reshape(nb, m, C)
        return a_pred, labels, out_scores, host[2].numpy().reshape(total, per_item).copy()

    def run_device(self, tensors, n=None, inputs_copied=None):
        with self._lock:         # one thread at a time on the shared stream (engine/executor.py: stream_lock)
            return self._run_device_locked(tensors, n, inputs_copied)

    def _run_device_locked(self, tensors, n=None, inputs_copied=None):
        """Device tensors in ([m <= n, ...] float32 on this device), device VIEWS of the outputs out (valid until the
        next forward of the same bound plan); everything is enqueued on `self.stream`, nothing touches the host.
        An input may be any strided view with the input's element count whose leading dim is m -- e.g. the
        [m, G, T/G, J, c] view of a rank-major all-gather result: the copy into the plan's contiguous [m, T, J, c]
        input does the re-ordering.  `inputs_copied`: optional torch event recorded on `self.stream` right after the
        input copies (the producer may then overwrite its buffers).
        Used by the frame-sharded clip runtime (parallel.py) around the RCCL all-gather."""
        torch = _torch()
        m = tensors[0].shape[0]
        n = n or m
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            bp = self._begin(n)
            for v, t in zip(self.plan.inputs, tensors):
                dst = bp.tensor(v)[:m] if m <= bp.n else None
                if dst is None or t.shape[0] != m or t.numel() != dst.numel() or \
                        tuple(t.shape[-1:]) != tuple(v.shape[-1:]):
                    raise ValueError('input has shape %s, model expects [<=%d, %s]' % (tuple(t.shape), bp.n, v.shape))
                if tuple(t.shape) != tuple(dst.shape):
                    dst = dst.view(tuple(t.shape))
                dst.copy_(t, non_blocking=True)
            if inputs_copied is not None:
                inputs_copied.record(self.stream)
            self.forward(bp)
            return [bp.tensor(v)[:m] for v in self.plan.outputs]
