"""Crop-and-resize front end: predict from FULL frames and boxes.

The reference crops on the host with PIL, per frame and per call -- T.rotate_crop(angle, objpos, winsize), T.resize(
crop_resolution), optional T.horizontal_flip() (deephar/data/mpii.py:114-118, pennaction.py:157-161) -- and callers such as
the box-refinement loop (exp/common/mpii_tools.py:13-52) re-crop the same images again and again.  Here the frames are
uploaded once (FrameStore) and every chunk's crops are ONE launch (dh_crop_resize_u8) that writes straight into the uint8
input of the bound plan; the result is bit for bit `model.predict(<the loader's uint8 crops>)`.
The launch reads a crop program (csrc/crop_index.h).  program='host' (the default) builds it on the host per chunk and copies
it over; program='device' stages only the chunk's 24-byte jobs and builds the program on the GPU (dh_crop_program_build_dev,
the same bytes), in front of the crop launch on the compute stream.
refine_from_frames runs the whole box-refinement loop with the boxes resident on the device (dh_refine_boxes_f64 behind every
forward, csrc/refine_index.h): the caller the device builder was made for.
frame_boxes_from_frames is the per-frame person-box pass: the pose -> box step is one launch behind every forward
(dh_pose_boxes_f64, csrc/posebox_index.h) and only the boxes leave the device.
votes_from_frames is the multi-clip action vote: the product of the per-clip class probabilities is one launch behind every
forward (dh_vote_products_f64, csrc/vote_index.h) and no model output leaves the device.

Scope: the loaders' test-mode geometry -- angle 0, integer window, bilinear, optional mirror, 3 channels, uint8.  Box and
matrix bookkeeping stays on the host in float64 (crop_box, crop_afmat), composed like deephar/utils/transform.py does.
The reference pins Pillow 5.1.0; bit-equality was checked against the Pillow recorded in tests/golden/crop_reference.npz.
"""
import ctypes as C

import numpy as np

from . import _lib


def crop_box(objpos, winsize):
    """The integer window of T.rotate_crop(0, objpos, winsize) (transform.py:110-111): corners truncated toward zero."""
    cx, cy = float(objpos[0]), float(objpos[1])
    w, h = float(winsize[0]), float(winsize[1])
    return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dtype=int)


def crop_afmat(box, out_wh, hflip=False):
    """afmat of the loaders after crop, resize, optional flip and normalize_affinemap: image pixels -> [0, 1] crop coordinates.
    Composed by np.dot(t, afmat) in the loaders' order, one elementary matrix at a time, so every entry has their bits."""
    x0, y0, x1, y1 = (int(v) for v in box)
    ow, oh = int(out_wh[0]), int(out_wh[1])

    def translate(x, y):
        t = np.eye(3)
        t[0, 2], t[1, 2] = x, y
        return t

    def scale(w, h):
        t = np.eye(3)
        t[0, 0] *= w
        t[1, 1] *= h
        return t

    A = np.dot(translate(-x0, -y0), np.eye(3))
    A = np.dot(scale(ow / (x1 - x0), oh / (y1 - y0)), A)
    if hflip:
        A = np.dot(scale(-1, 1), A)
        A = np.dot(translate(ow, 0), A)
    return np.dot(scale(1 / ow, 1 / oh), A)


def image_io(inputs, u8=True, outputs=None, outidx=None, clips=True, out_hw=None, who='the crop front end'):
    """What the frame front ends feed, stated once: a single uint8 image input [(T,) H, W, 3] per item (clips=False: [H, W, 3]
    only; out_hw: of that very size) and, where `outidx` is given, a pose output [(T,) J, D >= 2] at that index of `outputs`.
    `inputs` / `outputs`: a Model's or a Plan's (anything with a per-item .shape).  Returns (OH, OW, per_item)."""
    if len(inputs) != 1:
        raise ValueError('%s needs a single image input, got %d inputs' % (who, len(inputs)))
    shape = tuple(inputs[0].shape)
    if not u8 or len(shape) not in ((3, 4) if clips else (3,)) or shape[-1] != 3:
        raise ValueError('%s needs a uint8 image input [%sH, W, 3], not %s%s' %
                         (who, '(T,) ' if clips else '', '' if u8 else 'float32 ', shape))
    OH, OW = int(shape[-3]), int(shape[-2])
    if out_hw is not None and (int(out_hw[0]), int(out_hw[1])) != (OH, OW):
        raise ValueError('%s: crops of [%d, %d, 3] do not fill the input %s' % (who, out_hw[0], out_hw[1], shape))
    per_item = 1 if len(shape) == 3 else int(shape[0])
    if outidx is not None:
        if not -len(outputs) <= outidx < len(outputs):
            raise ValueError('output %d of %d' % (outidx, len(outputs)))
        vout = tuple(outputs[outidx].shape)
        if len(vout) != len(shape) - 1 or vout[-1] < 2 or (per_item > 1 and vout[0] != per_item):
            raise ValueError('output %d %s is no pose output [(T,) J, D >= 2]' % (outidx, vout))
    return OH, OW, per_item


def refused_window(status, where=''):
    """The ValueError for a window the crop-program builder refuses (its status: -2 beyond the scale cap, else a bad box)."""
    what = 'empty crop box' if status != -2 else \
        'a crop window is more than 16 times its output on one axis (or the output row does not fit LDS)'
    return ValueError(what + (': ' + where if where else ''))


def crop_program_max_bytes(lib, njobs, nsrc, OH, OW):
    """What the device program of `njobs` crops can take (dh_crop_program_max_bytes): allocated before the boxes are known."""
    nbytes = C.c_size_t(0)
    rc = lib.dh_crop_program_max_bytes(njobs, nsrc, OH, OW, C.byref(nbytes))
    if rc == -2:
        raise ValueError('the crop program of %d jobs does not fit 2^31 bytes' % njobs)
    _lib.check(rc, 'dh_crop_program_max_bytes')
    return nbytes.value


class FrameStore:
    """Full frames resident on the device: each uint8 [H, W, 3] frame is uploaded once; frames may differ in size."""

    def __init__(self, frames, device=None):
        import torch
        if not torch.cuda.is_available():
            raise _lib.DeepharHipError('no HIP device visible: the crop front end runs only on the GPU')
        self.device = torch.device(device or 'cuda:%d' % torch.cuda.current_device())
        self.tensors = []
        for f in frames:
            a = np.ascontiguousarray(f)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError('frames must be uint8 [H, W, 3] arrays, got %s %s' % (a.dtype, a.shape))
            self.tensors.append(torch.from_numpy(a).to(self.device))
        torch.cuda.synchronize(self.device)          # once, at upload: every later launch may read the frames on any stream
        self.srcs = (_lib.CropSrc * len(self.tensors))(*[
            _lib.CropSrc(t.data_ptr(), 3 * t.shape[1], t.shape[0], t.shape[1]) for t in self.tensors])
        self._srcs_dev = None

    @property
    def srcs_dev(self):
        """The source table on the device (what dh_crop_program_build_dev reads), uploaded once, on first use."""
        if self._srcs_dev is None:
            import torch
            self._srcs_dev = torch.from_numpy(np.frombuffer(bytes(self.srcs), np.uint8).copy()).to(self.device)
            torch.cuda.synchronize(self.device)
        return self._srcs_dev

    def __len__(self):
        return len(self.tensors)


class CropFeed:
    """What Executor.run_pipelined needs to crop its own input: the per-chunk crop programs over a FrameStore, as a feed
    (stage_chunk / upload / fill per chunk after slot_bytes and open: engine/executor.py, ArrayFeed)."""

    def __init__(self, store, index, boxes, hflip, out_hw, program='host'):
        if program not in ('host', 'device'):
            raise ValueError("program must be 'host' or 'device', got %r" % (program,))
        self.store, self.lib, self.program = store, _lib.load(), program
        # chosen here, once: what a chunk stages into its slot (its job table / its program) and what fills the plan's input
        self._stage, self.fill = (self.stage, self._fill_built) if program == 'device' else (self.build, self._fill_uploaded)
        self.index = np.asarray(index, np.int64)
        self.boxes = np.asarray(boxes, np.int64)
        self.hflip = np.asarray(hflip).astype(bool)
        self.OH, self.OW = int(out_hw[0]), int(out_hw[1])
        self.total = self.index.shape[0]
        self.per_item = int(np.prod(self.index.shape[1:], dtype=np.int64))           # frames per item: 1, or T of a clip model
        if self.boxes.shape != self.index.shape + (4,) or self.hflip.shape != self.index.shape:
            raise ValueError('index %s, boxes %s and hflip %s do not describe the same jobs' %
                             (self.index.shape, self.boxes.shape, self.hflip.shape))
        if self.total and (self.index.min() < 0 or self.index.max() >= len(store)):
            raise ValueError('frame index outside the %d stored frames' % len(store))
        if np.any(self.boxes[..., 2] <= self.boxes[..., 0]) or np.any(self.boxes[..., 3] <= self.boxes[..., 1]):
            raise refused_window(-1)
        flat = np.concatenate([self.index.reshape(-1, 1), self.boxes.reshape(-1, 4), self.hflip.reshape(-1, 1)], axis=1)
        self.jobs = np.ascontiguousarray(flat.astype(np.int32))                       # == dh_crop_job[total * per_item]

    def _jobs(self, start, m):
        part = self.jobs[start * self.per_item:(start + m) * self.per_item]
        return part.ctypes.data_as(C.POINTER(_lib.CropJob)), len(part)

    def program_bytes(self, start, m):
        jobs, n = self._jobs(start, m)
        nbytes = C.c_size_t(0)
        rc = self.lib.dh_crop_program_bytes(jobs, n, len(self.store), self.OH, self.OW, C.byref(nbytes))
        if rc == -2:
            raise refused_window(rc)
        _lib.check(rc, 'dh_crop_program_bytes')
        return nbytes.value

    def build(self, start, m, out):
        """The program of items [start, start + m) into the pinned uint8 tensor `out`; returns its bytes."""
        nbytes = self.program_bytes(start, m)
        jobs, n = self._jobs(start, m)
        if out.numel() < nbytes or out.data_ptr() % 8:
            raise ValueError('crop program buffer too small or misaligned')
        _lib.check(self.lib.dh_crop_program_build_host(self.store.srcs, len(self.store), jobs, n, self.OH, self.OW,
                                                       out.data_ptr(), nbytes), 'dh_crop_program_build_host')
        return nbytes

    # ---- program='device': a chunk's staging is its job table, the program is built by the GPU
    def max_bytes(self, m):
        """What the device program of a chunk of m items can take (dh_crop_program_max_bytes)."""
        return crop_program_max_bytes(self.lib, m * self.per_item, len(self.store), self.OH, self.OW)

    def stage(self, start, m, out):
        """The job table of items [start, start + m) -- 24 bytes per job, nothing else -- into the uint8 tensor `out`; returns
        its bytes."""
        import torch
        part = self.jobs[start * self.per_item:(start + m) * self.per_item]
        nbytes = part.size * 4
        if out.numel() < nbytes:
            raise ValueError('job staging too small')
        out[:nbytes].copy_(torch.from_numpy(part.reshape(-1).view(np.uint8)))
        return nbytes

    # ---- the feed of Executor.run_pipelined
    def slot_bytes(self, bs, u8):
        return 0                          # nothing of the model's input is staged: the crop launch writes it in place

    def open(self, ex, bp, bs, depth):
        """The checks against the plan's input; then per slot of bp.byte_slots pinned host memory for a chunk's crop program
        (program='device': for its JOB table, and bp.crop_prog for the program the GPU builds) and its device twin."""
        import torch
        if (self.OH, self.OW, self.per_item) != image_io(ex.plan.inputs, bp.u8 is not None):
            raise ValueError('crops of %d x [%d, %d, 3] do not fill the model input %s' %
                             (self.per_item, self.OH, self.OW, tuple(ex.plan.inputs[0].shape)))
        # (the size query refuses a window beyond the scale cap before anything is enqueued)
        nbytes = max(self.program_bytes(c0, min(bs, self.total - c0)) for c0 in range(0, self.total, bs))
        if self.program == 'device':
            nbytes = 24 * bs * self.per_item
            ex.crop_room(bp, self.store, bs * self.per_item, self.OH, self.OW)
        for k in range(depth):
            if k == len(bp.byte_slots):
                bp.byte_slots.append(None)
            if bp.byte_slots[k] is None or bp.byte_slots[k][0].numel() < nbytes:
                bp.byte_slots[k] = (torch.empty(nbytes, dtype=torch.uint8, pin_memory=True),
                                    torch.empty(nbytes, dtype=torch.uint8, device=ex.device))
        self.ex, self.bp = ex, bp

    def stage_chunk(self, pool, slot, start, m):
        return [pool.submit(self._stage, start, m, self.bp.byte_slots[slot][0])]     # built / copied off the main thread

    def upload(self, slot, m, staged, copy_stream):
        host, dev = self.bp.byte_slots[slot]
        dev[:staged[0]].copy_(host[:staged[0]], non_blocking=True)                   # the bytes `_stage` reported

    def _fill_uploaded(self, slot, m):
        dst = self.bp.input_bytes()
        _lib.check(self.lib.dh_crop_resize_u8(self.bp.byte_slots[slot][1].data_ptr(), m * self.per_item, self.OH, self.OW,
                                              dst.data_ptr(), self.OH * self.OW * 3, self.ex.stream_ptr), 'dh_crop_resize_u8')

    def _fill_built(self, slot, m):      # the program from the slot's jobs, on the compute stream, in front of the launch
        self.ex.crop_step(self.bp, self.store, self.bp.byte_slots[slot][1].data_ptr(), m * self.per_item, self.OH, self.OW)


def refine_from_frames(model, frames, index, bbox0, outidx, num_iter=2, winsize_scale=1.50, momentum=0.8, batch_size=8):
    """The box-refinement loop of evaltools.refine_pred_frames with the boxes resident on the GPU (Executor.run_refine): every
    iteration's windows come from the previous iteration's poses through dh_refine_boxes_f64 and go straight into
    dh_crop_program_build_dev; nothing visits the host between the first launch and the final drain.  Single-image models only.
    Returns (raw output `outidx` per iteration, crop-normalised; the integer windows [num_iter, N, 4] every iteration
    cropped; their crop_afmat maps [num_iter, N, 3, 3]).  ValueError, after the drain, for the first window the program builder
    refused: the errors CropFeed raises on the host for the same window."""
    OH, OW, _ = image_io(model.inputs, clips=False, who='refine_from_frames of %s' % model.name)
    ex = model.executor
    store = frames if isinstance(frames, FrameStore) else FrameStore(frames, ex.device)
    total = len(index)
    bs = int(min(batch_size or total, total))
    raws, jobs, status = ex.run_refine(store, index, bbox0, (OH, OW), outidx, num_iter, winsize_scale, momentum, bs,
                                       model.channel_power)
    bad = np.argwhere(status != 0)
    if len(bad):
        t, i = (int(v) for v in bad[0])
        raise refused_window(status[t, i], 'iteration %d, sample %d, window %s' % (t, i, jobs[t, i, 1:5].tolist()))
    windows = jobs[:, :, 1:5].astype(np.int64)
    afmat = np.zeros((num_iter, total, 3, 3))
    for pos in np.ndindex(num_iter, total):
        afmat[pos] = crop_afmat(windows[pos], (OW, OH), False)
    return raws, windows, afmat


def frame_boxes_from_frames(model, frames, index, windows, outidx=-1, scale=1.5, batch_size=32):
    """The per-frame person-box pass with the pose -> box step on the GPU (Executor.run_frame_boxes): every chunk is cropped
    out of the resident frames, predicted, and its poses are turned into boxes by dh_pose_boxes_f64 where the forward left them
    (csrc/posebox_index.h restates evaltools.bbox.get_bbox_from_poses); no model output is copied to the host.
    index [N] (image model) or [N, T] (clip model); windows: integer (x0, y0, x1, y1) per item as crop_box makes them, [N, 4],
    cropped unflipped and, for a clip model, broadcast over the item's frames.
    Returns (boxes int64 [N, 4] -- get_bbox_from_poses(...).astype(int); boxes float64 [N, 4]; status int32 [N]: 0 ok, 1 a frame
    keeps no joint, 2 a kept joint is NaN, 3 a corner does not fit int32, 4 never here).  ValueError, after the drain, for the
    first window the program builder refused: the errors CropFeed raises on the host for the same window."""
    OH, OW, _ = image_io(model.inputs, who='frame_boxes_from_frames of %s' % model.name)
    index = np.asarray(index, np.int64)
    windows = np.asarray(windows)
    if windows.dtype.kind not in 'iu':
        raise ValueError('windows must be integer windows (frontend.crop_box)')
    if index.ndim < 1 or index.shape[1:] != tuple(model.inputs[0].shape[:-3]):
        raise ValueError('index has shape %s, the model takes %s per item' % (index.shape, tuple(model.inputs[0].shape)))
    total = index.shape[0]
    if windows.shape != (total, 4):
        raise ValueError('windows %s do not give one window for each of %d items' % (windows.shape, total))
    if total == 0:
        return np.zeros((0, 4), np.int64), np.zeros((0, 4)), np.zeros((0,), np.int32)
    if np.abs(windows).max() > 0x7fffffff:
        raise ValueError('a window corner does not fit int32')
    ex = model.executor
    store = frames if isinstance(frames, FrameStore) else FrameStore(frames, ex.device)
    bs = int(min(batch_size or total, total))
    boxes, boxes_f64, status, built = ex.run_frame_boxes(store, index, windows, (OH, OW), outidx, scale, bs, model.channel_power)
    bad = np.argwhere(built != 0)
    if len(bad):
        i = int(bad[0][0])
        raise refused_window(built[tuple(bad[0])], 'sample %d, window %s' % (i, windows[i].tolist()))
    return boxes.astype(np.int64), boxes_f64, status


def vote_outputs(outputs, outidx=None):
    """The action outputs a vote reads: `outidx` (None: all) as non-negative indices into `outputs`, which must all have the
    same per-item shape (C,).  Returns (indices, C)."""
    picked = list(range(len(outputs))) if outidx is None else [int(k) for k in outidx]
    if not picked:
        raise ValueError('no output to vote on')
    for k in picked:
        if not -len(outputs) <= k < len(outputs):
            raise ValueError('output %d of %d' % (k, len(outputs)))
    picked = [k % len(outputs) for k in picked]
    shapes = [tuple(outputs[k].shape) for k in picked]
    if any(len(s) != 1 or s != shapes[0] for s in shapes):
        raise ValueError('outputs %s are not action outputs of one shape (C,): %s' % (picked, shapes))
    return picked, int(shapes[0][0])


def votes_from_frames(model, frames, index, windows, hflip, seq, nseq=None, outidx=None, keep_scores=False, batch_size=8):
    """The multi-clip action vote with the vote on the GPU (Executor.run_votes): every chunk of items -- clips as they are or
    mirrored -- is cropped out of the resident frames and predicted, and dh_vote_products_f64 multiplies its class probabilities
    into the running products of the items' sequences where the forward left them (csrc/vote_index.h restates
    evaltools.action.vote_products); no model output is copied to the host.
    index [N] (image model) or [N, T] (clip model); windows: integer (x0, y0, x1, y1) per item as crop_box makes them, [N, 4],
    broadcast over the item's frames; hflip: one mirror flag per item, [N]; seq: the sequence of every item, [N], in [0, nseq)
    (nseq None: max(seq) + 1); outidx: the action outputs voted on (None: all), every one of per-item shape (C,).
    Items are voted in their order; they need not be sorted by sequence.
    Returns (a_pred float64 [nb, nseq, C]: the products; labels int32 [nb, N]: np.argmax of the item's sequence right after the
    item; scores float32 [nb, N, C]: the per-item probabilities, or None without keep_scores).  ValueError, after the drain, for
    the first window the program builder refused: the errors CropFeed raises on the host for the same window."""
    image_io(model.inputs, who='votes_from_frames of %s' % model.name)
    picked, C = vote_outputs(model.outputs, outidx)
    index = np.asarray(index, np.int64)
    windows = np.asarray(windows)
    if windows.dtype.kind not in 'iu':
        raise ValueError('windows must be integer windows (frontend.crop_box)')
    if index.ndim < 1 or index.shape[1:] != tuple(model.inputs[0].shape[:-3]):
        raise ValueError('index has shape %s, the model takes %s per item' % (index.shape, tuple(model.inputs[0].shape)))
    total = index.shape[0]
    hflip = np.asarray(hflip).astype(bool)
    seq = np.asarray(seq)
    if windows.shape != (total, 4) or hflip.shape != (total,) or seq.shape != (total,):
        raise ValueError('windows %s, hflip %s and seq %s do not give one window, flag and sequence for each of %d items' %
                         (windows.shape, hflip.shape, seq.shape, total))
    if total and seq.dtype.kind not in 'iu':
        raise ValueError('seq must be integers')
    nseq = int(nseq) if nseq is not None else (int(seq.max()) + 1 if total else 0)
    if total and (nseq < 1 or seq.min() < 0 or seq.max() >= nseq):
        raise ValueError('seq outside [0, %d)' % nseq)
    if total == 0:
        return (np.ones((len(picked), max(nseq, 0), C)), np.zeros((len(picked), 0), np.int32),
                np.zeros((len(picked), 0, C), np.float32) if keep_scores else None)
    if np.abs(windows).max() > 0x7fffffff:
        raise ValueError('a window corner does not fit int32')
    ex = model.executor
    store = frames if isinstance(frames, FrameStore) else FrameStore(frames, ex.device)
    if index.min() < 0 or index.max() >= len(store):
        raise ValueError('frame index outside the %d stored frames' % len(store))
    bs = int(min(batch_size or total, total))
    a_pred, labels, scores, built = ex.run_votes(store, index, windows, hflip, seq, nseq, picked, keep_scores, bs,
                                                 model.channel_power)
    bad = np.argwhere(built != 0)
    if len(bad):
        i = int(bad[0][0])
        raise refused_window(built[tuple(bad[0])], 'item %d, window %s' % (i, windows[i].tolist()))
    return a_pred, labels, scores


def predict_from_frames(model, frames, index, boxes, hflip=None, batch_size=32, program='host'):
    """model.predict on crops of full frames, cropped on the GPU.

    frames : a FrameStore, or a sequence of uint8 [H, W, 3] arrays (uploaded once, here)
    index  : [N] frame numbers, or [N, T] for a clip model
    boxes  : integer windows (x0, y0, x1, y1) as crop_box makes them: [N, 4], [N, T, 4], or [N, 4] for a clip model (the
             clip-level box is broadcast over the clip's frames)
    hflip  : None, one flag, or one per item ([N]) or per frame ([N, T])
    Returns the outputs of model.predict as a list, followed by the float64 affine maps [N(, T), 3, 3] (crop_afmat).
    program: 'host' -- every chunk's crop program is built on the host and copied to the device; 'device' -- only the chunk's
             jobs are staged and the program is built on the GPU in front of the crop launch.  The same bits either way.
    Bit for bit model.predict(<uint8 crops of the loader>, batch_size)."""
    if program not in ('host', 'device'):
        raise ValueError("program must be 'host' or 'device', got %r" % (program,))
    OH, OW, _ = image_io(model.inputs, who='predict_from_frames of %s' % model.name)
    index = np.asarray(index, np.int64)
    boxes = np.asarray(boxes)
    if boxes.dtype.kind not in 'iu':
        raise ValueError('boxes must be integer windows (frontend.crop_box)')
    if index.ndim < 1 or index.shape[1:] != tuple(model.inputs[0].shape[:-3]):
        raise ValueError('index has shape %s, the model takes %s per item' % (index.shape, tuple(model.inputs[0].shape)))
    if index.ndim == 2 and boxes.ndim == 2:
        boxes = np.broadcast_to(boxes[:, None, :], index.shape + (4,))
    flips = np.zeros(index.shape, bool) if hflip is None else np.asarray(hflip).astype(bool)
    if flips.ndim < index.ndim:
        flips = np.broadcast_to(flips.reshape(flips.shape + (1,) * (index.ndim - flips.ndim)), index.shape)
    afmat = np.zeros(index.shape + (3, 3))
    for pos in np.ndindex(*index.shape):
        afmat[pos] = crop_afmat(boxes[pos], (OW, OH), bool(flips[pos]))
    if index.shape[0] == 0:
        return [np.zeros((0,) + tuple(t.shape), np.float32) for t in model.outputs] + [afmat]
    ex = model.executor
    store = frames if isinstance(frames, FrameStore) else FrameStore(frames, ex.device)
    feed = CropFeed(store, index, boxes, flips, (OH, OW), program)
    bs = int(min(batch_size or feed.total, feed.total))
    outs = ex.run_pipelined(None, bs, u8_norm=model.channel_power, crop=feed)
    return list(outs) + [afmat]
