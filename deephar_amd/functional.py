"""Op-level Python API over the C-ABI, on torch CUDA tensors (NHWC fp32, contiguous).

One function per kernel entry point of include/deephar_hip.h; used by the op parity tests and available to
callers that want a single fused op rather than a whole Model.  Launches go to torch's current stream.
No CPU path: every function raises if handed a non-CUDA tensor.
"""
import ctypes as C

import numpy as np

from . import _lib
from .engine import packing
from .engine.executor import grid_x, grid_depth
from .layers import same_pad


def _t():
    import torch
    return torch


def _stream():
    return _t().cuda.current_stream().cuda_stream


def _chk(*tensors):
    torch = _t()
    for t in tensors:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError('deephar_amd.functional expects contiguous float32 CUDA tensors')


def _p(t):
    return t.data_ptr() if t is not None else None


def pack_conv_weight(w_hwio, device='cuda'):
    """HWIO numpy kernel -> (packed device tensor, Kp, Np)."""
    torch = _t()
    packed, kp, np_ = packing.pack_conv(np.asarray(w_hwio, np.float32))
    return torch.from_numpy(packed).to(device), kp, np_


def conv2d(x, w_hwio, strides=(1, 1), padding='same', pre_scale=None, pre_shift=None, pre_relu=False,
           post_scale=None, post_shift=None, post_relu=False, res1=None, res2=None, up2=False, tile_cfg=-1,
           packed=None, in_lut=None, split=False, halo=False, res2_down=False, pool2=False, x_resample=0, seg=None,
           precision=None, scope='standard'):
    """Fused conv (see dh_conv2d_f32).  x [N,H,W,Cin]; w_hwio numpy [kh,kw,Cin,Cout].  A uint8 `x` needs
    `in_lut` (float32 [Cin,256] device tensor, engine.executor.normalization_lut): bytes are normalised on load.
    precision: None / 'f32' (fp32 matrix path), or 'bf16x3' / 'bf16x2' / 'bf16' -- the split-bf16 GEMM with three / two / one
    bf16 part per operand (dh_conv_args.w_split = 1 / 3 / 4); split=True means 'bf16x3'.  A `packed` weight must have been
    packed for the same mode.  scope='extended': the mode's extended-scope code (w_split = 5 / 6 / 7, the same packing), which
    also takes a pointwise convolution with a BN prologue and K x K with Cin % 16 == 0 (dh_conv2d_split_wide_eligible)."""
    torch = _t()
    if x.dtype == torch.uint8:
        if in_lut is None or tuple(in_lut.shape) != (x.shape[-1], 256):
            raise ValueError('uint8 input needs in_lut of shape [Cin, 256]')
        if not x.is_cuda or not x.is_contiguous():
            raise ValueError('conv2d expects contiguous CUDA tensors')
        _chk(in_lut, pre_scale, pre_shift, post_scale, post_shift, res1, res2)
    else:
        _chk(x, pre_scale, pre_shift, post_scale, post_shift, res1, res2)
    lib = _lib.load()
    kh, kw, cin, cout = w_hwio.shape
    n, h, w_, c = x.shape
    if seg is not None:        # dh_conv2d_seg_f32: seg = (x2 or None, pool_sh): the input is [maxpool(x, strides (pool_sh, 2)) | x2]
        x2, pool_sh = seg
        _chk(x2)
        assert c + (x2.shape[-1] if x2 is not None else 0) == cin and h % pool_sh == 0 and w_ % 2 == 0
        h, w_ = h // pool_sh, w_ // 2
    else:
        assert c == cin
    if x_resample:             # dh_conv_args.x_resample: x is stored at half (1) / double (2, 3) the resolution the conv sees
        h, w_ = (2 * h, 2 * w_) if x_resample == 1 else (h // 2, w_ // 2)
    if padding == 'same':
        pt, _, oh = same_pad(h, kh, strides[0])
        pl, _, ow = same_pad(w_, kw, strides[1])
    else:
        pt = pl = 0
        oh, ow = (h - kh) // strides[0] + 1, (w_ - kw) // strides[1] + 1
    if precision not in (None, 'f32', 'bf16x3', 'bf16x2', 'bf16'):
        raise ValueError("precision must be 'f32', 'bf16x3', 'bf16x2' or 'bf16', got %r" % (precision,))
    if split and precision not in (None, 'bf16x3'):
        raise ValueError("split=True means precision='bf16x3', got precision=%r" % (precision,))
    if halo and precision not in (None, 'f32'):
        raise ValueError('the halo-resident kernel takes fp32 weights only')
    w_split = packing.LAYOUT_CODES['standard'].get(precision or ('bf16x3' if split else 'f32'), 0)
    if w_split and packed is None:
        pk, kp, np_ = packing.pack_conv_split(np.asarray(w_hwio, np.float32), parts=packing.SPLIT_PARTS[w_split])
        packed = (torch.from_numpy(pk).to(x.device), kp, np_)
    if halo and packed is None:                  # chunk-major fp32 packing for the halo-resident K x K kernel
        pk, kp, np_ = packing.pack_conv_halo(np.asarray(w_hwio, np.float32))
        packed = (torch.from_numpy(pk).to(x.device), kp, np_)
    wt, kp, np_ = packed if packed is not None else pack_conv_weight(w_hwio, x.device)
    up = 2 if up2 else 1
    y = torch.empty((n, oh * up, ow * up, cout), dtype=torch.float32, device=x.device)
    a = _lib.ConvArgs()
    if scope not in ('standard', 'extended'):
        raise ValueError("scope must be 'standard' or 'extended', got %r" % (scope,))
    if scope == 'extended' and w_split:
        w_split = packing.LAYOUT_CODES['extended'][packing.LAYOUT_MODE[w_split]]
    a.w_split = 2 if halo else w_split
    a.x, a.w, a.y = _p(x), _p(wt), _p(y)
    a.pre_scale, a.pre_shift, a.post_scale, a.post_shift = _p(pre_scale), _p(pre_shift), _p(post_scale), _p(post_shift)
    a.res1, a.res2 = _p(res1), _p(res2)
    a.N, a.H, a.W, a.Cin, a.ldx = n, h, w_, cin, c
    a.OH, a.OW, a.Cout, a.ldy = oh, ow, cout, cout
    a.KH, a.KW, a.SH, a.SW, a.PT, a.PL = kh, kw, strides[0], strides[1], pt, pl
    a.K, a.Kp, a.Np = kh * kw * cin, kp, np_
    a.ldr1 = res1.shape[-1] if res1 is not None else 0
    a.ldr2 = res2.shape[-1] if res2 is not None else 0
    a.pre_relu, a.post_relu, a.up2 = int(pre_relu), int(post_relu), int(up2)
    a.res2_down = int(res2_down)
    a.x_resample = int(x_resample)
    if x.dtype == torch.uint8:
        a.in_lut, a.x_u8 = _p(in_lut), 1
    yp = None
    if pool2:                                    # second output: MaxPooling2D((2, 2)) of y (dh_conv_args.y_pool)
        yp = torch.empty((n, oh // 2, ow // 2, cout), dtype=torch.float32, device=x.device)
        a.y_pool, a.ldyp = _p(yp), cout
    if seg is not None:
        sg = _lib.ConvSeg()
        if x2 is not None:
            sg.x2, sg.ldx2 = _p(x2), x2.shape[-1]
        sg.c_split, sg.pool_sh = c, pool_sh
        _lib.check(lib.dh_conv2d_seg_f32(C.byref(a), C.byref(sg), _stream()), 'dh_conv2d_seg_f32')
        return y
    _lib.check(lib.dh_conv2d_f32(C.byref(a), tile_cfg, _stream()), 'dh_conv2d_f32')
    return (y, yp) if pool2 else y


def normalize_u8(x, lut):
    """uint8 [.., C] -> float32 through lut [C,256] (dh_normalize_u8_f32)."""
    torch = _t()
    if x.dtype != torch.uint8 or not x.is_cuda or not x.is_contiguous():
        raise ValueError('normalize_u8 expects a contiguous CUDA uint8 tensor')
    _chk(lut)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dh_normalize_u8_f32(_p(x), _p(lut), _p(y), x.numel() // x.shape[-1], x.shape[-1],
                                               _stream()), 'dh_normalize_u8_f32')
    return y


def crop_resize(sources, jobs, out_hw, out=None, item_pitch=None, program='host'):
    """Crop-and-resize front end (dh_crop_resize_u8): every job in one launch on torch's current stream.
    sources: uint8 CUDA tensors [H, W, 3], rows contiguous (a row pitch above 3 W is fine: a column slice of a wider
    image); jobs: (source index, (x0, y0, x1, y1), hflip); out_hw = (OH, OW).  Returns uint8 [len(jobs), OH, OW, 3], bit for
    bit PIL's Image.crop(box).resize((OW, OH), BILINEAR) [mirrored].  `out`: a flat uint8 CUDA tensor to write into, item j
    at byte j * item_pitch (the op then returns `out`).  ValueError for a window more than 16 times its output.
    program='device': the crop program is built on the GPU (dh_crop_program_build_dev) from the uploaded source and job tables
    instead of on the host -- the same bytes, the same output; the per-job status is read back before the crop launch, which
    SYNCHRONISES the current stream (fine for an op; the pipelined front end does not read it), and any refused job raises the
    ValueError the host path raises, before anything is written."""
    torch = _t()
    lib = _lib.load()
    if program not in ('host', 'device'):
        raise ValueError("program must be 'host' or 'device', got %r" % (program,))
    OH, OW = int(out_hw[0]), int(out_hw[1])
    srcs = (_lib.CropSrc * len(sources))()
    for i, s in enumerate(sources):
        if not (s.is_cuda and s.dtype == torch.uint8 and s.dim() == 3 and s.shape[2] == 3 and s.stride(2) == 1 and s.stride(1) == 3):
            raise ValueError('crop_resize expects uint8 CUDA tensors [H, W, 3] with contiguous rows')
        srcs[i] = _lib.CropSrc(s.data_ptr(), s.stride(0), s.shape[0], s.shape[1])
    cj = (_lib.CropJob * len(jobs))(*[_lib.CropJob(int(s), int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(bool(f)))
                                      for s, b, f in jobs])
    nbytes = C.c_size_t(0)
    device = sources[0].device
    if program == 'device':
        what = 'dh_crop_program_build_dev'
        rc = lib.dh_crop_program_max_bytes(len(jobs), len(sources), OH, OW, C.byref(nbytes))
        if rc == 0:
            tables = [torch.from_numpy(np.frombuffer(bytes(t), np.uint8).copy()).to(device) for t in (srcs, cj)]
            prog_dev = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
            status = torch.empty(len(jobs), dtype=torch.int32, device=device)
            rc = lib.dh_crop_program_build_dev(tables[0].data_ptr(), len(sources), tables[1].data_ptr(), len(jobs), OH, OW,
                                               prog_dev.data_ptr(), nbytes.value, status.data_ptr(), _stream())
        if rc == 0:
            codes = status.cpu().numpy()                       # the synchronisation the docstring speaks of
            rc = -1 if np.any(codes == -1) else (-2 if np.any(codes == -2) else int(codes.min()))
    else:
        what = 'dh_crop_program_build_host'
        rc = lib.dh_crop_program_bytes(cj, len(jobs), len(sources), OH, OW, C.byref(nbytes))
        if rc == 0:
            prog = torch.empty(nbytes.value, dtype=torch.uint8, pin_memory=True)
            rc = lib.dh_crop_program_build_host(srcs, len(sources), cj, len(jobs), OH, OW, prog.data_ptr(), nbytes.value)
    if rc == -2:
        raise ValueError('crop_resize: a window is more than 16 times its output on one axis, or the output is too wide')
    if rc == -1:
        raise ValueError('crop_resize: bad argument (empty box, source index, row pitch below 3 W)')
    _lib.check(rc, what)
    if program == 'host':
        prog_dev = prog.to(device, non_blocking=True)
    if out is None:
        item_pitch = OH * OW * 3
        y = torch.empty((len(jobs), OH, OW, 3), dtype=torch.uint8, device=device)
    else:
        y = out
        if not (y.is_cuda and y.dtype == torch.uint8 and y.is_contiguous()) or item_pitch is None or \
                y.numel() < (len(jobs) - 1) * item_pitch + OH * OW * 3:
            raise ValueError('crop_resize: `out` must be a contiguous uint8 CUDA tensor holding every item at item_pitch')
    rc = lib.dh_crop_resize_u8(prog_dev.data_ptr(), len(jobs), OH, OW, y.data_ptr(), item_pitch, _stream())
    if rc == -2:
        raise ValueError('crop_resize: output rows of %d pixels do not fit the kernel' % OW)
    _lib.check(rc, 'dh_crop_resize_u8')
    prog_dev.record_stream(torch.cuda.current_stream())     # the launch reads the program after this function returns
    return y


def _refine_tables(boxes, jobs=None, src=None):
    torch = _t()
    if not (boxes.is_cuda and boxes.dtype == torch.float64 and boxes.dim() == 2 and boxes.shape[1] == 4 and boxes.is_contiguous()):
        raise ValueError('boxes must be a contiguous float64 CUDA tensor [n, 4]')
    n = boxes.shape[0]
    if jobs is not None and not (jobs.is_cuda and jobs.dtype == torch.int32 and tuple(jobs.shape) == (n, 6) and jobs.is_contiguous()):
        raise ValueError('jobs must be a contiguous int32 CUDA tensor [%d, 6] (src, x0, y0, x1, y1, hflip)' % n)
    if src is not None and not (src.is_cuda and src.dtype == torch.int32 and tuple(src.shape) == (n,) and src.is_contiguous()):
        raise ValueError('src must be a contiguous int32 CUDA tensor [%d]' % n)
    return n


def jobs_from_boxes(boxes, src, out=None):
    """Crop jobs from float boxes on the GPU (dh_jobs_from_boxes_f64): boxes float64 [n, 4], src int32 [n] (frame indices).
    Returns int32 [n, 6] rows (src, x0, y0, x1, y1, 0) with the window frontend.crop_box(*bbox_to_objposwin(b)) -- corners
    truncated toward zero; a box whose corners are not finite int32 values gives the empty job (src, 0, 0, 0, 0, 0)."""
    torch = _t()
    n = _refine_tables(boxes, src=src)
    jobs = torch.empty((n, 6), dtype=torch.int32, device=boxes.device) if out is None else out
    _refine_tables(boxes, jobs=jobs)
    rc = _lib.load().dh_jobs_from_boxes_f64(_p(boxes), _p(src), n, _p(jobs), _stream())
    if rc == -1:
        raise ValueError('jobs_from_boxes: bad argument (no samples)')
    _lib.check(rc, 'dh_jobs_from_boxes_f64')
    return jobs


def refine_boxes(poses, jobs, boxes, winsize_scale=1.5, momentum=0.8, out_boxes=None, out_jobs=None):
    """One pose -> box step of the box-refinement loop on the GPU (dh_refine_boxes_f64), on torch's current stream.
    poses: float32 CUDA [n, J, D >= 2] in crop-normalised coordinates, any sample and joint strides with a unit channel stride
    (a view of a plan's output is read where it lies); jobs int32 [n, 6]: the windows the poses were predicted in; boxes
    float64 [n, 4]: the float boxes those windows came from.  Returns (new boxes, new jobs); out_boxes / out_jobs may be the
    inputs themselves (in place)."""
    torch = _t()
    n = _refine_tables(boxes, jobs=jobs)
    if not (poses.is_cuda and poses.dtype == torch.float32 and poses.dim() == 3 and poses.shape[0] == n and poses.shape[2] >= 2 and
            (poses.stride(2) == 1)):
        raise ValueError('poses must be a float32 CUDA tensor [%d, J, D >= 2] with a unit channel stride' % n)
    nb = torch.empty_like(boxes) if out_boxes is None else out_boxes
    nj = torch.empty_like(jobs) if out_jobs is None else out_jobs
    _refine_tables(nb, jobs=nj)
    J = poses.shape[1]
    sample_stride = poses.stride(0) if n > 1 else max(poses.stride(0), (J - 1) * poses.stride(1) + 2)
    rc = _lib.load().dh_refine_boxes_f64(_p(poses), sample_stride, poses.stride(1) if J > 1 else max(poses.stride(1), 2), J,
                                         _p(jobs), _p(boxes), n, float(winsize_scale), float(momentum), _p(nb), _p(nj), _stream())
    if rc == -1:
        raise ValueError('refine_boxes: bad argument (no samples, no joints, or strides smaller than the extent they span)')
    _lib.check(rc, 'dh_refine_boxes_f64')
    return nb, nj


def pose_boxes(poses, windows, scale=1.5, conf_channel=None):
    """One person box per item from predicted poses on the GPU (dh_pose_boxes_f64), on torch's current stream: the device form
    of evaltools.bbox.get_bbox_from_poses.  poses: float32 CUDA [N, J, D >= 2] or [N, F, J, D] (an item of F frames) in
    crop-normalised coordinates, any item, frame and joint strides with a unit channel stride (a view of a plan's output is
    read where it lies); windows: the unflipped integer windows (x0, y0, x1, y1) the items were cropped with, [N, 4] (an int32
    CUDA tensor, or anything np.asarray takes).  conf_channel: None -- D - 2, the reference's poses[..., -2:-1].
    Returns (boxes int32 [N, 4], boxes float64 [N, 4], status int32 [N]) on the device; a non-zero status (1 a frame keeps no
    joint, 2 a kept joint is NaN, 3 a corner does not fit int32, 4 an empty window) leaves its boxes zero."""
    torch = _t()
    if not (poses.is_cuda and poses.dtype == torch.float32 and poses.dim() in (3, 4) and poses.shape[-1] >= 2 and
            poses.stride(-1) == 1):
        raise ValueError('poses must be a float32 CUDA tensor [N, (F,) J, D >= 2] with a unit channel stride')
    n, J, D = poses.shape[0], poses.shape[-2], poses.shape[-1]
    F = poses.shape[1] if poses.dim() == 4 else 1
    cc = D - 2 if conf_channel is None else int(conf_channel)
    if not 0 <= cc < D:
        raise ValueError('conf_channel %d outside the %d channels' % (cc, D))
    if not torch.is_tensor(windows):
        windows = torch.from_numpy(np.ascontiguousarray(windows, np.int32)).to(poses.device)
    if not (windows.is_cuda and windows.dtype == torch.int32 and tuple(windows.shape) == (n, 4)):
        raise ValueError('windows must be int32 [%d, 4] (x0, y0, x1, y1)' % n)
    jobs = torch.zeros((n, 6), dtype=torch.int32, device=poses.device)
    jobs[:, 1:5] = windows
    boxes = torch.empty((n, 4), dtype=torch.int32, device=poses.device)
    boxes_f = torch.empty((n, 4), dtype=torch.float64, device=poses.device)
    status = torch.empty((n,), dtype=torch.int32, device=poses.device)
    ext = max(2, cc + 1)                          # (torch gives a dimension of size 1 any stride: take the extent it spans)
    js = poses.stride(-2) if J > 1 else max(poses.stride(-2), ext)
    fs = (J - 1) * js + ext
    if F > 1:
        fs = poses.stride(1)
    its = poses.stride(0) if n > 1 else max(poses.stride(0), (F - 1) * fs + (J - 1) * js + ext)
    if F == 1:
        fs = its
    rc = _lib.load().dh_pose_boxes_f64(_p(poses), its, fs, js, F, J, cc, _p(jobs), 1, n, float(scale), _p(boxes), _p(boxes_f),
                                       _p(status), _stream())
    if rc == -1:
        raise ValueError('pose_boxes: bad argument (no items, no joints, or strides smaller than the extent they span)')
    _lib.check(rc, 'dh_pose_boxes_f64')
    return boxes, boxes_f, status


def vote_sources(probs, n, C):
    """The dh_vote_src table of `probs` -- float32 CUDA tensors [n, C] with a unit class stride, any row stride (a view of a
    plan's output is read where it lies) -- as a ctypes array."""
    torch = _t()
    srcs = (_lib.VoteSrc * len(probs))()
    for b, p in enumerate(probs):
        if not (torch.is_tensor(p) and p.is_cuda and p.dtype == torch.float32 and tuple(p.shape) == (n, C) and
                (C == 1 or p.stride(1) == 1)):
            raise ValueError('probs[%d] must be a float32 CUDA tensor [%d, %d] with a unit class stride' % (b, n, C))
        srcs[b].p = p.data_ptr()
        srcs[b].item_stride = p.stride(0) if n > 1 else max(p.stride(0), C)   # (torch gives a dimension of size 1 any stride)
    return srcs


def vote_products(probs, seq, nseq, acc=None, keep_scores=False):
    """The multi-clip action vote on the GPU (dh_vote_products_f64), on torch's current stream: the device form of
    evaltools.action.vote_products.  probs: a list of nb float32 CUDA tensors [n, C] (one per action output; row k is item k's
    class probabilities; any row stride); seq: the sequence of every item, [n] (an int32 CUDA tensor, or anything np.asarray
    takes); acc: the running products float64 CUDA [nb, nseq, C], multiplied IN PLACE (None: ones).  For k in order,
    acc[b, seq[k]] *= probs[b][k] and label[b, k] = np.argmax(acc[b, seq[k]]); an item with seq[k] outside [0, nseq) is skipped
    with label -1.  Returns (acc, label int32 [nb, n]) and, with keep_scores, scores float32 [nb, n, C], on the device."""
    torch = _t()
    probs = list(probs)
    if not probs or not torch.is_tensor(probs[0]) or probs[0].dim() != 2:
        raise ValueError('probs must be a non-empty list of float32 CUDA tensors [n, C]')
    n, C = (int(v) for v in probs[0].shape)
    nb, nseq, dev = len(probs), int(nseq), probs[0].device
    srcs = vote_sources(probs, n, C)
    if not torch.is_tensor(seq):
        seq = torch.from_numpy(np.ascontiguousarray(seq, np.int32)).to(dev)
    if not (seq.is_cuda and seq.dtype == torch.int32 and tuple(seq.shape) == (n,) and seq.is_contiguous()):
        raise ValueError('seq must be int32 [%d]' % n)
    if nseq < 1:
        raise ValueError('nseq must be positive')
    if acc is None:
        acc = torch.ones((nb, nseq, C), dtype=torch.float64, device=dev)
    if not (acc.is_cuda and acc.dtype == torch.float64 and tuple(acc.shape) == (nb, nseq, C) and acc.is_contiguous()):
        raise ValueError('acc must be a contiguous float64 CUDA tensor [%d, %d, %d]' % (nb, nseq, C))
    label = torch.empty((nb, n), dtype=torch.int32, device=dev)
    scores = torch.empty((nb, n, C), dtype=torch.float32, device=dev) if keep_scores else None
    rc = _lib.load().dh_vote_products_f64(srcs, nb, C, _p(seq), n, nseq, _p(acc), _p(label), _p(scores), _stream())
    if rc == -1:
        raise ValueError('vote_products: bad argument (no items, no classes, or a row stride smaller than the classes)')
    _lib.check(rc, 'dh_vote_products_f64')
    return (acc, label, scores) if keep_scores else (acc, label)


def dwconv2d(x, dw_kernel, pre_scale=None, pre_shift=None, pre_relu=False, up_in=False):
    """Depthwise conv, stride 1, TF-SAME.  dw_kernel numpy [kh,kw,C,1].  up_in: x is at half resolution and the
    convolution runs on UpSampling2D((2, 2))(x) without writing it out (dh_dw_args.up_in)."""
    torch = _t()
    _chk(x, pre_scale, pre_shift)
    lib = _lib.load()
    kh, kw, c, _ = dw_kernel.shape
    n, h, w_, cx = x.shape
    assert cx == c
    if up_in:
        h, w_ = 2 * h, 2 * w_
    pt, _, _ = same_pad(h, kh, 1)
    pl, _, _ = same_pad(w_, kw, 1)
    wt = torch.from_numpy(np.ascontiguousarray(dw_kernel.reshape(kh * kw, c), np.float32)).to(x.device)
    y = torch.empty((n, h, w_, c), dtype=torch.float32, device=x.device)
    a = _lib.DwArgs()
    a.x, a.w, a.y, a.pre_scale, a.pre_shift = _p(x), _p(wt), _p(y), _p(pre_scale), _p(pre_shift)
    a.N, a.H, a.W, a.C, a.ldx, a.ldy = n, h, w_, c, c, c
    a.KH, a.KW, a.PT, a.PL, a.pre_relu, a.up_in = kh, kw, pt, pl, int(pre_relu), int(up_in)
    _lib.check(lib.dh_dwconv2d_f32(C.byref(a), _stream()), 'dh_dwconv2d_f32')
    return y


def dwconv2d_strided(x, dw_kernel, strides=(2, 2), pre_scale=None, pre_shift=None, pre_relu=False, channels=None, out=None):
    """Depthwise conv at a stride, TF-SAME (dh_dwconv2d_strided_f32: the depthwise half of SeparableConv2D(strides=(2, 2))).
    dw_kernel numpy [kh,kw,C,1].  channels: x is [N,H,W,ldx] with ldx >= C and only its first C channels are read;
    out: a preallocated [N,OH,OW,ldy] tensor (ldy >= C) whose first C channels are written."""
    torch = _t()
    _chk(x, pre_scale, pre_shift, out)
    lib = _lib.load()
    kh, kw, c, _ = dw_kernel.shape
    n, h, w_, ldx = x.shape
    assert (channels or ldx) == c
    pt, _, oh = same_pad(h, kh, strides[0])
    pl, _, ow = same_pad(w_, kw, strides[1])
    wt = torch.from_numpy(np.ascontiguousarray(dw_kernel.reshape(kh * kw, c), np.float32)).to(x.device)
    y = out if out is not None else torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    assert tuple(y.shape[:3]) == (n, oh, ow) and y.shape[3] >= c
    a = _lib.DwsArgs()
    a.x, a.w, a.y, a.pre_scale, a.pre_shift = _p(x), _p(wt), _p(y), _p(pre_scale), _p(pre_shift)
    a.N, a.H, a.W, a.C, a.ldx, a.ldy = n, h, w_, c, ldx, y.shape[3]
    a.OH, a.OW = oh, ow
    a.KH, a.KW, a.SH, a.SW, a.PT, a.PL, a.pre_relu = kh, kw, strides[0], strides[1], pt, pl, int(pre_relu)
    _lib.check(lib.dh_dwconv2d_strided_f32(C.byref(a), _stream()), 'dh_dwconv2d_strided_f32')
    return y


def pack_convt_weight(w, device='cuda', parts=None):
    """Keras Conv2DTranspose kernel [2,2,Cout,Cin] (numpy) -> (packed device tensor, Kp, Np) for conv2d_transpose.
    parts = 3 / 2 / 1: the split-bf16 packing of precision = 'bf16x3' / 'bf16x2' / 'bf16'; None: fp32."""
    torch = _t()
    packed, kp, np_ = packing.pack_convt(np.asarray(w, np.float32), parts=parts)
    return torch.from_numpy(packed).to(device), kp, np_


def conv2d_transpose(x, w, strides=(2, 2), pre_scale=None, pre_shift=None, pre_relu=False, res=None, post_relu=False,
                     tile_cfg=-1, packed=None, channels=None, out=None, precision=None):
    """Conv2DTranspose((2, 2), strides=(2, 2), use_bias=False) with the fused BN / ReLU prologue and residual / ReLU
    epilogue of dh_conv2d_transpose2x2_f32.  x [N,H,W,Cin]; w numpy, Keras layout [2,2,Cout,Cin]; res [N,2H,2W,ldr] at the
    OUTPUT resolution.  channels: x is [N,H,W,ldx] and only its first Cin channels are read; out: a preallocated
    [N,2H,2W,ldy] tensor whose first Cout channels are written.
    precision: None / 'f32' (fp32 matrix path), or 'bf16x3' / 'bf16x2' / 'bf16' -- the split-bf16 form with three / two / one
    bf16 part per operand (dh_conv2d_transpose2x2_split_f32; tile_cfg then indexes its tilings).  A `packed` weight must have
    been packed for the same mode (pack_convt_weight(..., parts=...))."""
    if precision not in (None, 'f32', 'bf16x3', 'bf16x2', 'bf16'):
        raise ValueError("precision must be 'f32', 'bf16x3', 'bf16x2' or 'bf16', got %r" % (precision,))
    parts = packing.MODE_PARTS.get(precision)
    torch = _t()
    kh, kw, cout, cin = w.shape
    if (kh, kw) != (2, 2) or tuple(strides) != (2, 2):
        raise NotImplementedError('conv2d_transpose is built for kernel_size=(2, 2), strides=(2, 2) only')
    _chk(x, pre_scale, pre_shift, res, out)
    lib = _lib.load()
    n, h, w_, ldx = x.shape
    assert (channels or ldx) == cin
    wt, kp, np_ = packed if packed is not None else pack_convt_weight(w, x.device, parts=parts)
    y = out if out is not None else torch.empty((n, 2 * h, 2 * w_, cout), dtype=torch.float32, device=x.device)
    assert tuple(y.shape[:3]) == (n, 2 * h, 2 * w_) and y.shape[3] >= cout
    a = _lib.ConvtArgs()
    a.x, a.w, a.y, a.pre_scale, a.pre_shift, a.res = _p(x), _p(wt), _p(y), _p(pre_scale), _p(pre_shift), _p(res)
    a.N, a.H, a.W, a.Cin, a.ldx = n, h, w_, cin, ldx
    a.Cout, a.ldy, a.ldr = cout, y.shape[3], res.shape[-1] if res is not None else 0
    a.Kp, a.Np, a.pre_relu, a.post_relu = kp, np_, int(pre_relu), int(post_relu)
    if parts is not None:
        _lib.check(lib.dh_conv2d_transpose2x2_split_f32(C.byref(a), parts, tile_cfg, _stream()),
                   'dh_conv2d_transpose2x2_split_f32')
        return y
    _lib.check(lib.dh_conv2d_transpose2x2_f32(C.byref(a), tile_cfg, _stream()), 'dh_conv2d_transpose2x2_f32')
    return y


def pool2d(x, pool=(2, 2), strides=None, padding='valid', mode=0):
    torch = _t()
    _chk(x)
    lib = _lib.load()
    strides = strides or pool
    n, h, w_, c = x.shape
    if padding == 'same':
        pt, _, oh = same_pad(h, pool[0], strides[0])
        pl, _, ow = same_pad(w_, pool[1], strides[1])
    else:
        pt = pl = 0
        oh, ow = (h - pool[0]) // strides[0] + 1, (w_ - pool[1]) // strides[1] + 1
    y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    a = _lib.PoolArgs()
    a.x, a.y = _p(x), _p(y)
    a.N, a.H, a.W, a.C, a.ldx, a.OH, a.OW, a.ldy = n, h, w_, c, c, oh, ow, c
    a.KH, a.KW, a.SH, a.SW, a.PT, a.PL, a.mode = pool[0], pool[1], strides[0], strides[1], pt, pl, mode
    _lib.check(lib.dh_pool2d_f32(C.byref(a), _stream()), 'dh_pool2d_f32')
    return y


def upsample2x_add(b, a=None):
    torch = _t()
    _chk(a, b)
    n, h, w_, c = b.shape
    y = torch.empty((n, 2 * h, 2 * w_, c), dtype=torch.float32, device=b.device)
    _lib.check(_lib.load().dh_upsample2x_add_f32(_p(a), c, _p(b), c, _p(y), c, n, 2 * h, 2 * w_, c, _stream()),
               'dh_upsample2x_add_f32')
    return y


def softargmax2d(h, alpha=1.0, conf_scale=1.0, want_prob=False):
    """Returns dict(xy [F,C,2], conf_raw [F,C,1], conf_prob [F,C,1], gmax [F,C], prob [F,H,W,C] | None)."""
    torch = _t()
    _chk(h)
    f, hh, ww, c = h.shape
    dev = h.device
    out = dict(xy=torch.empty((f, c, 2), device=dev), conf_raw=torch.empty((f, c, 1), device=dev),
               conf_prob=torch.empty((f, c, 1), device=dev), gmax=torch.empty((f, c), device=dev),
               prob=torch.empty_like(h) if want_prob else None)
    gx = torch.from_numpy(grid_x(ww)).to(dev)
    gy = torch.from_numpy(grid_x(hh)).to(dev)
    a = _lib.SamArgs()
    a.h, a.gx, a.gy = _p(h), _p(gx), _p(gy)
    a.xy, a.conf_raw, a.conf_prob, a.prob, a.gmax = (_p(out['xy']), _p(out['conf_raw']), _p(out['conf_prob']),
                                                     _p(out['prob']), _p(out['gmax']))
    a.F, a.H, a.W, a.C, a.ldh, a.ldxy, a.ldcr, a.ldcp, a.ldp = f, hh, ww, c, c, 2, 1, 1, c
    a.alpha, a.conf_scale = float(alpha), float(conf_scale)
    _lib.check(_lib.load().dh_softargmax2d_f32(C.byref(a), _stream()), 'dh_softargmax2d_f32')
    torch.cuda.current_stream().synchronize()  # gx/gy are temporaries
    return out


def softargmax2d_context(h, joints, num_context, agg_alpha, alpha=1.0, conf_scale=1.0, pitch=None):
    """dh_softargmax2d_context_f32: h [F, H, W, >= J*(1+nctx)] (channel pitch = h.shape[-1], the first J*(1+nctx)
    channels are read) -> (pose [F, J, 2], joint confidences [F, J, 1])."""
    torch = _t()
    _chk(h)
    f, hh, ww, ld = h.shape
    dev = h.device
    y = torch.empty((f, joints, 2), device=dev)
    conf = torch.empty((f, joints, 1), device=dev)
    gx = torch.from_numpy(grid_x(ww)).to(dev)
    gy = torch.from_numpy(grid_x(hh)).to(dev)
    a = _lib.SamArgs()
    a.h, a.gx, a.gy, a.conf_raw = _p(h), _p(gx), _p(gy), _p(conf)
    a.F, a.H, a.W, a.C, a.ldh, a.ldcr = f, hh, ww, joints * (1 + num_context), ld, 1
    a.alpha, a.conf_scale = float(alpha), float(conf_scale)
    _lib.check(_lib.load().dh_softargmax2d_context_f32(C.byref(a), joints, num_context, float(agg_alpha), _p(y), 2,
                                                       _stream()), 'dh_softargmax2d_context_f32')
    torch.cuda.current_stream().synchronize()  # gx/gy are temporaries
    return y, conf


def context_aggregation(ys, yc, pc, num_context, alpha):
    torch = _t()
    _chk(ys, yc, pc)
    f, j, _ = ys.shape
    y = torch.empty_like(ys)
    _lib.check(_lib.load().dh_context_aggregation_f32(_p(ys), _p(yc), _p(pc), _p(y), f, j, num_context,
                                                      float(alpha), 2, _stream()), 'dh_context_aggregation_f32')
    return y


def depth_means(h, depth, joints):
    torch = _t()
    _chk(h)
    f, hh, ww, c = h.shape
    assert c == depth * joints
    hxy = torch.empty((f, hh, ww, joints), device=h.device)
    hz = torch.empty((f, depth, joints), device=h.device)
    _lib.check(_lib.load().dh_depth_means_f32(_p(h), c, _p(hxy), _p(hz), f, hh * ww, depth, joints, _stream()),
               'dh_depth_means_f32')
    return hxy, hz


def softargmax1d(hz):
    torch = _t()
    _chk(hz)
    f, d, j = hz.shape
    z = torch.empty((f, j, 1), device=hz.device)
    vz = torch.empty((f, j), device=hz.device)
    grid = torch.from_numpy(grid_depth(d)).to(hz.device)
    _lib.check(_lib.load().dh_softargmax1d_f32(_p(hz), _p(grid), _p(z), 1, _p(vz), f, d, j, _stream()),
               'dh_softargmax1d_f32')
    torch.cuda.current_stream().synchronize()
    return z, vz


def kronecker(hm, x, out_pitch=None):
    """layers.kronecker_prod.  `out_pitch` > C writes the rows into a wider (packed) buffer, as a plan does."""
    torch = _t()
    _chk(hm, x)
    b, hh, ww, j = hm.shape
    c = x.shape[-1]
    ld = c if out_pitch is None else int(out_pitch)
    f = torch.zeros((b, j, ld), device=hm.device)
    _lib.check(_lib.load().dh_kronecker_f32(_p(hm), j, _p(x), c, _p(f), ld, b, hh * ww, j, c, _stream()),
               'dh_kronecker_f32')
    return f if ld == c else f[..., :c]


def global_maxmin_softmax(x, softmax=True):
    torch = _t()
    _chk(x)
    b, t, j, c = x.shape
    y = torch.empty((b, c), device=x.device)
    _lib.check(_lib.load().dh_global_maxmin_softmax_f32(_p(x), c, _p(y), b, t * j, c, int(softmax), _stream()),
               'dh_global_maxmin_softmax_f32')
    return y
