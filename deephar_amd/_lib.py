"""ctypes binding of libdeephar_hip.so (the C-ABI declared in include/deephar_hip.h).

The product path has no CPU fallback: if the shared library is missing this module raises, loudly.
Build it with `python -m deephar_amd.csrc.build` (or __graft_entry__.build()).
"""
import ctypes as C
import itertools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libdeephar_hip.so')

c_f = C.POINTER(C.c_float)
i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p


class ConvArgs(C.Structure):
    _fields_ = [(n, vp) for n in ('x', 'w', 'y', 'pre_scale', 'pre_shift', 'post_scale', 'post_shift',
                                   'res1', 'res2', 'in_lut')] + \
               [(n, i32) for n in ('N', 'H', 'W', 'Cin', 'ldx', 'OH', 'OW', 'Cout', 'ldy', 'KH', 'KW', 'SH',
                                   'SW', 'PT', 'PL', 'K', 'Kp', 'Np', 'ldr1', 'ldr2', 'pre_relu', 'post_relu',
                                   'up2', 'x_u8', 'w_split', 'res2_down', 'ldyp', 'x_resample')] + [('y_pool', vp)]


class ConvSeg(C.Structure):                      # == struct dh_conv_seg
    _fields_ = [('x2', vp)] + [(n, i32) for n in ('ldx2', 'c_split', 'pool_sh', 'reserved')]


class DwArgs(C.Structure):
    _fields_ = [(n, vp) for n in ('x', 'w', 'y', 'pre_scale', 'pre_shift')] + \
               [(n, i32) for n in ('N', 'H', 'W', 'C', 'ldx', 'ldy', 'KH', 'KW', 'PT', 'PL', 'pre_relu', 'up_in')]


class DwsArgs(C.Structure):                      # == struct dh_dw_strided
    _fields_ = [(n, vp) for n in ('x', 'w', 'y', 'pre_scale', 'pre_shift')] + \
               [(n, i32) for n in ('N', 'H', 'W', 'C', 'ldx', 'ldy', 'OH', 'OW', 'KH', 'KW', 'SH', 'SW', 'PT', 'PL',
                                   'pre_relu', 'reserved')]


class ConvtArgs(C.Structure):                    # == struct dh_conv_transpose
    _fields_ = [(n, vp) for n in ('x', 'w', 'y', 'pre_scale', 'pre_shift', 'res')] + \
               [(n, i32) for n in ('N', 'H', 'W', 'Cin', 'ldx', 'Cout', 'ldy', 'ldr', 'Kp', 'Np', 'pre_relu', 'post_relu')]


class PoolArgs(C.Structure):
    _fields_ = [(n, vp) for n in ('x', 'y')] + \
               [(n, i32) for n in ('N', 'H', 'W', 'C', 'ldx', 'OH', 'OW', 'ldy', 'KH', 'KW', 'SH', 'SW', 'PT',
                                   'PL', 'mode')]


class EltArgs(C.Structure):
    _fields_ = [(n, vp) for n in ('a', 'b', 'c', 'y', 'scale', 'shift')] + \
               [(n, i32) for n in ('lda', 'ldb', 'ldc', 'ldy')] + [('npix', i64)] + \
               [(n, i32) for n in ('C', 'relu', 'op', 'bcast_b')]


class SamArgs(C.Structure):
    _fields_ = [(n, vp) for n in ('h', 'gx', 'gy', 'xy', 'conf_raw', 'conf_prob', 'prob', 'gmax')] + \
               [(n, i32) for n in ('F', 'H', 'W', 'C', 'ldh', 'ldxy', 'ldcr', 'ldcp', 'ldp')] + \
               [('alpha', C.c_float), ('conf_scale', C.c_float), ('xy_times_conf', i32)]


class ConvRoute(C.Structure):                    # == struct dh_conv_route: what dh_conv2d_f32 will do (dh_conv2d_route)
    _fields_ = [(n, i32) for n in ('rc', 'kernel', 'tile_cfg', 'parts', 'bm', 'bn', 'tm', 'vec4', 'epi', 'pool')] + \
               [('tiles', C.c_uint32)]


class SamRoute(C.Structure):                     # == struct dh_sam_route (dh_softargmax2d_route)
    _fields_ = [(n, i32) for n in ('rc', 'channels', 'staged', 'ctx_rc')]


class CutSeg(C.Structure):                       # == struct dh_cut_seg (dh_unpack_cut_f32)
    _fields_ = [('dst', vp)] + [(n, i32) for n in ('ld', 'coff', 'c', 'pad')]


class OutSeg(C.Structure):                       # == struct dh_out_seg (dh_pack_outputs_f32)
    _fields_ = [('src', vp), ('dst', vp), ('npix', i64), ('C', i32), ('ld', i32)]


class CropSrc(C.Structure):                      # == struct dh_crop_src (dh_crop_program_build_host)
    _fields_ = [('ptr', vp), ('pitch', i64), ('H', i32), ('W', i32)]


class CropJob(C.Structure):                      # == struct dh_crop_job
    _fields_ = [(n, i32) for n in ('src', 'x0', 'y0', 'x1', 'y1', 'hflip')]


class VoteSrc(C.Structure):                      # == struct dh_vote_src (dh_vote_products_f64)
    _fields_ = [('p', vp), ('item_stride', i64)]


class SchedOp(C.Structure):                    # == struct dh_sched_op (dh_sched_build_ops)
    _fields_ = [(n, i32) for n in ('kind', 'stream', 'arg', 'entry')]


SCHED_LAUNCH, SCHED_RECORD, SCHED_WAIT = range(3)    # dh_sched_op.kind


class ClipInfo(C.Structure):                     # == struct dh_clip_info (dh_clip_inspect)
    _fields_ = [(n, i32) for n in ('version', 'world', 'T', 'Tl', 'packed_channels', 'num_cut', 'num_outputs',
                                   'num_head_outputs')] + [('P', i64)] + \
               [(n, C.c_uint64) for n in ('frames_offset', 'frames_bytes', 'head_offset', 'head_bytes')]


class PlanInfo(C.Structure):                     # == struct dh_plan_info (dh_plan_inspect)
    _fields_ = [(n, i32) for n in ('version', 'batch', 'num_inputs', 'num_outputs', 'num_steps', 'nstreams', 'num_ops',
                                   'num_events')] + [(n, C.c_uint64) for n in ('arena_bytes', 'weight_bytes', 'byte_bytes')]


# dh_allgather_fn: (ctx, send, recv, floats per rank, stream) -> 0 on success
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, vp, vp, vp, i64, vp)


# dh_conv_route.kernel
CONV_GENERAL, CONV_DMA, CONV_SPLIT, CONV_SPLIT_EXT, CONV_HALO, CONV_SKINNY, CONV_FIRST_LAYER = range(1, 8)


def conv_route(lib, args, tile_cfg=-1):
    """dh_conv2d_route as a ConvRoute."""
    r = ConvRoute()
    assert lib.dh_conv2d_route(C.byref(args), tile_cfg, C.byref(r)) == 0
    return r


def sam_route(lib, args, J=0, nctx=0):
    """dh_softargmax2d_route as a SamRoute."""
    r = SamRoute()
    assert lib.dh_softargmax2d_route(C.byref(args), J, nctx, C.byref(r)) == 0
    return r


def plan_record(lib, fn):
    """dh_plan_record as (entry point name, first blob version, payload bytes, [pointer offsets]); None outside the table."""
    name, first, size, n = C.c_char_p(), C.c_int(), C.c_size_t(), C.c_int()
    offs = (i32 * 32)()
    if lib.dh_plan_record(fn, C.byref(name), C.byref(first), C.byref(size), offs, len(offs), C.byref(n)) != 0:
        return None
    assert n.value <= len(offs)
    return name.value.decode(), first.value, size.value, list(offs[:n.value])


def sched_program(lib, entries, nstreams, npre):
    """dh_sched_build_ops over a schedule table (engine/schedule.py: schedule_entries) as ([(kind, stream, arg, entry)],
    number of events); a table the library refuses -- more than 4 streams, for one -- raises DeepharHipError."""
    col = lambda vals: (i32 * (len(vals) + 1))(*vals)
    waits = [w for e in entries for w in e[3]]
    offs = list(itertools.accumulate([len(e[3]) for e in entries], initial=0))
    args = (len(entries), col([-1 if e[0] is None else e[0] for e in entries]), col([e[1] for e in entries]),
            col([e[2] for e in entries]), col(offs), col(waits), len(waits), nstreams, npre, sum(e[0] is not None for e in entries))
    what = 'enqueue program of %d calls on %d streams (a plan has at most 4 streams)' % (len(entries), nstreams)
    n, nev = C.c_int(), C.c_int()
    check(lib.dh_sched_build_ops(*args, None, 0, C.byref(n), C.byref(nev)), what)
    ops = (SchedOp * (n.value + 1))()
    check(lib.dh_sched_build_ops(*args, ops, n.value, C.byref(n), C.byref(nev)), what)
    return [(o.kind, o.stream, o.arg, o.entry) for o in ops[:n.value]], nev.value


# name -> (restype, argtypes); every symbol include/deephar_hip.h declares
SIGNATURES = {
    'dh_version': (C.c_int, []),
    'dh_error_string': (C.c_char_p, [C.c_int]),
    'dh_device_info': (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    'dh_conv2d_packed_dims': (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2),
    'dh_conv2d_pack_weights_host': (C.c_int, [vp, vp] + [C.c_int] * 4),
    'dh_conv2d_pack_weights_split_host': (C.c_int, [vp, vp] + [C.c_int] * 4),
    'dh_conv2d_pack_weights_parts_host': (C.c_int, [vp, vp] + [C.c_int] * 5),
    'dh_conv2d_num_tile_cfgs': (C.c_int, []),
    'dh_conv2d_num_split_tile_cfgs': (C.c_int, []),
    'dh_conv2d_pick_tile_cfg': (C.c_int, [C.c_int, C.c_int]),
    'dh_conv2d_uses_split_k': (C.c_int, [C.POINTER(ConvArgs)]),
    'dh_conv2d_uses_first_layer_kernel': (C.c_int, [C.POINTER(ConvArgs)]),
    'dh_conv2d_split_eligible': (C.c_int, [C.POINTER(ConvArgs)]),
    'dh_conv2d_split_wide_eligible': (C.c_int, [C.POINTER(ConvArgs)]),
    'dh_conv2d_halo_eligible': (C.c_int, [C.POINTER(ConvArgs)]),
    'dh_conv2d_num_halo_tile_cfgs': (C.c_int, []),
    'dh_conv2d_route': (C.c_int, [C.POINTER(ConvArgs), C.c_int, C.POINTER(ConvRoute)]),
    'dh_conv2d_f32': (C.c_int, [C.POINTER(ConvArgs), C.c_int, vp]),
    'dh_normalize_u8_f32': (C.c_int, [vp, vp, vp, C.c_int64, C.c_int, vp]),
    'dh_dwconv2d_f32': (C.c_int, [C.POINTER(DwArgs), vp]),
    'dh_dwconv2d_uses_lds_kernel': (C.c_int, [C.POINTER(DwArgs)]),
    'dh_dwconv2d_strided_f32': (C.c_int, [C.POINTER(DwsArgs), vp]),
    'dh_conv2d_transpose2x2_num_tile_cfgs': (C.c_int, []),
    'dh_conv2d_transpose2x2_f32': (C.c_int, [C.POINTER(ConvtArgs), C.c_int, vp]),
    'dh_conv2d_transpose2x2_num_split_tile_cfgs': (C.c_int, []),
    'dh_conv2d_transpose2x2_split_eligible': (C.c_int, [C.POINTER(ConvtArgs)]),
    'dh_conv2d_transpose2x2_split_f32': (C.c_int, [C.POINTER(ConvtArgs), C.c_int, C.c_int, vp]),
    'dh_conv2d_dw_group_f32': (C.c_int, [C.POINTER(ConvArgs), C.POINTER(DwArgs), vp]),
    'dh_conv2d_pair_f32': (C.c_int, [C.POINTER(ConvArgs), C.POINTER(ConvArgs), vp]),
    'dh_conv2d_seg_f32': (C.c_int, [C.POINTER(ConvArgs), C.POINTER(ConvSeg), vp]),
    'dh_pool2d_f32': (C.c_int, [C.POINTER(PoolArgs), vp]),
    'dh_upsample2x_add_f32': (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int] + [C.c_int] * 4 + [vp]),
    'dh_eltwise_f32': (C.c_int, [C.POINTER(EltArgs), vp]),
    'dh_softargmax2d_f32': (C.c_int, [C.POINTER(SamArgs), vp]),
    'dh_softargmax2d_context_f32': (C.c_int, [C.POINTER(SamArgs), C.c_int, C.c_int, C.c_float, vp, C.c_int, vp]),
    'dh_softargmax2d_route': (C.c_int, [C.POINTER(SamArgs), C.c_int, C.c_int, C.POINTER(SamRoute)]),
    'dh_context_aggregation_f32': (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp]),
    'dh_depth_means_f32': (C.c_int, [vp, C.c_int, vp, vp] + [C.c_int] * 4 + [vp]),
    'dh_softargmax1d_f32': (C.c_int, [vp, vp, vp, C.c_int, vp] + [C.c_int] * 3 + [vp]),
    'dh_kronecker_f32': (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int] + [C.c_int] * 4 + [vp]),
    'dh_global_maxmin_softmax_f32': (C.c_int, [vp, C.c_int, vp] + [C.c_int] * 4 + [vp]),
    'dh_copy_channels_f32': (C.c_int, [vp, C.c_int, vp, C.c_int, i64, C.c_int, vp]),
    'dh_zeropad2d_f32': (C.c_int, [vp, vp] + [C.c_int] * 8 + [vp]),
    'dh_depth_from_maps_f32': (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int] + [C.c_int] * 3 + [vp]),
    'dh_plan_create': (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    'dh_plan_destroy': (C.c_int, [vp]),
    'dh_plan_batch': (C.c_int, [vp]),
    'dh_plan_num_inputs': (C.c_int, [vp]),
    'dh_plan_num_outputs': (C.c_int, [vp]),
    'dh_plan_input_items': (C.c_int64, [vp, C.c_int]),
    'dh_plan_input_is_u8': (C.c_int, [vp, C.c_int]),
    'dh_plan_output_items': (C.c_int64, [vp, C.c_int]),
    'dh_forward': (C.c_int, [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), vp]),
    'dh_forward_host': (C.c_int, [vp, C.POINTER(vp), C.c_int, C.POINTER(vp)]),
    'dh_plan_input_ptr': (vp, [vp, C.c_int]),
    'dh_plan_num_streams': (C.c_int, [vp]),
    'dh_plan_side_stream': (vp, [vp, C.c_int]),
    'dh_plan_inspect': (C.c_int, [vp, C.c_size_t, C.POINTER(PlanInfo)]),
    'dh_plan_record': (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(i32), C.c_int,
                                 C.POINTER(C.c_int)]),
    'dh_pack_outputs_f32': (C.c_int, [C.POINTER(OutSeg), C.c_int, vp]),
    'dh_pack_outputs_host': (C.c_int, [C.POINTER(OutSeg), C.c_int]),
    'dh_pack_outputs_vec4': (C.c_int, [C.c_int, C.c_int, vp, vp]),
    'dh_crop_program_bytes': (C.c_int, [C.POINTER(CropJob), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    'dh_crop_program_build_host': (C.c_int, [C.POINTER(CropSrc), C.c_int, C.POINTER(CropJob), C.c_int, C.c_int, C.c_int, vp,
                                             C.c_size_t]),
    'dh_crop_resize_u8': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, i64, vp]),
    'dh_crop_resize_host': (C.c_int, [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, i64]),
    'dh_crop_axis_taps': (C.c_int, [C.c_int, C.c_int]),
    'dh_crop_axis_coeffs_host': (C.c_int, [C.c_int] * 3 + [C.POINTER(i32)] * 3),
    'dh_crop_program_max_bytes': (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    'dh_crop_program_build_dev': (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]),
    'dh_frames_create': (C.c_int, [C.POINTER(CropSrc), C.c_int, C.POINTER(vp)]),
    'dh_frames_destroy': (C.c_int, [vp]),
    'dh_frames_count': (C.c_int, [vp]),
    'dh_frames_table_dev': (vp, [vp]),
    'dh_forward_frames_shape': (C.c_int, [C.c_int, C.c_int, i64] + [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2),
    'dh_forward_frames': (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), vp]),
    'dh_forward_frames_host': (C.c_int, [vp, vp, C.POINTER(CropJob), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    'dh_plan_output_channels': (C.c_int, [vp, C.c_int]),
    'dh_jobs_from_boxes_f64': (C.c_int, [vp, vp, C.c_int, vp, vp]),
    'dh_jobs_from_boxes_host': (C.c_int, [vp, vp, C.c_int, vp]),
    'dh_refine_boxes_f64': (C.c_int, [vp, i64, i64, C.c_int, vp, vp, C.c_int, C.c_double, C.c_double, vp, vp, vp]),
    'dh_refine_boxes_host': (C.c_int, [vp, i64, i64, C.c_int, vp, vp, C.c_int, C.c_double, C.c_double, vp, vp]),
    'dh_refine_frames_shape': (C.c_int, [C.c_int, C.c_int, i64] + [C.c_int] * 6 + [i64, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    'dh_refine_frames_host': (C.c_int, [vp, vp, vp, vp] + [C.c_int] * 5 + [C.c_double, C.c_double, vp, vp, vp]),
    'dh_pose_boxes_f64': (C.c_int, [vp, i64, i64, i64, C.c_int, C.c_int, C.c_int, vp, i64, C.c_int, C.c_double, vp, vp, vp, vp]),
    'dh_pose_boxes_host': (C.c_int, [vp, i64, i64, i64, C.c_int, C.c_int, C.c_int, vp, i64, C.c_int, C.c_double, vp, vp, vp]),
    'dh_frame_boxes_shape': (C.c_int, [C.c_int, C.c_int, i64] + [C.c_int] * 6 + [i64, C.c_int, C.POINTER(C.c_int)]),
    'dh_frame_boxes_host': (C.c_int, [vp, vp, vp, vp] + [C.c_int] * 4 + [C.c_double, vp, vp, vp]),
    'dh_vote_products_f64': (C.c_int, [C.POINTER(VoteSrc), C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    'dh_vote_products_host': (C.c_int, [C.POINTER(VoteSrc), C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp]),
    'dh_sched_build_ops':(C.c_int, [C.c_int] + [C.POINTER(i32)] * 5 + [C.c_int] * 4 + [C.POINTER(SchedOp), C.c_int,
                                     C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'dh_unpack_cut_f32': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, i64, C.c_int, vp, C.c_int, vp]),
    'dh_unpack_cut_host': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, i64, C.c_int, vp, C.c_int]),
    'dh_unpack_cut_vec4': (C.c_int, [C.c_int] * 4 + [vp, vp]),
    'dh_clip_inspect': (C.c_int, [vp, C.c_size_t, C.POINTER(ClipInfo)]),
    'dh_clip_inspect_cut': (C.c_int, [vp, C.c_size_t, C.c_int, C.POINTER(i32), C.POINTER(i32)]),
    'dh_clip_inspect_output': (C.c_int, [vp, C.c_size_t, C.c_int, C.POINTER(i32), C.POINTER(i32)]),
    'dh_clip_create': (C.c_int, [vp, C.c_size_t, C.c_int, ALLGATHER_FN, vp, C.POINTER(vp)]),
    'dh_clip_forward': (C.c_int, [vp, vp, C.c_int, C.POINTER(vp), vp]),
    'dh_clip_forward_host': (C.c_int, [vp, vp, C.c_int, C.POINTER(vp)]),
    'dh_clip_destroy': (C.c_int, [vp]),
    'dh_clip_world': (C.c_int, [vp]),
    'dh_clip_batch': (C.c_int, [vp]),
    'dh_clip_num_outputs': (C.c_int, [vp]),
    'dh_clip_output_items': (C.c_int64, [vp, C.c_int]),
    'dh_clip_frame_items': (C.c_int64, [vp]),
    'dh_clip_input_is_u8': (C.c_int, [vp]),
    'dh_graph_begin_capture': (C.c_int, [vp]),
    'dh_graph_end_capture': (C.c_int, [vp, C.POINTER(vp)]),
    'dh_graph_launch': (C.c_int, [vp, vp]),
    'dh_graph_destroy': (C.c_int, [vp]),
    'dh_event_create': (C.c_int, [C.POINTER(vp)]),
    'dh_event_record': (C.c_int, [vp, vp]),
    'dh_event_synchronize': (C.c_int, [vp]),
    'dh_event_elapsed_ms': (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
    'dh_event_destroy': (C.c_int, [vp]),
    'dh_stream_synchronize': (C.c_int, [vp]),
    'dh_stream_create': (C.c_int, [C.POINTER(vp)]),
    'dh_stream_destroy': (C.c_int, [vp]),
    'dh_event_create_sync': (C.c_int, [C.POINTER(vp)]),
    'dh_stream_wait_event': (C.c_int, [vp, vp]),
    'dh_stream_spin_us': (C.c_int, [vp, C.c_int]),
}

_lib = None


class DeepharHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, a different SONAME from the system
    # libamdhip64.so.7 this library links against).  Streams and device pointers only mean something inside
    # ONE runtime, so torch must be in the process (its runtime in the global symbol scope) before this
    # library is loaded; loaded the other way round the two runtimes coexist and every launch on a torch
    # stream fails.  A host without torch simply gets the system runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get('DEEPHAR_HIP_LIB', LIB_PATH)     # override: A/B runs of two builds of the library
    if not os.path.exists(path):
        raise DeepharHipError(
            'libdeephar_hip.so not found at %s -- the HIP back-end is mandatory (no CPU fallback). '
            'Build it with `python -m deephar_amd.csrc.build`.' % path)
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().dh_error_string(rc).decode()
        raise DeepharHipError('%s failed: %s (rc=%d)' % (what or 'deephar_hip call', msg, rc))
