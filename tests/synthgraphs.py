"""Synthetic graphs out of the public `layers` vocabulary, one per planner guard and each with its near-miss twin, plus a
seeded generator of random feature-map DAGs.  TEST INFRASTRUCTURE (tests/test_graphref_host.py, tests/test_gpu_synth_graphs.py;
tests/test_synth_split_host.py and tests/test_gpu_synth_graphs_split.py for the split-bf16 ladder).

Every graph is a function (H, W, C) -> (inputs, outputs).  `ZOO` lists them with the shapes they are built at, the plan
feature they exist for (`FEATURES`) and whether the default plan must show it there: a graph in which the guard holds says
True, its twin -- one clause of the guard broken -- says False.  Shapes: 16 x 16 maps (256 pixels: the split-K "skinny"
kernel once K >= 64) and 32 x 32 maps (the general / LDS-DMA / halo families), each with an aligned channel count (48) and an
odd one (34: scalar paths, channel offsets that are no multiples of four); graphs tied to one geometry say so.

The split-bf16 ladder (Model.gemm_precision) is tested on the same graphs at `SPLIT_SHAPES` (`split_graphs`): 32 x 32 x 48
(pointwise layers of the standard class, 3 x 3 layers with Cin % 32 == 16 of the extended class), 32 x 32 x 64 (K x K layers of
the standard class) and 16 x 16 x 48 (K = 48 < 64: pointwise layers stay off the skinny kernel), and at 32 x 32 x 34, where
next to nothing is eligible.
"""
import dataclasses

import numpy as np

from deephar_amd import Model, graph, layers as L, weights
from deephar_amd.engine.rules import RuleSet

SIZES = ((16, 16), (32, 32))
CHANNELS = (48, 34)
STD = tuple((h, w, c) for (h, w) in SIZES for c in CHANNELS)
SPLIT_SHAPES = ((32, 32, 48), (32, 32, 64), (16, 16, 48))      # the shapes of the split-bf16 leg
UNALIGNED_SHAPE = (32, 32, 34)                                  # ... and the one where the views are unaligned

BOOL_RULES = tuple(f.name for f in dataclasses.fields(RuleSet) if f.type is bool)


def all_off():
    return RuleSet(**{k: False for k in BOOL_RULES})


def one_off(name):
    return RuleSet(**{name: False})


# ---- R1 / R2: prologue and epilogue taps ---------------------------------------------------------------------------
def epi_chain(H, W, C):
    x = L.Input((H, W, C))
    return [x], [L.add([L.conv_bn_act(x, C, (3, 3), name='c'), x])]


def epi_bn_tapped(H, W, C):
    """... the BatchNormalization output is a model output too: the ReLU must not move into the convolution"""
    x = L.Input((H, W, C))
    b = L.conv_bn(x, C, (3, 3), name='c')
    return [x], [L.add([L.relu(b), x]), b]


def epi_all_tapped(H, W, C):
    """conv -> BN -> ReLU, all three tensors are outputs: nothing may be absorbed"""
    x = L.Input((H, W, C))
    c = L.conv(x, C, (3, 3), name='c')
    b = L.BatchNormalization(c, name='b')
    return [x], [c, b, L.relu(b)]


def pro_shared(H, W, C):
    """one BN -> ReLU chain read by two convolutions: both apply it on load, it is never written"""
    x = L.Input((H, W, C))
    t = L.relu(L.BatchNormalization(x, name='b'))
    return [x], [L.conv(t, C, (3, 3), name='c3'), L.conv(t, 17, (1, 1), name='c1')]


def pro_shared_tapped(H, W, C):
    """... and the activated tensor is an output as well: it has to be written"""
    x = L.Input((H, W, C))
    t = L.relu(L.BatchNormalization(x, name='b'))
    return [x], [L.conv(t, C, (3, 3), name='c3'), L.conv(t, 17, (1, 1), name='c1'), t]


# ---- R3: up-sampled second residual ----------------------------------------------------------------------------------
def _low(x, C):
    return L.conv(L.MaxPooling2D(x, (2, 2)), C, (1, 1), name='lo')


def up_res(H, W, C):
    x = L.Input((H, W, C))
    return [x], [L.add([L.conv_bn(x, C, (3, 3), name='a'), L.UpSampling2D(_low(x, C))])]


def up_res_lo3(H, W, C):
    """... with a 3x3 low-resolution convolution: K = 9 C >= 64 puts it on the skinny kernel, whose up-sampling epilogue has a
    scalar form (34 channels)"""
    x = L.Input((H, W, C))
    lo = L.conv(L.MaxPooling2D(x, (2, 2)), C, (3, 3), name='lo')
    return [x], [L.add([L.conv_bn(x, C, (3, 3), name='a'), L.UpSampling2D(lo)])]


def up_res_shared(H, W, C):
    """... the up-sampled tensor is read by a second convolution: it must exist at full resolution"""
    x = L.Input((H, W, C))
    u = L.UpSampling2D(_low(x, C))
    return [x], [L.add([L.conv_bn(x, C, (3, 3), name='a'), u]), L.conv(u, 17, (3, 3), name='c2')]


def up_res_output(H, W, C):
    x = L.Input((H, W, C))
    u = L.UpSampling2D(_low(x, C))
    return [x], [L.add([L.conv_bn(x, C, (3, 3), name='a'), u]), u]


def up_res_clip(H, W, C):
    """... under a leading clip dim"""
    x = L.Input((3, H, W, C))
    return [x], [L.add([L.conv_bn(x, C, (3, 3), name='a'), L.UpSampling2D(_low(x, C))])]


# ---- R4 / R4b: concatenation views ---------------------------------------------------------------------------------
def cat_direct(H, W, C):
    x = L.Input((H, W, C))
    a, b = L.conv(x, C, (3, 3), name='a'), L.conv_bn(x, 17, (1, 1), name='b')
    return [x], [L.conv(L.concatenate([a, b]), C, (1, 1), name='o')]


def cat_parts_shared(H, W, C):
    """... a part is read by a convolution of its own as well: it cannot live inside the concatenation (copy)"""
    x = L.Input((H, W, C))
    a, b = L.conv(x, C, (3, 3), name='a'), L.conv_bn(x, 17, (1, 1), name='b')
    return [x], [L.conv(L.concatenate([a, b]), C, (1, 1), name='o'), L.conv(b, C, (3, 3), name='o2')]


def cat_output_and_slice(H, W, C):
    x = L.Input((H, W, C))
    cat = L.concatenate([L.conv(x, C, (3, 3), name='a'), L.conv_bn(x, 17, (1, 1), name='b')])
    return [x], [cat, cat.channels(C - 5, C + 9)]


def cat_nested(H, W, C):
    x = L.Input((H, W, C))
    inner = L.concatenate([L.conv(x, 17, (1, 1), name='a'), L.conv(x, C, (3, 3), name='b')])
    return [x], [L.conv(L.concatenate([inner, L.conv_bn(x, 17, (1, 1), name='c')]), C, (1, 1), name='o')]


def cat_twice(H, W, C):
    """the same tensor listed twice in one concatenation: the second copy cannot be a view"""
    x = L.Input((H, W, C))
    a, b = L.conv(x, 17, (1, 1), name='a'), L.conv(x, C, (3, 3), name='b')
    return [x], [L.conv(L.concatenate([a, b, a]), C, (1, 1), name='o')]


def head17(H, W, C):
    """the 17-joint head: concatenate([f, h]) read by a 1x1 convolution of Cin = 34, h also read by the soft-argmax decoder"""
    x = L.Input((H, W, C))
    t = L.relu(L.BatchNormalization(x, name='b'))
    f, h = L.conv(t, 17, (1, 1), name='f'), L.conv(t, 17, (1, 1), name='h')
    p = L.act_channel_softmax(h)
    back = L.add([L.conv(L.concatenate([f, h]), C, (1, 1), name='o'), x])
    return [x], [back, L.softargmax2d(p), L.keypoint_confidence(p)]


def head17_conv_reader(H, W, C):
    """... h read by a convolution of its own: not a view reader, the concatenation is filled by a copy"""
    x = L.Input((H, W, C))
    t = L.relu(L.BatchNormalization(x, name='b'))
    f, h = L.conv(t, 17, (1, 1), name='f'), L.conv(t, 17, (1, 1), name='h')
    back = L.add([L.conv(L.concatenate([f, h]), C, (1, 1), name='o'), x])
    return [x], [back, L.conv(h, 17, (3, 3), name='o2')]


def pose_times_conf(H, W, C, tap=False):
    """multiply([coordinates, confidence]) right behind a read-out: folded into the soft-argmax launch"""
    x = L.Input((H, W, C))
    h = L.conv(L.relu(L.BatchNormalization(x, name='b')), 17, (1, 1), name='h')
    p = L.act_channel_softmax(h)
    xy = L.softargmax2d(p)
    outs = [L.add([L.conv(h, C, (3, 3), name='o'), x]), L.multiply([xy, L.keypoint_confidence(p)])]
    return [x], outs + ([xy] if tap else [])


def pose_times_conf_tapped(H, W, C):
    """... the coordinates are a model output as well: they have to be written"""
    return pose_times_conf(H, W, C, tap=True)


# ---- channel-slice readers (the input operand of a GEMM as a view) ----------------------------------------------------------
def _slice_reader(H, W, C, start):
    x = L.Input((H, W, C))
    wide = L.conv(x, C + 24, (1, 1), name='wide')
    return [x], [wide, L.conv(wide.channels(start, start + C), C, (1, 1), name='p'),
                 L.conv(wide.channels(start + 4, start + 4 + C), 40, (3, 3), name='k')]


def slice_reader(H, W, C):
    """a 1x1 and a 3x3 convolution each read C channels out of a tensor of C + 24 that is a model output as well, from channel
    4 and 8 on: x.coff % 4 == 0, x.ld > Cin -- 16-byte aligned views, which the LDS-DMA main loops of the split-bf16 kernels take"""
    return _slice_reader(H, W, C, 4)


def slice_reader_odd(H, W, C):
    """... from channel 2 and 6 on: the views are 8 bytes off, every GEMM family that loads 16 bytes at a time must refuse them"""
    return _slice_reader(H, W, C, 2)


# ---- R7: pooled second output ----------------------------------------------------------------------------------------
def conv_pool(H, W, C):
    """conv -> MaxPooling2D((2, 2)), the un-pooled tensor read as well"""
    x = L.Input((H, W, C))
    c = L.conv_bn(x, C, (1, 1), name='c')
    return [x], [L.conv(L.MaxPooling2D(c, (2, 2)), C, (1, 1), name='lo'), L.conv(c, 17, (1, 1), name='hi')]


# ---- R9 and the second-add rule ----------------------------------------------------------------------------------------
def add4(H, W, C):
    x = L.Input((H, W, C))
    return [x], [L.add([x, L.conv(x, C, (1, 1), name='a'), L.sepconv2d(x, C, (5, 5), name='s'), L.conv_bn(x, C, (3, 3), name='b')])]


def add4_shared(H, W, C):
    """... one producer has a second reader: it stays a tensor of its own, the sum is still spread over the other two"""
    x = L.Input((H, W, C))
    a = L.conv(x, C, (1, 1), name='a')
    s = L.add([x, a, L.sepconv2d(x, C, (5, 5), name='s'), L.conv(x, C, (3, 3), name='b')])
    return [x], [s, L.conv(a, 17, (3, 3), name='o2')]


def add_twice(H, W, C):
    """add([c, c]): the convolution's own output cannot be its residual"""
    x = L.Input((H, W, C))
    c = L.conv_bn(x, C, (3, 3), name='c')
    return [x], [L.add([c, c])]


def add3_inputs(H, W, C):
    x, z = L.Input((H, W, C), name='x'), L.Input((H, W, C), name='z')
    return [x, z], [L.add([x, z, L.conv(x, C, (3, 3), name='c')])]


def add_chain(H, W, C):
    """s1 = a + x (an output), s2 = s1 + b, s3 = s2 + x, relu(s3)"""
    x = L.Input((H, W, C))
    s1 = L.add([L.conv(x, C, (3, 3), name='a'), x])
    s2 = L.add([s1, L.conv_bn(x, C, (1, 1), name='b')])
    return [x], [s1, L.relu(L.add([s2, x]))]


# ---- R10 / R10b / R10c: sibling merges ---------------------------------------------------------------------------------
def siblings(H, W, C):
    """two 1x1 siblings of one relu(BN(x)) (Cin = 2 C, so that K >= 64 reaches the skinny kernel on the small maps), one
    followed by ReLU and one by BN, each read by a further convolution"""
    x = L.Input((H, W, 2 * C))
    t = L.relu(L.BatchNormalization(x, name='b'))
    p = L.relu(L.conv(t, C, (1, 1), name='p'))
    q = L.BatchNormalization(L.conv(t, 17, (1, 1), name='q'), name='qb')
    return [x], [L.conv(p, C, (3, 3), name='po'), L.conv(q, C, (3, 3), name='qo')]


def siblings_output(H, W, C):
    """... one sibling is a model output: it keeps its own buffer"""
    x = L.Input((H, W, 2 * C))
    t = L.relu(L.BatchNormalization(x, name='b'))
    p = L.relu(L.conv(t, C, (1, 1), name='p'))
    q = L.BatchNormalization(L.conv(t, 17, (1, 1), name='q'), name='qb')
    return [x], [L.conv(p, C, (3, 3), name='po'), L.conv(q, C, (3, 3), name='qo'), q]


def kxk_siblings(H, W, C):
    """the 3x1 | 3x3 | 3x5 siblings of a (T, J) plane into one concatenation"""
    x = L.Input((H, W, C))
    parts = [L.conv(x, 12, (3, 1), name='k31'), L.conv(x, 17, (3, 3), name='k33'), L.conv(x, 20, (3, 5), name='k35')]
    return [x], [L.concatenate(parts)]


# ---- R11 / R12: up-scaling unit, resampling on load ----------------------------------------------------------------------
def up_unit(H, W, C):
    x = L.Input((H // 2, W // 2, C))
    r = L.relu(L.BatchNormalization(L.UpSampling2D(x), name='b'))
    return [x], [L.add([L.conv(r, 40, (1, 1), name='sc'), L.sepconv2d(r, 40, (5, 5), name='s')])]


def up_unit_tapped(H, W, C):
    """... the activated tensor is a model output: the up-sampled tensor has to be written"""
    x = L.Input((H // 2, W // 2, C))
    r = L.relu(L.BatchNormalization(L.UpSampling2D(x), name='b'))
    return [x], [L.add([L.conv(r, 40, (1, 1), name='sc'), L.sepconv2d(r, 40, (5, 5), name='s')]), r]


def up_up(H, W, C):
    """UpSampling2D(UpSampling2D(x)) -> 1x1 convolution"""
    x = L.Input((H // 4, W // 4, C))
    return [x], [L.conv(L.UpSampling2D(L.UpSampling2D(x)), 17, (1, 1), name='c')]


def pool_one_reader(H, W, C):
    x = L.Input((H, W, C))
    return [x], [L.conv(L.MaxPooling2D(x, (2, 2)), C, (3, 3), name='c')]


def pool_two_readers(H, W, C):
    x = L.Input((H, W, C))
    p = L.MaxPooling2D(x, (2, 2))
    return [x], [L.conv(p, C, (3, 3), name='c'), L.conv(p, 17, (3, 3), name='c2')]


def maxmin_pool(H, W, C):
    """max_min_pooling (mode 1) whose only reader, through BN -> ReLU, is one convolution"""
    x = L.Input((H, W, C))
    return [x], [L.conv(L.relu(L.BatchNormalization(L.max_min_pooling(x, (2, 2)), name='b')), C, (3, 3), name='c')]


# ---- R13 / R14: merged pools, pooled segments (the action-head shape on a (T, J) plane) ----------------------------------
def _pools_cat(H, W, C, ca, cb, extra_reader=False):
    x, z = L.Input((H, W, C), name='x'), L.Input((H // 2, W // 2, 24), name='z')
    a, b = L.conv(x, ca, (3, 3), name='a'), L.conv_bn(x, cb, (3, 3), name='b')
    cat = L.concatenate([L.maxpooling2d(a, (2, 2), (2, 2)), L.maxpooling2d(b, (2, 2), (2, 2)), z])
    outs = [L.conv(cat, C, (1, 1), name='o')]
    if extra_reader:
        outs.append(L.conv(a, 17, (1, 1), name='o2'))
    return [x, z], outs


def pools_cat(H, W, C):
    return _pools_cat(H, W, C, C, 40 if C % 4 == 0 else 38)


def pools_cat_unpooled_read(H, W, C):
    return _pools_cat(H, W, C, C, 40 if C % 4 == 0 else 38, extra_reader=True)


def pools_cat_odd(H, W, C):
    """... the pooled channels are no multiple of four: one pooling launch still, but the convolution cannot pool on load"""
    return _pools_cat(H, W, C, 17, 17)


# ---- R15: learned resampling ---------------------------------------------------------------------------------------------
def learned_resample(H, W, C):
    x = L.Input((H, W, C))
    mid = (C + 16) // 4 * 4                   # (the transposed-convolution kernel takes multiples of four input channels)
    d = L.add([L.conv(x, mid, (1, 1), strides=(2, 2), name='sc'), L.sepconv2d(x, mid, (5, 5), strides=(2, 2), name='down')])
    u = L.conv2dtranspose(L.relu(L.BatchNormalization(d, name='b')), C, (2, 2), strides=(2, 2), name='up')
    return [x], [L.add([u, x])]


def learned_resample_bn_twice(H, W, C):
    """... the BatchNormalization output has a second reader"""
    x = L.Input((H, W, C))
    mid = (C + 16) // 4 * 4
    d = L.add([L.conv(x, mid, (1, 1), strides=(2, 2), name='sc'), L.sepconv2d(x, mid, (5, 5), strides=(2, 2), name='down')])
    n = L.BatchNormalization(d, name='b')
    u = L.conv2dtranspose(L.relu(n), C, (2, 2), strides=(2, 2), name='up')
    return [x], [L.add([u, x]), L.conv(n, 17, (1, 1), name='o2')]


# ---- element-wise tail ---------------------------------------------------------------------------------------------------
def eltwise_tail(H, W, C):
    x = L.Input((H, W, C))
    g = L.sigmoid(L.conv(x, C, (1, 1), name='g'))
    return [x], [L.scale(L.multiply([L.conv_bn(x, C, (3, 3), name='c'), g]), 0.5)]


# ---- plan features ---------------------------------------------------------------------------------------------------------
def _steps(plan, kind):
    return [s for s in plan.steps if s.kind == kind]


FEATURES = {
    'relu_in_epilogue': lambda p: any(s.attrs.get('post_relu') and 'post_bn' in s.params for s in _steps(p, 'conv')),
    'bn_in_epilogue': lambda p: any('post_bn' in s.params for s in _steps(p, 'conv')),
    'never_materialised': lambda p: not any(s.name == 'materialize' for s in p.steps),
    'res2_down': lambda p: any(s.attrs.get('res2_down') for s in _steps(p, 'conv')),
    'up2': lambda p: any(s.attrs.get('up2') for s in _steps(p, 'conv')),
    'no_upsample_launch': lambda p: not _steps(p, 'upsample_add'),
    'no_copy': lambda p: not _steps(p, 'copy'),
    'merged_conv': lambda p: any('+' in (s.name or '') for s in _steps(p, 'conv')),
    'ypool': lambda p: any('ypool' in s.outs for s in _steps(p, 'conv')),
    'no_eltwise_add': lambda p: not any(s.attrs.get('op') == 0 and 'b' in s.ins for s in _steps(p, 'eltwise')),
    'conv_before_upsampling': lambda p: any(s.outs['y'].shape[-2] * 2 == p.outputs[0].shape[-2] for s in _steps(p, 'conv')),
    'x_resample': lambda p: any(s.attrs.get('x_resample') for s in _steps(p, 'conv')),
    # (one pooling launch out of a joint buffer -- or, where R14 then takes it on load, a convolution pooling that joint buffer)
    'merged_pool': lambda p: any('+' in (s.name or '') for s in _steps(p, 'pool')) or any(
        s.attrs.get('seg') and sum(1 for q in p.steps for v in q.outs.values() if v is not None and v.buf is s.ins['x'].buf) == 2
        for s in _steps(p, 'conv')),
    'seg': lambda p: any(s.attrs.get('seg') for s in _steps(p, 'conv')),
    'convt_with_residual': lambda p: any('res1' in s.ins and 'pre_bn' in s.params for s in _steps(p, 'convtranspose')) and
    any(s.attrs.get('sh') == 2 for s in _steps(p, 'dwconv')),
    'xy_times_conf': lambda p: any(s.attrs.get('xy_times_conf') for s in _steps(p, 'sam')),
    'two_bn_prologues': lambda p: sum(1 for s in p.steps if 'pre_bn' in s.params) == 2 and not any(s.name == 'materialize' for s in p.steps),
    'three_eltwise': lambda p: len(_steps(p, 'eltwise')) == 3,
    # a convolution reads its input through a channel-slab view
    'x_view': lambda p: any(s.ins['x'].coff != 0 or s.ins['x'].ld != s.ins['x'].C for s in _steps(p, 'conv')),
}


@dataclasses.dataclass(frozen=True)
class Case:
    fn: object
    feature: str
    expect: object                    # bool, or (H, W, C) -> bool where the guard depends on the shape
    shapes: tuple = STD

    @property
    def name(self):
        return self.fn.__name__

    def expected(self, H, W, C):
        return self.expect(H, W, C) if callable(self.expect) else self.expect


_large = lambda H, W, C: H * W > 256          # the general kernels: a half-resolution residual / a pooled second output
_small = lambda H, W, C: H * W <= 256         # the skinny kernel (K >= 64 in every graph that says so)
PLANE = ((4, 16, 40), (4, 16, 48))            # the action heads' (T, J) plane
POOLED = tuple((32, w, c) for w in (32, 16, 8, 12) for c in CHANNELS)

ZOO = (
    Case(epi_chain, 'relu_in_epilogue', True),
    Case(epi_bn_tapped, 'relu_in_epilogue', False),
    Case(epi_all_tapped, 'bn_in_epilogue', False),
    Case(pro_shared, 'never_materialised', True),
    Case(pro_shared_tapped, 'never_materialised', False),
    # R3: the general kernels read the low-resolution tensor as a second residual; the skinny kernel (16 x 16) cannot, the
    # low-resolution convolution writes at 2x resolution instead (up2)
    Case(up_res, 'res2_down', _large),
    Case(up_res, 'up2', lambda H, W, C: H * W <= 256 and C % 4 == 0),     # (C = 34: a stand-alone upsample_add launch)
    Case(up_res_lo3, 'up2', _small),
    Case(up_res_lo3, 'res2_down', _large),
    Case(up_res_shared, 'res2_down', False),
    Case(up_res_shared, 'up2', False),
    Case(up_res_output, 'res2_down', False),
    Case(up_res_output, 'up2', False),
    Case(up_res_clip, 'up2', True, ((16, 16, 32),)),
    Case(up_res_clip, 'res2_down', True, ((32, 32, 32),)),
    Case(cat_direct, 'no_copy', True),
    Case(cat_parts_shared, 'no_copy', False),
    Case(cat_output_and_slice, 'no_copy', True),
    Case(cat_nested, 'no_copy', True),
    Case(cat_twice, 'no_copy', False),
    Case(head17, 'no_copy', True),
    Case(head17, 'merged_conv', True),
    Case(head17_conv_reader, 'no_copy', False),
    Case(pose_times_conf, 'xy_times_conf', True),
    Case(pose_times_conf_tapped, 'xy_times_conf', False),
    # R7: 32, 16 and 8 columns, channel counts that are multiples of four
    Case(conv_pool, 'ypool', lambda H, W, C: W in (32, 16, 8) and C % 4 == 0, POOLED),
    Case(add4, 'no_eltwise_add', True),
    Case(add4_shared, 'no_eltwise_add', True),
    Case(add_twice, 'no_eltwise_add', False),
    Case(add3_inputs, 'no_eltwise_add', True),
    Case(add_chain, 'no_eltwise_add', True),
    # R10c merges inside the skinny family only
    Case(siblings, 'merged_conv', _small),
    Case(siblings_output, 'merged_conv', False),
    # R10b: K x K siblings merge on the general kernel only -- Cin no multiple of 16 (the K x K MFMA families order K by chunks
    # of channels), not on the skinny kernel (its K runs follow from K: 4 x 16 x 40) -- and only where every part's taps keep
    # their places along the kernel's fmaf chain (planner.kxk_window_keeps_k_order: Cin = 40 does, Cin = 4 and 34 do not)
    Case(kxk_siblings, 'merged_conv', lambda H, W, C: (H, W, C) == (32, 32, 40),
         PLANE + ((4, 16, 4), (32, 32, 40), (32, 32, 34))),
    Case(up_unit, 'no_upsample_launch', True),
    Case(up_unit_tapped, 'no_upsample_launch', False),
    Case(up_up, 'conv_before_upsampling', True),
    # R12: readers on the skinny kernel only (the pooled map has a quarter of the pixels: 64 and 256)
    Case(pool_one_reader, 'x_resample', True),
    Case(pool_two_readers, 'x_resample', False),
    Case(maxmin_pool, 'x_resample', lambda H, W, C: H * W <= 1024, STD + ((48, 48, 48),)),
    Case(pools_cat, 'merged_pool', True, PLANE + ((16, 16, 34),)),
    Case(pools_cat, 'seg', True, PLANE + ((16, 16, 34),)),
    Case(pools_cat_unpooled_read, 'merged_pool', False, PLANE + ((16, 16, 34),)),
    Case(pools_cat_unpooled_read, 'seg', False, PLANE + ((16, 16, 34),)),
    Case(pools_cat_odd, 'merged_pool', True, PLANE + ((16, 16, 34),)),
    Case(pools_cat_odd, 'seg', False, PLANE + ((16, 16, 34),)),
    Case(learned_resample, 'convt_with_residual', True),
    Case(learned_resample_bn_twice, 'convt_with_residual', True),
    # the twin's BatchNormalization is applied on load by both of its readers
    Case(learned_resample, 'two_bn_prologues', False),
    Case(learned_resample_bn_twice, 'two_bn_prologues', True),
    Case(eltwise_tail, 'three_eltwise', True),
    # (the twin's plan is the same: what differs is the library's answer about the misaligned views, tests/test_synth_split_host.py)
    Case(slice_reader, 'no_copy', True),
    Case(slice_reader, 'x_view', True),
    Case(slice_reader_odd, 'no_copy', True),
    Case(slice_reader_odd, 'x_view', True),
)


def graphs():
    """every (graph function, H, W, C) of the zoo, once"""
    seen, out = set(), []
    for c in ZOO:
        for s in c.shapes:
            if (c.name,) + s not in seen:
                seen.add((c.name,) + s)
                out.append((c.fn,) + s)
    return out


def split_graphs(shapes=SPLIT_SHAPES):
    """every (graph function, H, W, C) of the split-bf16 leg: each zoo graph at each of `shapes`.  Every zoo graph can be
    built at any even H, W >= 16 and any C (conv_pool and pools_cat* at their 32-column form: 32 x 32, C = 48 and 64; the
    action heads' (T, J) plane of pools_cat* and kxk_siblings stays with the fp32 leg)."""
    fns = []
    for c in ZOO:
        if c.fn not in fns:
            fns.append(c.fn)
    return [(fn,) + tuple(s) for fn in fns for s in shapes]


SPLIT_RANDOM_SHAPES = ((32, 32, 48), (32, 32, 64))


# ---- the generator -----------------------------------------------------------------------------------------------------------
# The committed seeds: eleven whose default plan differs from the all-off plan at one size or both (R7, R9, R11, R12 between
# them) and one (5) that no switchable rule touches -- most random DAGs trigger none.
SEEDS = (2, 5, 9, 12, 13, 21, 26, 31, 48, 63, 64, 75)
RANDOM_SHAPES = ((16, 16, 34), (32, 32, 48))


def random_graph(seed, H, W, C):
    """A DAG of 8 - 14 feature-map nodes drawn from {conv 1x1 / 3x3 / (3, 1), sepconv 5x5, bn, relu, add of 2 - 4 earlier
    tensors of equal shape, concat, channel slice, MaxPooling2D((2, 2)), UpSampling2D}; 1 - 3 outputs among the sinks plus
    one interior tensor.  Candidates are drawn from one seeded stream until one has 8 - 14 nodes behind its outputs."""
    rng = np.random.default_rng(1000 + seed)
    while True:
        graph.reset_naming()
        inputs, outputs = _random_candidate(rng, H, W, C)
        if 8 <= len(graph.topo_nodes(outputs)) <= 14:
            return inputs, outputs


_RANDOM_OPS = ('conv1', 'conv1', 'conv3', 'conv31', 'sep5', 'sep5', 'bn', 'relu', 'add', 'add', 'add', 'concat', 'slice', 'pool', 'pool',
               'up', 'up', 'up')


def _random_candidate(rng, H, W, C):
    x = L.Input((H, W, C))
    ts, used = [x], set()
    widths = (C, C, 17, C // 2 + 1)
    for _ in range(int(rng.integers(9, 15))):
        op = str(rng.choice(_RANDOM_OPS))
        # unread tensors are preferred, so that the graph funnels towards few sinks; else one of the recent ones
        free = [t for t in ts if t.uid not in used]
        pool_ = free if free and rng.random() < 0.7 else ts[-5:]
        src = pool_[int(rng.integers(len(pool_)))]
        h, w, c = src.shape
        y = None
        if op in ('conv1', 'conv3', 'conv31'):
            y = L.conv(src, int(rng.choice(widths)), {'conv1': (1, 1), 'conv3': (3, 3), 'conv31': (3, 1)}[op])
        elif op == 'sep5':
            y = L.sepconv2d(src, int(rng.choice(widths)), (5, 5))
        elif op == 'bn' and (src.node is None or src.node.op != 'bn'):
            y = L.BatchNormalization(src, scale=bool(rng.integers(2)))
        elif op == 'relu' and (src.node is None or src.node.op != 'relu'):
            y = L.relu(src)
        elif op == 'add':
            same = [t for t in ts if t.shape == src.shape and t is not src]
            if same:
                k = int(rng.integers(1, min(3, len(same)) + 1))
                terms = [src] + [same[i] for i in rng.choice(len(same), size=k, replace=False)]
                y = L.add([terms[i] for i in rng.permutation(len(terms))])
        elif op == 'concat':
            same = [t for t in ts if t.shape[:2] == src.shape[:2] and t is not src and t.shape[2] + c <= 3 * C]
            if same:
                y = L.concatenate([src, same[int(rng.integers(len(same)))]])
        elif op == 'slice' and c >= 8:
            a = int(rng.integers(0, c - 4))
            y = src.channels(a, int(rng.integers(a + 3, c + 1)))
        elif op == 'pool' and h % 2 == 0 and w % 2 == 0 and h >= 8:
            y = L.MaxPooling2D(src, (2, 2))
        elif op == 'up' and h < H:
            y = L.UpSampling2D(src)
        if y is None:
            continue
        used.update(t.uid for t in y.node.inputs)
        ts.append(y)
    sinks = [t for t in ts[1:] if t.uid not in used]
    if not sinks:
        return [x], []
    nout = int(rng.integers(1, 4))
    outs = [sinks[i] for i in sorted(rng.choice(len(sinks), size=min(nout, len(sinks), 2 if nout == 3 else nout), replace=False))]
    if nout > len(outs):
        reach = {t.uid for n in graph.topo_nodes(outs) for t in n.outputs}
        interior = [t for t in ts[1:] if t.uid in used and t.uid in reach]
        if interior:
            outs.append(interior[int(rng.integers(len(interior)))])
    return [x], outs


# ---- building ----------------------------------------------------------------------------------------------------------------
def build(fn, H, W, C, seed=None):
    """(model with synthetic weights, the frames to feed it): graph `fn` at (H, W, C), or random_graph(seed, H, W, C)"""
    graph.reset_naming()
    inputs, outputs = random_graph(seed, H, W, C) if fn is None else fn(H, W, C)
    m = Model(list(inputs), list(outputs), name=('random%d' % seed) if fn is None else fn.__name__)
    weights.init_synthetic(m, seed=0)
    return m


def frames(m, n, seed=0):
    rng = np.random.default_rng(100 + seed)
    return [rng.uniform(-1, 1, (n,) + t.shape).astype(np.float32) for t in m.inputs]


# the switches that act when a plan is BOUND (engine/executor.py: the halo-resident kernel, grouped and paired launches): the step
# list cannot show them
EXECUTOR_RULES = ('halo_conv', 'group_launches', 'pair_convs')
PLANNER_RULES = tuple(k for k in BOOL_RULES if k not in EXECUTOR_RULES)


def switches_that_change(m):
    """the planner switches whose one-switch-off plan has another step list than the default plan"""
    from deephar_amd.engine.planner import build_plan
    base = describe(build_plan(m.inputs, m.outputs, rules=RuleSet()))
    return [k for k in PLANNER_RULES if describe(build_plan(m.inputs, m.outputs, rules=one_off(k))) != base]


def executor_switches(plan):
    """the executor switches a bound plan could show: the halo-resident kernel takes K x K convolutions, a grouped launch is a
    1x1 convolution followed by a depthwise step on the same tensor, a paired launch two convolutions of the skinny kernel"""
    from deephar_amd.engine.planner import split_k_rule
    convs = [s for s in plan.steps if s.kind == 'conv']
    out = []
    if any(s.attrs['kh'] * s.attrs['kw'] > 1 for s in convs):
        out.append('halo_conv')
    if any(a.kind == 'conv' and b.kind == 'dwconv' and a.ins['x'].buf is b.ins['x'].buf
           for a, b in zip(plan.steps, plan.steps[1:])):
        out.append('group_launches')
    px = lambda s: int(np.prod(s.outs['y'].shape[-3:-1])) // (4 if s.attrs.get('up2') else 1)
    if sum(1 for s in convs if split_k_rule(px(s), s.attrs['K'], s.attrs['Cout'], s.attrs['Cin'], s.attrs['kh'], s.attrs['kw'])) >= 2:
        out.append('pair_convs')
    return out


def describe(plan):
    """one line per step: the step list as the coverage and rule-switch checks compare it"""
    out = []
    for s in plan.steps:
        flags = ','.join('%s=%s' % (k, v) for k, v in sorted(s.attrs.items())
                         if k in ('post_relu', 'pre_relu', 'up2', 'res2_down', 'x_resample', 'pool2', 'seg', 'up_in', 'sh', 'op',
                                  'Cout', 'kh', 'kw') and v)
        views = ' '.join('%s:%s@%d/%d' % (r, 'x'.join(map(str, v.shape)), v.coff, v.ld)
                         for r, v in list(s.ins.items()) + list(s.outs.items()) if v is not None)
        out.append('%s %s [%s] {%s} %s' % (s.kind, s.name, flags, ','.join(sorted(s.params)), views))
    return out
