"""downsampling_type='conv' (learned resampling: stride-2 residual units down, BN -> ReLU -> Conv2DTranspose up; reference
deephar/models/common.py:70-108, spnet.py:317-352) -- host side: builders, plan contents, weight files, struct layout.
No GPU needed."""
import collections
import ctypes
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

from deephar_amd import graph, utils, weights
from deephar_amd.config import ModelConfig
from deephar_amd.engine.planner import build_plan
from deephar_amd.engine.rules import RuleSet
from deephar_amd.models import spnet

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_OFF = RuleSet(**{f.name: False for f in dataclasses.fields(RuleSet) if f.type is bool})


def _build(ds, layout='pa16j2d', shape=(128, 128, 3), num_actions=(), action_pyramids=(), pyramids=2):
    graph.reset_naming()
    cfg = ModelConfig(shape, getattr(utils, layout), num_actions=list(num_actions), num_pyramids=pyramids,
                      action_pyramids=list(action_pyramids), downsampling_type=ds)
    return spnet.build(cfg)


def _layers_of(m, prefix):
    """(layer name, class, [(weight name, shape)]) of the layers whose name starts with `prefix`, in creation order."""
    seen = {}
    for n in m._nodes:
        for layer in n.layers.values():
            if layer.name.startswith(prefix):
                seen[layer.uid] = layer
    return [(l.name, l.cls, [(p.name, p.shape) for p in l.params]) for _, l in sorted(seen.items())]


@pytest.mark.parametrize('layout,shape,num_actions,action_pyramids', [
    ('pa16j2d', (128, 128, 3), (), ()),
    ('pa17j3d', (128, 128, 3), (), ()),
    ('pa17j3d', (4, 128, 128, 3), (10,), (1, 2)),
])
def test_conv_flavour_builds_with_the_shapes_of_the_pooling_flavour(layout, shape, num_actions, action_pyramids):
    conv = _build('conv', layout, shape, num_actions, action_pyramids)
    pool = _build('maxpooling', layout, shape, num_actions, action_pyramids)
    assert [o.shape for o in conv.outputs] == [o.shape for o in pool.outputs]
    ops = collections.Counter(n.op for n in conv._nodes)
    # no nearest up-sampling on the pose stream: what is left are the action heads' own (spnet.py:89-91), as in the other flavour
    assert ops['upsample'] == sum(1 for n in pool._nodes if n.op == 'upsample') - 3
    assert ops['upsample'] == 0 or action_pyramids
    assert ops['convtranspose'] == 3
    # one 3x3 / stride-2 pooling in the entry flow (spnet.py:325) and the action heads' poolings: none of them 2x2 'same' on
    # the pose stream's pyramids
    assert not any(n.op == 'pool' and n.name and '_du' in n.name for n in conv._nodes)


def test_layer_names_shapes_and_order_of_one_down_and_one_up_unit():
    """Written out from common.py:25-67 (residual_unit with strides=(2, 2): BatchNormalization '_bn1', the 1x1 stride-2
    '_shortcut_conv', the SeparableConv2D '_conv1') and common.py:103-106 ('_bn1', '_convtrans1')."""
    m = _build('conv')
    cin, out = 288, 384                        # first down unit of the first pyramid at growth 96
    bn = lambda c: [('gamma', (c,)), ('beta', (c,)), ('moving_mean', (c,)), ('moving_variance', (c,))]
    assert _layers_of(m, 'dp1_du1_') == [
        ('dp1_du1_r0_bn1', 'BatchNormalization', bn(cin)),
        ('dp1_du1_r0_shortcut_conv', 'Conv2D', [('kernel', (1, 1, cin, out))]),
        ('dp1_du1_r0_conv1', 'SeparableConv2D', [('depthwise_kernel', (5, 5, cin, 1)), ('pointwise_kernel', (1, 1, cin, out))]),
    ]
    cin, out = 576, 480                        # first up unit of the second pyramid
    assert _layers_of(m, 'up2_uu2_') == [
        ('up2_uu2_bn1', 'BatchNormalization', bn(cin)),
        ('up2_uu2_convtrans1', 'Conv2DTranspose', [('kernel', (2, 2, out, cin))]),
    ]
    nodes = {n.name: n for n in m._nodes if n.name}
    assert nodes['dp1_du1_r0_conv1'].attrs['sh'] == 2 and nodes['dp1_du1_r0_conv1'].attrs['sw'] == 2
    assert nodes['dp1_du1_r0_conv1'].attrs['pt'] == 1 and nodes['dp1_du1_r0_conv1'].attrs['pl'] == 1      # SAME at stride 2: (1, 2)
    assert nodes['dp1_du1_r0_conv1'].outputs[0].shape == (8, 8, 384)
    assert nodes['up2_uu2_convtrans1'].outputs[0].shape == (4, 4, 480)


def test_auto_name_and_unsupported_geometries():
    from deephar_amd import layers as L
    graph.reset_naming()
    x = L.Input((4, 4, 8))
    y = L.conv2dtranspose(x, 6, (2, 2), strides=(2, 2))
    assert y.node.name == 'conv2d_transpose_1' and y.shape == (8, 8, 6)
    assert y.node.layers['convt'].params[0].shape == (2, 2, 6, 8)
    for size, strides in (((3, 3), (2, 2)), ((2, 2), (1, 1)), ((4, 4), (2, 2))):
        with pytest.raises(NotImplementedError, match=r'kernel_size=\(2, 2\), strides=\(2, 2\)'):
            L.conv2dtranspose(x, 6, size, strides=strides)
    z = L.sepconv2d(L.Input((7, 9, 8)), 12, (5, 5), strides=(2, 2))
    assert z.shape == (4, 5, 12) and (z.node.attrs['pt'], z.node.attrs['pl']) == (2, 2)      # odd extents: (2, 2)


def test_plan_has_strided_depthwise_and_transposed_conv_steps_and_folds_the_lateral_add():
    m = _build('conv')
    on = build_plan(m.inputs, m.outputs, rules=RuleSet())
    kinds = collections.Counter(s.kind for s in on.steps)
    assert kinds['upsample_add'] == 0
    assert [s.name for s in on.steps if s.kind == 'pool'] == ['pool'] or kinds['pool'] == 1      # the entry flow's 3x3 pooling only
    pool = next(s for s in on.steps if s.kind == 'pool')
    assert (pool.attrs['kh'], pool.attrs['sh']) == (3, 2)
    convt = [s for s in on.steps if s.kind == 'convtranspose']
    assert [s.name for s in convt] == ['up2_uu2_convtrans1', 'up2_uu1_convtrans1', 'up2_uu0_convtrans1']
    for s in convt:                            # BN + ReLU are the prologue, the lateral add is the residual
        assert 'pre_bn' in s.params and s.attrs['pre_relu'] == 1 and 'res1' in s.ins
        assert s.ins['res1'].shape == s.outs['y'].shape
        assert s.outs['y'].shape[-3:-1] == tuple(2 * d for d in s.ins['x'].shape[-3:-1])
    strided = [s for s in on.steps if s.kind == 'dwconv' and (s.attrs.get('sh', 1), s.attrs.get('sw', 1)) != (1, 1)]
    assert [s.name for s in strided] == ['dp1_du%d_r0_conv1/dw' % i for i in (1, 2, 3)]
    for s in strided:
        assert (s.attrs['sh'], s.attrs['sw'], s.attrs['pt'], s.attrs['pl'], s.attrs['up_in']) == (2, 2, 1, 1, 0)
        assert s.outs['y'].shape[-3:-1] == tuple(d // 2 for d in s.ins['x'].shape[-3:-1]) and 'pre_bn' in s.params
    # the stride-2 shortcut of each down unit stays a launch of its own with its stride (no joint buffer, no pooled output)
    short = [s for s in on.steps if s.kind == 'conv' and s.name and s.name.endswith('_r0_shortcut_conv')]
    assert len(short) == 3 and all((s.attrs['sh'], s.attrs['sw'], s.attrs['kh']) == (2, 2, 1) and 'ypool' not in s.outs for s in short)
    # with the add rule off the three lateral adds are element-wise launches again
    off = build_plan(m.inputs, m.outputs, rules=dataclasses.replace(RuleSet(), split_adds=False))
    convt_off = [s for s in off.steps if s.kind == 'convtranspose']
    assert len(convt_off) == 3 and not any('res1' in s.ins for s in convt_off)
    adds_on = sum(1 for s in on.steps if s.kind == 'eltwise')
    adds_off = sum(1 for s in off.steps if s.kind == 'eltwise')
    plain = build_plan(m.inputs, m.outputs, rules=ALL_OFF)
    assert sum(1 for s in plain.steps if s.kind == 'convtranspose' and 'res1' not in s.ins) == 3
    assert adds_on == 0 and adds_off >= 3
    # exactly three steps apart from what split_adds does to the rest of the network: the same switch on the pooling flavour
    # moves the same wide / second adds, minus the three lateral adds of the up path that flavour folds elsewhere
    assert len(off.steps) - len(on.steps) == adds_off - adds_on


def test_clip_model_with_actions_plans_under_every_policy():
    m = _build('conv', 'pa17j3d', (4, 128, 128, 3), (10,), (1, 2))
    for kw in (dict(), dict(nstreams=2, stream_policy='tail'), dict(rules=ALL_OFF)):
        p = build_plan(m.inputs, m.outputs, **kw)
        assert sum(1 for s in p.steps if s.kind == 'convtranspose') == 3
        assert sum(1 for s in p.steps if s.kind == 'dwconv' and s.attrs.get('sh', 1) == 2) == 3


def test_max_pooling_flavour_plan_is_unchanged():
    """Step for step what the commit before this feature planned for the 128 px pose-only SPNet (tests/golden/
    spnet128_maxpooling_plan.json: kind, name, operand roles, attributes and output shapes of its 76 steps)."""
    m = _build('maxpooling')
    p = build_plan(m.inputs, m.outputs, rules=RuleSet())
    clean = lambda v: v if isinstance(v, (int, float, str, bool)) or v is None else repr(v)
    got = [[s.kind, s.name, sorted(s.ins), sorted(k for k, v in s.outs.items() if v is not None),
            {k: clean(v) for k, v in sorted(s.attrs.items())},
            [list(s.outs[k].shape) for k in sorted(s.outs) if s.outs[k] is not None]] for s in p.steps]
    want = json.load(open(os.path.join(HERE, 'golden', 'spnet128_maxpooling_plan.json')))
    assert len(got) == len(want) == 76
    for g, w in zip(got, want):
        assert g == w
    # and the protocol model of the README's speed2d figures keeps the step count this planner gave it before the feature
    graph.reset_naming()
    cfg = ModelConfig((8, 256, 256, 3), utils.pa16j2d, num_actions=[15], num_pyramids=6, action_pyramids=[1, 2, 3, 4, 5, 6],
                      pose_replica=True, num_pose_features=160, num_visual_features=160)
    big = spnet.build(cfg)
    steps = build_plan(big.inputs, big.outputs, rules=RuleSet()).steps
    assert len(steps) == 448 and not any(s.kind == 'convtranspose' or 'sh' in s.attrs and s.kind == 'dwconv' for s in steps)


def test_init_synthetic_fills_every_parameter_and_keeps_activations_of_order_one():
    m = _build('conv')
    weights.init_synthetic(m, seed=0)
    assert all(p.value is not None and np.all(np.isfinite(p.value)) for p in m.params)
    k = next(p for p in m.params if p.key.endswith('up2_uu2_convtrans1/kernel'))
    assert k.role == 'convt' and k.fan_in == 576
    # He-normal over the ONE tap an output pixel sees: std = sqrt(2 / Cin), not sqrt(2 / (4 Cin))
    assert abs(float(k.value.std()) / np.sqrt(2.0 / 576) - 1) < 0.02


@pytest.mark.parametrize('by_name', [False, True])
def test_hdf5_round_trip(tmp_path, by_name):
    m = _build('conv')
    weights.init_synthetic(m, seed=3)
    path = str(tmp_path / 'conv_flavour.h5')
    weights.save_weights(m, path)
    want = {p.key: p.value.copy() for p in m.params}
    m2 = _build('conv')
    weights.load_weights(m2, path, by_name=by_name)
    got = weights.as_dict(m2)
    assert set(got) == set(want)
    for k in want:
        assert got[k] is not None and np.array_equal(got[k], want[k]), k
    from deephar_amd import keras_compat
    names = [name for name, _ in keras_compat.layout(m)]
    assert 'up2_uu0_convtrans1' in names and 'dp1_du3_r0_conv1' in names


def test_new_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of dh_dw_strided and dh_conv_transpose against the ctypes mirrors."""
    from deephar_amd import _lib
    root = os.path.dirname(HERE)
    pairs = {'dh_dw_strided': _lib.DwsArgs, 'dh_conv_transpose': _lib.ConvtArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "deephar_hip.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('return 0; }')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', exe], check=True)
    got = dict(l.split() for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, ct in pairs.items():
        assert int(got[cname]) == ctypes.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(ct, fname).offset, (cname, fname)
    assert ctypes.sizeof(_lib.DwsArgs) == 104 and ctypes.sizeof(_lib.ConvtArgs) == 96


def test_transposed_kernel_packing_routes_the_four_taps(hip_lib):
    """[2, 2, Cout, Cin] -> the [Cin, 4 Cout] B operand: column (2a + b) * Cout + co is W[a, b, co, :], also when Cout is not
    a multiple of the packer's 32-column padding (the padding follows the LAST block)."""
    from deephar_amd.engine import packing
    rng = np.random.default_rng(0)
    for cout, cin in ((20, 48), (16, 32), (24, 36), (288, 384)):
        w = rng.standard_normal((2, 2, cout, cin)).astype(np.float32)
        packed, kp, np_ = packing.pack_convt(w)
        assert kp == (cin + 31) // 32 * 32 and np_ == (4 * cout + 31) // 32 * 32
        b = packing.unpack_conv(packed, 1, 1, cin, 4 * cout)[0, 0]
        for a_ in range(2):
            for b_ in range(2):
                blk = b[:, (2 * a_ + b_) * cout:(2 * a_ + b_ + 1) * cout]
                assert np.array_equal(blk, w[a_, b_].T)


def test_serialised_function_table_keeps_version_2_ids():
    """New step records were appended: the ids a version-2 blob uses are unchanged."""
    from deephar_amd.engine import serialize
    assert serialize.FUNCTIONS[:19][-1] == 'dh_conv2d_seg_f32' and serialize.FUNCTIONS[0] == 'dh_conv2d_f32'
    assert serialize.FUNCTIONS[19:] == ['dh_dwconv2d_strided_f32', 'dh_conv2d_transpose2x2_f32']
    assert serialize.V3_FUNCTIONS == 19 and serialize.VERSION == 2
