"""Host side of the extended split-bf16 scope (Model.gemm_scope = 'extended', dh_conv_args.w_split = 5 / 6 / 7): the library's
rule dh_conv2d_split_wide_eligible beside dh_conv2d_split_eligible, and the engine option.  No launch is made."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAX_PRE_KP = 4096      # csrc/conv_common.h: kMaxPreKp


def conv_args(hip_lib, n=2, h=32, w=32, cin=576, cout=576, kh=1, kw=None, stride=1, ldx=None, xptr=256, bn=False):
    from deephar_amd import _lib
    kw = kh if kw is None else kw
    a = _lib.ConvArgs()
    a.x, a.y = xptr, 1 << 20
    oh, ow = -(-h // stride), -(-w // stride)
    a.N, a.H, a.W, a.Cin, a.ldx, a.OH, a.OW, a.Cout, a.ldy = n, h, w, cin, ldx or cin, oh, ow, cout, cout
    a.KH, a.KW, a.SH, a.SW = kh, kw, stride, stride
    a.PT, a.PL = max((oh - 1) * stride + kh - h, 0) // 2, max((ow - 1) * stride + kw - w, 0) // 2      # TF-SAME
    a.K = kh * kw * cin
    kp, np_ = C.c_int(), C.c_int()
    assert hip_lib.dh_conv2d_packed_dims(kh, kw, cin, cout, C.byref(kp), C.byref(np_)) == 0
    a.Kp, a.Np = kp.value, np_.value
    if bn:
        a.pre_scale = a.pre_shift = 4096
        a.pre_relu = 1
    return a


def table(hip_lib):
    """(name, struct, standard, wide): the truth table of the two rules."""
    rows = [
        ('pointwise 576 -> 576', conv_args(hip_lib), 1, 1),
        ('3x3 Cin 64', conv_args(hip_lib, h=64, w=64, cin=64, cout=96, kh=3), 1, 1),
        ('3x3 Cin 48', conv_args(hip_lib, cin=48, cout=96, kh=3), 0, 1),
        ('3x3 Cin 144 stride 2', conv_args(hip_lib, h=128, w=128, cin=144, cout=96, kh=3, stride=2), 0, 1),
        ('1x5 Cin 80', conv_args(hip_lib, cin=80, cout=33, kh=1, kw=5), 0, 1),
        ('3x3 Cin 24', conv_args(hip_lib, cin=24, cout=96, kh=3), 0, 0),
        ('1x1 with BN prologue', conv_args(hip_lib, bn=True), 0, 1),
        ('1x1 with BN prologue, Cin 36', conv_args(hip_lib, cin=36, cout=24, bn=True), 0, 1),
        ('1x1 with BN prologue, Kp = kMaxPreKp', conv_args(hip_lib, cin=K_MAX_PRE_KP, cout=32, bn=True), 0, 1),
        ('1x1 with BN prologue, Kp = kMaxPreKp + 32', conv_args(hip_lib, cin=K_MAX_PRE_KP + 32, cout=32, bn=True), 0, 0),
        ('3x3 with BN prologue', conv_args(hip_lib, cin=64, cout=96, kh=3, bn=True), 0, 0),
        ('3x3 Cin 48 with BN prologue', conv_args(hip_lib, cin=48, cout=96, kh=3, bn=True), 0, 0),
        ('8x8x288 -> 128 skinny', conv_args(hip_lib, h=8, w=8, cin=288, cout=128), 0, 0),
        ('8x8x288 -> 128 skinny with BN prologue', conv_args(hip_lib, h=8, w=8, cin=288, cout=128, bn=True), 0, 0),
        ('3x3 Cin 48 skinny', conv_args(hip_lib, h=16, w=16, cin=48, cout=96, kh=3), 0, 0),
        ('Cin = 3', conv_args(hip_lib, h=256, w=256, cin=3, cout=32, kh=3, stride=2), 0, 0),
        ('ldx % 4 != 0', conv_args(hip_lib, ldx=578), 0, 0),
        ('BN prologue, ldx % 4 != 0', conv_args(hip_lib, ldx=578, bn=True), 0, 0),
        ('BN prologue, x not 16-byte aligned', conv_args(hip_lib, xptr=260, bn=True), 0, 0),
        ('3x3 Cin 48, x not 16-byte aligned', conv_args(hip_lib, cin=48, cout=96, kh=3, xptr=260), 0, 0),
    ]
    a = conv_args(hip_lib, bn=True)
    a.pre_shift = None
    rows.append(('scale without shift', a, 0, 0))
    a = conv_args(hip_lib)
    a.x_u8 = 1
    rows.append(('x_u8', a, 0, 0))
    a = conv_args(hip_lib, cin=48, cout=96, kh=3)
    a.x_u8 = 1
    rows.append(('x_u8, 3x3 Cin 48', a, 0, 0))
    a = conv_args(hip_lib, bn=True)
    a.up2 = 1
    rows.append(('BN prologue with fused up-sampling', a, 0, 0))
    return rows


def test_symbol_is_exported_and_declared(hip_lib):
    assert hasattr(hip_lib, 'dh_conv2d_split_wide_eligible')
    header = open(os.path.join(ROOT, 'include', 'deephar_hip.h')).read()
    assert re.search(r'\*/\s*int dh_conv2d_split_wide_eligible\(const dh_conv_args\* a\);', header)      # with its comment
    assert hip_lib.dh_conv2d_split_wide_eligible(None) == 0 and hip_lib.dh_conv2d_split_eligible(None) == 0


def test_truth_table_of_the_two_rules(hip_lib):
    for name, a, std, wide in table(hip_lib):
        assert hip_lib.dh_conv2d_split_eligible(C.byref(a)) == std, name
        assert hip_lib.dh_conv2d_split_wide_eligible(C.byref(a)) == wide, name
        assert wide >= std, name                 # the wide rule accepts everything the standard rule accepts


def test_answer_is_independent_of_w_split_of_n_and_of_the_weight_pointer(hip_lib):
    for name, a, _std, wide in table(hip_lib):
        for code in (0, 1, 2, 3, 4, 5, 6, 7):
            for n in (1, 2, 7, 64):
                for w in (0, 4, 1 << 16):
                    a.w_split, a.N, a.w = code, n, w
                    assert hip_lib.dh_conv2d_split_wide_eligible(C.byref(a)) == wide, (name, code, n, w)


def test_code_tables():
    from deephar_amd.engine import executor, packing
    assert executor.SPLIT_CODES == {'bf16x3': 1, 'bf16x2': 3, 'bf16': 4} and packing.SPLIT_PARTS == {1: 3, 3: 2, 4: 1}
    assert executor.WIDE_SPLIT_CODES == {'bf16x3': 5, 'bf16x2': 6, 'bf16': 7}
    assert packing.WIDE_SPLIT_PARTS == {5: 3, 6: 2, 7: 1}
    for mode, code in executor.WIDE_SPLIT_CODES.items():      # the packing of the standard code, byte for byte
        assert packing.WIDE_SPLIT_BASE[code] == executor.SPLIT_CODES[mode]
        assert packing.WIDE_SPLIT_PARTS[code] == packing.SPLIT_PARTS[executor.SPLIT_CODES[mode]]


def _mpii(blocks=1):
    from deephar_amd import graph
    from deephar_amd.models import reception
    graph.reset_naming()
    return reception.build((256, 256, 3), 16, dim=2, num_blocks=blocks, ksize=(5, 5), num_context_per_joint=2)


def test_option_default_validation_and_replan():
    m = _mpii()
    assert m.gemm_scope == 'standard'
    with pytest.raises(ValueError):
        m.gemm_scope = 'extented'                         # a typo raises at assignment
    assert m.gemm_scope == 'standard'
    m.gemm_precision = 'bf16'
    p1 = m.plan
    assert p1.gemm_scope == 'standard'
    m.gemm_scope = 'standard'
    assert m.plan is p1                                   # unchanged value: nothing is thrown away
    m.gemm_scope = 'extended'
    assert m._plan is None and m._exec is None
    p2 = m.plan
    assert p2 is not p1 and p2.gemm_scope == 'extended' and p2.gemm_precision == 'bf16'


def test_environment_default(monkeypatch):
    monkeypatch.setenv('DEEPHAR_GEMM_SCOPE', 'extended')
    assert _mpii().gemm_scope == 'extended'
    monkeypatch.setenv('DEEPHAR_GEMM_SCOPE', 'wide')
    with pytest.raises(ValueError):
        _mpii()
    monkeypatch.delenv('DEEPHAR_GEMM_SCOPE')
    assert _mpii().gemm_scope == 'standard'


def test_build_plan_validates_and_records():
    import inspect
    from deephar_amd.engine import planner, rules
    m = _mpii()
    params = list(inspect.signature(planner.build_plan).parameters)
    assert params[-1] == 'gemm_scope' and params[:6] == ['inputs', 'outputs', 'nstreams', 'gemm_precision', 'stream_policy', 'rules']
    assert planner.build_plan(m.inputs, m.outputs).gemm_scope == 'standard'
    assert planner.build_plan(m.inputs, m.outputs, gemm_precision='bf16x2', gemm_scope='extended').gemm_scope == 'extended'
    with pytest.raises(ValueError):
        planner.build_plan(m.inputs, m.outputs, gemm_scope='wide')
    import dataclasses
    names = [f.name for f in dataclasses.fields(rules.RuleSet)]
    assert len(names) == 18 and 'gemm_scope' not in names       # an engine option like gemm_precision, not a rule switch


def test_mpii_plans_are_identical_under_both_scopes():
    """The scope is an executor matter: the planner's steps do not depend on it."""
    def steps(scope):
        m = _mpii()
        m.gemm_precision, m.gemm_scope = 'bf16', scope
        return [(s.kind, sorted(s.ins), sorted(s.outs), sorted(s.params), sorted((k, repr(v)) for k, v in s.attrs.items() if not k.startswith('_')))
                for s in m.plan.steps]
    a, b = steps('standard'), steps('extended')
    assert len(a) == len(b) > 30
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, i
