"""Host tests (no GPU) that go with tests/test_gpu_slab_ops.py: the shapes its soft-argmax cases use reach all four
instantiations of softargmax2d_kernel, by the launcher's own rule."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slabview as SV                              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_softargmax2d_shapes_reach_all_four_instantiations():
    """launch_softargmax2d picks <16, *> when F * ceil(C / 16) >= 1024 and the un-staged kernels when the LDS slab would
    exceed 128 KB (wide) or 60 KB (narrow).  slabview.sam_variant restates that rule; the statements it restates must still
    stand in the source as written, so that a change of a threshold fails here and the shapes are looked at again instead
    of quietly becoming several tests of one variant."""
    src = open(os.path.join(ROOT, 'deephar_amd', 'csrc', 'decoder.hip')).read()
    for line in SV.SAM_SOURCE_LINES:
        assert src.count(line) == 1, 'launch_softargmax2d no longer says `%s`: restate slabview.sam_variant' % line
    assert 'const size_t slab = ((size_t)a.H * a.W * g + a.W + a.H) * sizeof(float);' in src
    # the fused read-out (rule R5b) has no unstaged variant: the planner restates its refusal (tests/test_rect_host.py)
    from deephar_amd.engine import planner
    assert 'const size_t slab = ((size_t)a.H * a.W * CG + a.W + a.H) * sizeof(float);' in src and 'constexpr int CG = 16;' in src
    assert planner.SAM_CTX_MAX_SLAB == SV.SAM_CTX_SLAB
    assert all(planner.sam_ctx_slab_bytes(h, w) == SV.sam_slab_bytes(h, w, 16) for h, w in ((45, 45), (40, 52), (3, 300)))
    for shape, want in SV.SAM_VARIANT_SHAPES.items():
        assert SV.sam_variant(*shape) == want, (shape, SV.sam_variant(*shape), want)
    assert set(SV.SAM_VARIANT_SHAPES.values()) == {(16, True), (16, False), (4, True), (4, False)}
    # the slab sizes the shapes were chosen by, and the rule at its edges
    assert SV.sam_slab_bytes(46, 46, 16) == 135792 > SV.SAM_SLAB_WIDE
    assert SV.sam_slab_bytes(64, 64, 4) == 66048 > SV.SAM_SLAB_NARROW
    assert SV.sam_variant(1023, 4, 4, 16) == (4, True) and SV.sam_variant(1024, 4, 4, 16) == (16, True)
    assert SV.sam_variant(1, 32, 32, 272) == (4, True)      # the largest shape of test_gpu_ops.test_softargmax2d: 17 groups


def test_slab_layouts_are_what_they_claim():
    """dense / aligned / odd for every channel count and operand number the GPU tests use: the view fits its pixel, the
    aligned layout keeps 16-byte alignment with a pitch, the odd one breaks it."""
    # (second row: the channel counts of tests/convview.py, whose launches have up to five operands)
    for C in (1, 2, 3, 5, 16, 17, 20, 24, 60, 300, 576,
              18, 30, 32, 40, 48, 64, 66, 70, 72, 94, 96, 100, 200, 264):
        for k in range(5):
            assert SV.layout(C, 'dense', k) == (C, 0)
            ld, off = SV.layout(C, 'aligned', k)
            assert ld % 4 == 0 and off % 4 == 0 and off > 0 and off + C <= ld and ld > C
            ld, off = SV.layout(C, 'odd', k)
            assert ld % 2 == 1 and off % 2 == 1 and off + C <= ld
        assert len({SV.layout(C, 'aligned', k) for k in range(5)}) == 5
        assert len({SV.layout(C, 'odd', k) for k in range(5)}) == 5
