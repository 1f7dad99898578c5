"""Host tests (no GPU) that go with tests/test_gpu_slab_ops.py: the shapes its soft-argmax cases use reach all four
instantiations of softargmax2d_kernel, by the library's own answer (dh_softargmax2d_route)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slabview as SV                              # noqa: E402


def test_softargmax2d_shapes_reach_all_four_instantiations(hip_lib):
    """launch_softargmax2d picks <16, *> when F * ceil(C / 16) >= 1024 and the un-staged kernels when the LDS slab would
    exceed 128 KB (wide) or 60 KB (narrow).  The library says which (dh_softargmax2d_route, the function the launcher runs), so
    a change of a threshold fails here and the shapes are looked at again instead of quietly becoming several tests of one
    variant."""
    for shape, want in SV.SAM_VARIANT_SHAPES.items():
        assert SV.sam_variant(hip_lib, *shape) == want, (shape, SV.sam_variant(hip_lib, *shape), want)
    assert set(SV.SAM_VARIANT_SHAPES.values()) == {(16, True), (16, False), (4, True), (4, False)}
    # the slab sizes the shapes were chosen by, and the rule at its edges: 128 KiB with 16 channels, 60 KiB with 4
    assert SV.sam_slab_bytes(46, 46, 16) == 135792 > 128 * 1024 and SV.sam_variant(hip_lib, 1024, 46, 46, 3) == (16, False)
    assert SV.sam_slab_bytes(45, 45, 16) == 129960 <= 128 * 1024 and SV.sam_variant(hip_lib, 1024, 45, 45, 3) == (16, True)
    assert SV.sam_slab_bytes(64, 64, 4) == 66048 > 60 * 1024 and SV.sam_variant(hip_lib, 2, 64, 64, 5) == (4, False)
    assert SV.sam_slab_bytes(62, 62, 4) == 62000 > 60 * 1024 >= SV.sam_slab_bytes(61, 62, 4) == 61004
    assert SV.sam_variant(hip_lib, 2, 62, 62, 5) == (4, False) and SV.sam_variant(hip_lib, 2, 61, 62, 5) == (4, True)
    assert SV.sam_variant(hip_lib, 1023, 4, 4, 16) == (4, True) and SV.sam_variant(hip_lib, 1024, 4, 4, 16) == (16, True)
    assert SV.sam_variant(hip_lib, 1, 32, 32, 272) == (4, True)      # the largest shape of test_gpu_ops.test_softargmax2d: 17 groups
    # the fused read-out (rule R5b) has no unstaged variant: it refuses above 128 KiB of 16 channel lanes, and the planner
    # (pure Python: it plans without the library) keeps the same limit -- a sweep over map sizes on both sides of it
    from deephar_amd.engine import planner
    sides = set()
    for h in list(range(1, 64)) + [300]:
        for w in list(range(1, 64)) + [300]:
            fits = planner.sam_ctx_slab_bytes(h, w) <= planner.SAM_CTX_MAX_SLAB
            assert planner.sam_ctx_slab_bytes(h, w) == SV.sam_slab_bytes(h, w, 16)
            assert SV.sam_ctx_rc(hip_lib, h, w) == (0 if fits else -2), (h, w)
            sides.add(fits)
    assert sides == {True, False}
    # 45 x 45 and 40 x 48 fused; 44 x 48, 40 x 52 and 48 x 48 refused
    assert [SV.sam_ctx_rc(hip_lib, h, w) for h, w in ((45, 45), (40, 48), (44, 48), (40, 52), (48, 48))] == [0, 0, -2, -2, -2]


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
