"""Channel-slab views for the op-level tests.  TEST INFRASTRUCTURE (a plain module, imported like tests/wellcond.py).

The planner hands nearly every kernel a (pointer, pitch) view: a run of C channels at offset `off` inside pixels of `ld`
floats (concatenation slabs, pose-buffer columns, pooled / concatenated runs sharing a buffer).  `slab` builds such a view
on the device, `assert_untouched` checks bit for bit that a launch wrote nothing outside it:

  * inputs are built with fill = NaN, so a read outside the view that reaches a result poisons it;
  * outputs are built with a finite canary everywhere (inside the view too: an element the kernel forgets keeps it);
  * every slab sits between two guard runs of GUARD floats holding the same fill, so that an overrun in front of the
    first or behind the last pixel shows as well -- also for the dense layout, where the tensor itself has no spare channel.

Three layouts are used throughout (`layout`):
  dense    ld = C, off = 0
  aligned  ld a multiple of 4 above C, off a multiple of 4: the float4 path of a kernel, with a pitch
  odd      an odd off (and an odd ld unless the caller needs another): the scalar path
`k` = 0, 1, 2 .. gives the operands of one launch different pitches and offsets.

Also here, because the GPU test and the host test share it: the shapes that reach the four instantiations of the 2-D
soft-argmax kernel, and what the library says it will launch for a shape (`sam_variant`, `sam_ctx_rc`: dh_softargmax2d_route
on fake pointers -- nothing of the launchers is restated).
"""
import numpy as np

CANARY = 7.0
GUARD = 64            # floats in front of and behind every slab: 256 bytes, keeps the slab's 16-byte alignment
LAYOUTS = ('dense', 'aligned', 'odd')


def layout(C, name, k=0):
    """(ld, off) of layout `name` for a C-channel view; operand number k of a launch."""
    if name == 'dense':
        return C, 0
    if name == 'aligned':
        return (C + 3) // 4 * 4 + 4 * (2 + k), 4 * (1 + k)
    if name == 'odd':
        off = 1 + 2 * k
        return (C + off + 2 * k + 1) | 1, off
    raise ValueError(name)


def slab(values, ld, off, fill, device='cuda'):
    """Put a [..., C] array into channels [off, off + C) of a [..., ld] float32 device tensor whose other channels (and the
    guard runs around it) hold `fill`.  Returns (tensor, device pointer of the view = data_ptr() + 4 * off)."""
    import torch
    v = np.asarray(values, np.float32)
    C = v.shape[-1]
    assert 0 <= off and off + C <= ld, (C, ld, off)
    buf = np.full(v.shape[:-1] + (ld,), fill, np.float32)
    buf[..., off:off + C] = v
    flat = np.full(buf.size + 2 * GUARD, fill, np.float32)
    flat[GUARD:GUARD + buf.size] = buf.ravel()
    base = torch.from_numpy(flat).to(device)
    t = base[GUARD:GUARD + buf.size].view(buf.shape)
    assert t._base is base and t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off


def out_slab(shape, ld, off, canary=CANARY, device='cuda'):
    """An output view of `shape` = [..., C]: the whole slab, the view included, holds the canary."""
    return slab(np.full(shape, canary, np.float32), ld, off, canary, device)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def assert_untouched(tensor, off, C, canary=CANARY, what=''):
    """Everything outside channels [off, off + C) of a tensor made by `slab`, guard runs included, still holds `canary`
    bit for bit."""
    want = np.array(canary, np.float32).view(np.uint32)
    b = _bits(tensor)
    assert np.all(b[..., :off] == want) and np.all(b[..., off + C:] == want), \
        '%s: wrote outside channels [%d, %d) of its %d-float pixels' % (what, off, off + C, tensor.shape[-1])
    g = _bits(tensor._base)
    assert np.all(g[:GUARD] == want), '%s: wrote in front of its buffer' % what
    assert np.all(g[-GUARD:] == want), '%s: wrote behind its buffer' % what


def view(tensor, off, C):
    """The view's values as a NumPy array [..., C]."""
    return tensor[..., off:off + C].detach().cpu().contiguous().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the 2-D read-outs' launch decision, asked of the library (dh_softargmax2d_route) ------------------------------------------
def sam_slab_bytes(H, W, g):
    """LDS bytes of g channels of an H x W map and the two grids (include/deephar_hip.h: dh_sam_route.staged)."""
    return (H * W * g + W + H) * 4


def sam_route(lib, F, H, W, C, J=0, nctx=0, ldh=None, h=0x100000):
    """dh_softargmax2d_route for an [F, H, W, C] launch on fake, 16-byte aligned pointers; only conf_raw of the optional
    outputs is asked for, as the fused read-out requires."""
    from deephar_amd import _lib
    a = _lib.SamArgs()
    a.h, a.gx, a.gy, a.conf_raw = h, 0x200000, 0x300000, 0x400000
    a.F, a.H, a.W, a.C, a.ldh, a.ldxy, a.ldcr, a.ldcp, a.ldp = F, H, W, C, ldh or C, 2, 1, 1, C
    return _lib.sam_route(lib, a, J, nctx)


def sam_variant(lib, F, H, W, C):
    """(channels per work-group, staged in LDS) of softargmax2d_kernel<G, STAGED> for an [F, H, W, C] launch."""
    r = sam_route(lib, F, H, W, C)
    assert r.rc == 0, (F, H, W, C, r.rc)
    return r.channels, bool(r.staged)


def sam_ctx_rc(lib, H, W, J=8, nctx=2, F=2):
    """The code dh_softargmax2d_context_f32 answers for J joints with nctx context maps each on H x W maps (0: it launches)."""
    return sam_route(lib, F, H, W, J * (1 + nctx), J, nctx).ctx_rc


# (F, H, W, C) -> the instantiation the shape is there for
SAM_VARIANT_SHAPES = {
    (1024, 4, 4, 16): (16, True),
    (512, 8, 8, 17): (16, True),       # the second channel group holds one live channel
    (1024, 46, 46, 3): (16, False),    # slab of 135 792 B
    (2, 64, 64, 5): (4, False),        # slab of 66 048 B
    (3, 16, 16, 17): (4, True),        # the shape of the view cases
    (512, 6, 4, 17): (16, True),       # H != W, one orientation each (all four, both ways: tests/test_gpu_rect_ops.py)
    (2, 48, 96, 5): (4, False),        # slab of 74 304 B
}
