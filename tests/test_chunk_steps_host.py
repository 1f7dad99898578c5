"""The arithmetic the executor's chunk loops share (engine/executor.py: chunk_steps, ring_depth), without a GPU."""
import pytest

from deephar_amd.engine.executor import chunk_steps, ring_depth


@pytest.mark.parametrize('total,bs,depth,passes', [(6, 4, 2, 1), (5, 2, 2, 2), (1, 1, 2, 3), (17, 4, 8, 1), (8, 4, 2, 1)])
def test_chunk_steps_cover_every_pass_once_and_in_order(total, bs, depth, passes):
    steps = list(chunk_steps(total, bs, depth, passes))
    nchunks = -(-total // bs)
    assert [s[0] for s in steps] == list(range(passes * nchunks))               # consecutive across the passes
    for step, t, ci, slot, start, m in steps:
        assert (t, ci) == divmod(step, nchunks) and slot == step % depth and start == ci * bs
        assert 1 <= m <= bs
    for t in range(passes):
        mine = [s for s in steps if s[1] == t]
        rows = [r for _, _, _, _, start, m in mine for r in range(start, start + m)]
        assert rows == list(range(total))                                       # every row once, in order
        assert all(m == bs for _, _, _, _, _, m in mine[:-1])                    # only a pass's last chunk is short
        assert mine[-1][5] == total - (nchunks - 1) * bs


def test_ring_depth_at_its_edges(monkeypatch):
    monkeypatch.delenv('DEEPHAR_PREDICT_DEPTH', raising=False)
    assert ring_depth(1) == 2                                                   # one chunk: still two slots
    assert ring_depth(3) == 3 and ring_depth(8) == 8 and ring_depth(100) == 8   # one per step up to the default of 8
    assert ring_depth(100, 300 << 20) == 2                                      # 512 MB of staging hold one 300 MB slot: the floor
    assert ring_depth(100, 100 << 20) == 5 and ring_depth(100, 1) == 8
    monkeypatch.setenv('DEEPHAR_PREDICT_DEPTH', '1')
    assert ring_depth(100) == 2                                                 # the variable cannot go below the floor
    monkeypatch.setenv('DEEPHAR_PREDICT_DEPTH', '3')
    assert ring_depth(100) == 3 and ring_depth(2) == 2
