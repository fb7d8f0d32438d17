"""The Philox draw kernels against a host model, element for element, and the small rollout / replay entry points that
only ran inside Trainer.process: unreal_gather_i32, unreal_ring_cur_idx with a base actor, unreal_rollout_stats (GPU).

tests/philox_model.py is pinned to the Random123 known-answer vectors by test_replay_edges_cpu.py; here every element
of a draw is compared with it exactly, where test_philox pins element 0 of one stream and checks the rest for mean
and variance."""
import numpy as np
import pytest
import torch

try:
    import philox_model
except ImportError:            # imported as tests.<module>: tests/ itself is not on sys.path
    from tests import philox_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = (0xA3C, 0x9E3779B97F4A7C15)          # a small seed (key word 1 = 0) and one that fills both key words
STREAMS = (3, 0x1234567800000002)            # likewise for counter words 2 and 3


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_philox_draws_match_the_model(ops, seed, stream):
    n = 100000
    u = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    ops.philox_uniform(seed, stream, u)
    np.testing.assert_array_equal(u.cpu().numpy(), philox_model.uniform(seed, stream, n))
    for high in (1, 2, 1978, 2 ** 31 - 1):
        r = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        ops.philox_randint(seed, stream, high, r)
        got = r.cpu().numpy()
        np.testing.assert_array_equal(got, philox_model.randint(seed, stream, high, n))
        assert got.min() >= 0 and got.max() < high
    # the row / stride / column form a sharded job draws with: rows of 37 out of a global row of 111
    rl, rst = 37, 111
    n = rl * 2703                                # 100011 elements
    for col0 in (0, 37, 74):
        u = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
        r = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        ops.philox_uniform(seed, stream, u, rl, rst, col0)
        ops.philox_randint(seed, stream, 1978, r, rl, rst, col0)
        np.testing.assert_array_equal(u.cpu().numpy(), philox_model.uniform(seed, stream, n, rl, rst, col0))
        np.testing.assert_array_equal(r.cpu().numpy(), philox_model.randint(seed, stream, 1978, n, rl, rst, col0))


@pytest.mark.parametrize("rows", [1, 257, 70000])
def test_gather_i32(ops, rows):
    """out[g] = src[idx[g]] with repeated and out-of-order indices; nothing past `rows` is written."""
    rs = np.random.RandomState(rows)
    src = rs.randint(-2 ** 31, 2 ** 31, size=1000, dtype=np.int64).astype(np.int32)
    idx = rs.randint(0, len(src), size=rows).astype(np.int32)
    idx[:3] = [999, 0, 999][:rows]
    out = torch.full((rows + 64,), -7, dtype=torch.int32, device=DEV)
    ops.gather_i32(dev(src), dev(idx), out[:rows])
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:rows], src[idx])
    assert (got[rows:] == -7).all()


@pytest.mark.parametrize("base_actor", [0, 5])
def test_ring_cur_idx(ops, base_actor):
    """(base_actor + b) * H1 + count[b] % H1: an empty ring, one just full, one wrapped once and one wrapped often."""
    B, H = 4, 6
    H1 = H + 1
    ring = ops.Ring(B, H, DEV)
    counts = np.array([0, H, H + 1, 7 * H1 + 3], np.int32)
    ring.count.copy_(dev(counts))
    want = (base_actor + np.arange(B)) * H1 + counts % H1
    np.testing.assert_array_equal(ring.cur_idx(base_actor=base_actor).cpu().numpy(), want)
    out = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    assert ring.cur_idx(out, base_actor) is out
    np.testing.assert_array_equal(out.cpu().numpy(), list(want) + [-7, -7])


@pytest.mark.parametrize("B", [1, 63, 64, 300, 4096])
def test_rollout_stats(ops, B):
    """stats += (env steps, finished episodes, the sum of their scores); score_valid is cleared, so a second call adds the
    steps again and no episodes.  Scores are multiples of 1/8 and the steps are integers: every partial sum is exact in
    a double whatever the order of the atomics."""
    rs = np.random.RandomState(B)
    n_steps = rs.randint(0, 21, size=B).astype(np.int32)
    valid = (rs.rand(B) < 0.4).astype(np.int32)
    valid[-1] = 1
    score = (rs.randint(-800, 800, size=B) / 8.0).astype(np.float32)
    d_steps, d_valid, d_score = dev(n_steps), dev(valid), dev(score)
    start = np.array([1000.0, 10.0, -2.5])
    stats = dev(start.copy())
    ops.rollout_stats(B, d_steps, d_valid, d_score, stats)
    want = start + [n_steps.sum(), valid.sum(), score[valid != 0].astype(np.float64).sum()]
    np.testing.assert_array_equal(stats.cpu().numpy(), want)
    assert not d_valid.any()
    np.testing.assert_array_equal(d_steps.cpu().numpy(), n_steps)
    np.testing.assert_array_equal(d_score.cpu().numpy(), score)
    ops.rollout_stats(B, d_steps, d_valid, d_score, stats)
    np.testing.assert_array_equal(stats.cpu().numpy(), want + [n_steps.sum(), 0, 0])
