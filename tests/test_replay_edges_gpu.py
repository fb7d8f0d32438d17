"""Replay sampling and the replay return scans at their decision edges (GPU).

unreal_replay_sample_rp / unreal_replay_sample_seq against the oracle on the case tables of tests/replay_cases.py
(what every case is there for is written there; test_replay_edges_cpu.py proves the tables reach it), and
unreal_vr_returns / unreal_pc_returns / unreal_seq_mask / unreal_seq_last_idx on index lists built by hand, so that the
branches a sampled sequence cannot reach are fed directly.  All index work is compared exactly."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

try:
    import margins
    import replay_cases as RC
except ImportError:            # imported as tests.<module>: tests/ itself is not on sys.path
    from tests import margins
    from tests import replay_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


def dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dt is not None:
        t = t.to(dt)
    return t.to(DEV).contiguous()


def ring_stub(B, H, **arrays):
    """What the replay entry points read of a Ring (B, H, H1, count and the per-frame attributes they name), without
    the frames: a Ring at H = 2000 holds 42 MB of them per actor."""
    return SimpleNamespace(B=B, H=H, H1=H + 1, **{k: dev(v) for k, v in arrays.items()})


@pytest.mark.parametrize("mode", RC.RP_MODES)
@pytest.mark.parametrize("H", RC.RP_H)
def test_replay_sample_rp_case_table(ops, H, mode):
    """Every case of (H, mode) in one launch, one actor per case: the three frame indices and the reward class, exact."""
    cases = RC.rp_cases(H, mode)
    B, H1 = len(cases), H + 1
    count, rr, coin, u = RC.rp_device_inputs(cases)
    ring = ring_stub(B, H, count=count, r_reward=rr.reshape(-1))
    rp_idx = torch.full((3 * B,), -1, dtype=torch.int32, device=DEV)
    rp_cls = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ops.replay_sample_rp(ring, dev(coin), dev(u), rp_idx, rp_cls, mode)
    ri = rp_idx.cpu().numpy().reshape(B, 3)
    rc = rp_cls.cpu().numpy()
    want_i = np.empty((B, 3), np.int64)
    want_c = np.empty(B, np.int64)
    for b, c in enumerate(cases):
        rp = c.exp.rp_from_draws(c.coin, lambda n: min(n - 1, int(c.u * n)))
        want_i[b] = [b * H1 + i % H1 for i in rp[:3]]
        r = c.exp.frames[rp[3]].reward
        want_c[b] = 0 if -1e-10 < r < 1e-10 else (1 if r > 0 else 2)
    bad = np.flatnonzero((ri != want_i).any(1) | (rc != want_c))
    assert bad.size == 0, "%d of %d cases differ; first: %s got %s class %d, want %s class %d" % (
        bad.size, B, cases[bad[0]][:6], ri[bad[0]] - bad[0] * H1, rc[bad[0]], want_i[bad[0]] - bad[0] * H1,
        want_c[bad[0]])


@pytest.mark.parametrize("H", RC.SEQ_H)
def test_replay_sample_seq_case_table(ops, H):
    """Hand-placed terminals (replay_cases.seq_cases): indices and lengths against sequence_from_start, exact, the
    padding rows equal to the last sampled index; then the mask and the bootstrap index of the same sequences."""
    cases = RC.seq_cases(H)
    B, H1, L = len(cases), H + 1, RC.SEQ_L
    ring = ring_stub(B, H, count=np.array([c.count for c in cases], np.int32),
                     r_terminal=np.stack([RC.terminal_row(c.exp) for c in cases]).reshape(-1))
    seq_idx = torch.full((L * B,), -1, dtype=torch.int32, device=DEV)
    seq_len = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ops.replay_sample_seq(ring, L, dev(np.array([c.start for c in cases], np.int32)), seq_idx, seq_len)
    si = seq_idx.cpu().numpy().reshape(L, B)
    sl = seq_len.cpu().numpy()
    for b, c in enumerate(cases):
        want = [b * H1 + i % H1 for i in c.exp.sequence_from_start(c.start, L)]
        assert sl[b] == len(want), c[:6]
        assert list(si[:, b]) == want + [want[-1]] * (L - len(want)), c[:6]
    msk = torch.full(((L - 1) * B,), -1, dtype=torch.int32, device=DEV)
    last = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ops.seq_mask(B, L - 1, seq_len, msk)
    ops.seq_last_idx(B, seq_idx, seq_len, last)
    np.testing.assert_array_equal(msk.cpu().numpy().reshape(L - 1, B), np.arange(L - 1)[:, None] < sl[None, :] - 1)
    np.testing.assert_array_equal(last.cpu().numpy(), si[sl - 1, np.arange(B)])


# ---------------------------------------------------------------------------------------------------
# return scans on built index lists
# ---------------------------------------------------------------------------------------------------
SCAN_KINDS = ("len1", "len2", "lenL", "term_n-2", "term_n-1")


def _built_sequences(B, H, L, kinds, rs):
    """seq_idx [L, B], seq_len [B] and r_terminal [B, H1] for the kinds:
      len1      one frame: every output row is 0, and there is no frame n - 2 to look at
      len2      the shortest sequence with an output row
      lenL      the full length, no terminal
      term_n-2  n frames whose SECOND-to-last is terminal: no bootstrap, R starts at 0 (trainer.py:355,395).  A sampled
                sequence stops at its first terminal, so the sampler never produces this
      term_n-1  n frames, only the last terminal: bootstrap
    Each sequence takes n distinct consecutive slots of its actor's ring from a random slot (wrapping), so a terminal
    flag belongs to one frame of it; the rows past n repeat the last index, as the sampler pads."""
    H1 = H + 1
    seq_idx = np.zeros((L, B), np.int32)
    seq_len = np.zeros(B, np.int32)
    term = np.zeros((B, H1), np.int32)
    for b in range(B):
        k = kinds[b % len(kinds)]
        n = {"len1": 1, "len2": 2, "lenL": L}.get(k) or int(rs.randint(3, L + 1))
        s0 = int(rs.randint(0, H1))
        slots = [(s0 + i) % H1 for i in range(n)]
        if k == "term_n-2":
            term[b, slots[n - 2]] = 1
        if k == "term_n-1":
            term[b, slots[n - 1]] = 1
        seq_idx[:, b] = [b * H1 + slots[min(i, n - 1)] for i in range(L)]
        seq_len[b] = n
    return seq_idx, seq_len, term


@pytest.mark.parametrize("B,kinds", [(1, (k,)) for k in SCAN_KINDS] + [(5, SCAN_KINDS), (300, SCAN_KINDS)])
def test_return_scans_on_built_sequences(ops, B, kinds):
    """unreal_vr_returns / unreal_pc_returns / unreal_seq_mask / unreal_seq_last_idx against the fp64 recurrence of
    trainer.py:354-372, 394-406.  Bars as in test_pc_vr_return_scans: value replay exact after rounding to fp32, pixel
    control atol 1e-7 + rtol 1e-6; rows at and beyond n - 1 exactly 0.  B = 300: two workgroups of value replay, 469 of
    pixel control."""
    H, L, CELLS = 40, 21, 400
    H1 = H + 1
    rs = np.random.RandomState(100 + B + len(kinds[0]))
    seq_idx, seq_len, term = _built_sequences(B, H, L, kinds, rs)
    rr = rs.normal(size=(B, H1)).astype(np.float32)
    rr[rs.rand(B, H1) < 0.3] = 0.0
    rpc = rs.uniform(0, 1, size=(B, H1, CELLS)).astype(np.float32)
    qmax = rs.uniform(0, 1, size=(B, CELLS)).astype(np.float32)
    bv = rs.normal(size=B).astype(np.float32)
    ring = ring_stub(B, H, r_reward=rr.reshape(-1), r_terminal=term.reshape(-1), r_pc=rpc.reshape(-1))
    d_idx, d_len = dev(seq_idx.reshape(-1)), dev(seq_len)
    pcR = torch.full(((L - 1) * B * CELLS,), np.nan, device=DEV)
    vrR = torch.full(((L - 1) * B,), np.nan, device=DEV)
    msk = torch.full(((L - 1) * B,), -1, dtype=torch.int32, device=DEV)
    last = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ops.pc_returns(ring, L, d_idx, d_len, dev(qmax.reshape(-1)), 0.9, pcR)
    ops.vr_returns(ring, L, d_idx, d_len, dev(bv), 0.99, vrR)
    ops.seq_mask(B, L - 1, d_len, msk)
    ops.seq_last_idx(B, d_idx, d_len, last)
    pcR = pcR.cpu().numpy().reshape(L - 1, B, CELLS)
    vrR = vrR.cpu().numpy().reshape(L - 1, B)
    want_pc = np.zeros((L - 1, B, CELLS))
    want_vr = np.zeros((L - 1, B))
    flat_t, flat_r, flat_pc = term.reshape(-1), rr.reshape(-1).astype(np.float64), rpc.reshape(-1, CELLS).astype(np.float64)
    for b in range(B):
        n = int(seq_len[b])
        fr = list(seq_idx[:n, b])[::-1]                  # the reference walks the sampled frames newest first
        boot = not (n >= 2 and flat_t[fr[1]])
        pc_R = qmax[b].astype(np.float64) if boot else np.zeros(CELLS)
        vr_R = float(bv[b]) if boot else 0.0
        for t, f in zip(range(n - 2, -1, -1), fr[1:]):
            pc_R = flat_pc[f] + 0.9 * pc_R
            vr_R = flat_r[f] + 0.99 * vr_R
            want_pc[t, b], want_vr[t, b] = pc_R, vr_R
    np.testing.assert_array_equal(vrR, want_vr.astype(np.float32))
    live = np.arange(L - 1)[:, None] < seq_len[None, :] - 1
    r = margins.record_close("pc_R", pcR[live], want_pc[live], 1e-7, 1e-6)
    assert r <= 1, "pc_R: worst |d| / (1e-7 + 1e-6 |ref|) = %g" % r
    assert (pcR[~live] == 0).all() and (vrR[~live] == 0).all()
    np.testing.assert_array_equal(msk.cpu().numpy().reshape(L - 1, B), live)
    np.testing.assert_array_equal(last.cpu().numpy(), seq_idx[seq_len - 1, np.arange(B)])
