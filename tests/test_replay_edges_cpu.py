"""The case tables of tests/replay_cases.py reach what they claim, and tests/philox_model.py is Philox4x32-10 (no GPU).

test_replay_edges_gpu.py and test_draws_gpu.py compare the device with these two; here the oracle alone walks the
tables, so that a table that stopped reaching a branch of sample_rp_kernel / sample_seq_kernel fails a test instead of
quietly checking less."""
import numpy as np
import pytest

import philox_model
import replay_cases as RC


@pytest.fixture(scope="module")
def rp_wants():
    return {(H, m): [(c, RC.rp_expected(c)) for c in RC.rp_cases(H, m)] for H in RC.RP_H for m in RC.RP_MODES}


@pytest.mark.parametrize("mode", RC.RP_MODES)
@pytest.mark.parametrize("H", RC.RP_H)
def test_rp_table_reaches_every_chunk_and_lane(rp_wants, H, mode):
    """The chunk loop: picks in chunk 0 and in the last chunk for every window of more than one chunk, in a middle chunk
    where there are three or more (H = 200, 2000), the last chunk partial wherever nw is no multiple of 64 (all but
    H = 131); picks at lane 0 and at lane 63 of a chunk later than the first; every count of the table."""
    wants = rp_wants[H, mode]
    nw = H - 3
    nch = (nw + 63) // 64
    assert {w.nchunks for _, w in wants} == {nch}
    assert {c.count for c, _ in wants} == set(RC.rp_counts(H))
    chunks = {w.chunk for _, w in wants}
    if H == 40 or H == 67:
        assert nch == 1 and chunks == {0}               # the control, and exactly one full chunk
        assert (H == 67) == any(w.lane == 63 for _, w in wants)
        return
    assert chunks == set(range(nch))                    # first, every middle and the last chunk
    if H in (200, 2000):
        assert nch >= 3
    last = [w for _, w in wants if w.chunk == nch - 1]
    tail = nw - 64 * (nch - 1)
    assert max(w.lane for w in last) == tail - 1        # the newest frame of the window, in the (partial) last chunk
    assert (tail < 64) == (H != 131)
    for count in RC.rp_counts(H):                       # at every ring phase
        later = [w for c, w in wants if c.count == count and w.chunk > 0]
        assert any(w.lane == 0 for w in later)
        if nw >= 128:
            assert any(w.lane == 63 for w in later)
        for pos in (True, False):                       # both buckets picked from the last chunk
            assert any(w.from_pos == pos and w.chunk == nch - 1 for c, w in wants if c.count == count)
    if nw > 128:                                        # +-1 at exactly 63 | 64 and 127 | 128: both signs, both sides
        offs = {(w.offset, w.cls) for c, w in wants if c.pattern == "edges"}
        assert {(63, 1), (64, 2), (127, 1), (128, 2)} <= offs


@pytest.mark.parametrize("mode", RC.RP_MODES)
@pytest.mark.parametrize("H", RC.RP_H)
def test_rp_table_reaches_overrides_and_rank_edges(rp_wants, H, mode):
    """The empty-bucket overrides under both coins, rank 0, rank n - 1 from u = 1 - 2**-53 (where int(u n) == n - 1, the
    last value the clamp lets through), and single-member buckets."""
    wants = rp_wants[H, mode]
    for coin in (0, 1):
        assert any(w.npos == 0 and c.coin == coin and not w.from_pos for c, w in wants)
        assert any(w.nneg == 0 and c.coin == coin and w.from_pos for c, w in wants)
    assert any(w.raw_rank == w.n - 1 and w.n == H - 3 and c.u == 1.0 - 2.0 ** -53 for c, w in wants)
    assert any(w.raw_rank == 0 and w.n == H - 3 for c, w in wants)
    assert all(0 <= w.raw_rank <= w.n - 1 for _, w in wants)
    assert any(w.n == 1 and w.from_pos for _, w in wants)
    # the slot outside the live range is never part of an answer, and it is poisoned
    for c, w in wants[::97]:
        row = RC.reward_row(c.exp)
        assert row[c.count % (H + 1)] == RC.POISON and RC.POISON not in row[w.slots]
    if mode == 0:                                       # all -1: an empty positive bucket in mode 0, an empty zero bucket in 1
        assert any(c.pattern == "neg" and w.npos == 0 for c, w in wants)
    else:
        assert any(c.pattern == "neg" and w.nneg == 0 for c, w in wants)


@pytest.mark.parametrize("H", RC.RP_H)
def test_rp_table_tells_bucket_rule_from_class_rule(rp_wants, H):
    """Rewards of +-1e-11: r > 0 (mode 0 bucket), r != 0 (mode 1 bucket) and |r| < 1e-10 (class 0) all disagree."""
    t0 = [(c, w) for c, w in rp_wants[H, 0] if c.pattern == "tiny"]
    t1 = [(c, w) for c, w in rp_wants[H, 1] if c.pattern == "tiny"]
    assert {w.cls for _, w in t0} == {0} and {w.cls for _, w in t1} == {0}
    assert any(w.from_pos and w.reward == RC.TINY for _, w in t0)              # positive bucket, class 0
    assert any(not w.from_pos and w.reward == -RC.TINY for _, w in t0)         # -1e-11 is in mode 0's other bucket
    assert any(w.from_pos and w.reward == -RC.TINY for _, w in t1)             # non-zero bucket, class 0
    assert any(w.from_pos and w.reward == RC.TINY for _, w in t1)
    assert any(not w.from_pos and w.reward == 0 for _, w in t1)
    # and the other patterns reach all three classes
    assert {w.cls for c, w in rp_wants[H, 0] if c.pattern == "dense"} == {0, 1, 2}


@pytest.mark.parametrize("H", RC.SEQ_H)
def test_seq_table_reaches_every_placement(H):
    L = RC.SEQ_L
    H1 = H + 1
    seen = set()
    wrapped = False
    for c in RC.seq_cases(H):
        x = c.exp
        assert 0 <= c.start <= H - L - 2
        assert all(not (x.frames[i].terminal and x.frames[i + 1].terminal) for i in range(x.top, x.count - 1))
        seq = x.sequence_from_start(c.start, L)
        s = x.top + c.start
        term = [x.frames[i].terminal for i in seq]
        shifted = seq[0] == s + 1
        assert shifted == c.placement.startswith(("on_start", "shift"))
        assert seq == list(range(seq[0], seq[0] + len(seq))) and seq[-1] < x.count
        want_len = {"none": L, "on_start": L, "after": 2, "on_Lth": L, "one_past": L, "shift_Lth": L, "shift_past": L}
        assert len(seq) == want_len[c.placement]
        ends_on_terminal = {"after", "on_Lth", "shift_Lth"}
        assert term[-1] == (c.placement in ends_on_terminal) and not any(term[:-1])
        if c.placement in ("one_past", "shift_past"):
            assert x.frames[seq[-1] + 1].terminal
        slots = [i % H1 for i in seq]
        wrapped |= any(a == H and b == 0 for a, b in zip(slots, slots[1:]))
        seen.add((c.placement, c.start == H - L - 2, c.count == H))
    for p in ("none", "on_start", "after", "on_Lth", "one_past", "shift_Lth", "shift_past"):
        assert (p, True, True) in seen and (p, True, False) in seen and (p, False, False) in seen
    assert wrapped


def test_philox_model_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter and key all zero, all ones, and the digits of pi."""
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in kat:
        got = philox_model.philox4x32_10_raw(ctr, key)
        assert tuple(int(x) for x in got) == want
    # vectorised over the counter, and through the device function's packing of (seed, index, stream)
    ctrs = np.array([k[0] for k in kat[:2]], dtype=np.uint64).T
    assert [int(x) for x in philox_model.philox4x32_10_raw(tuple(ctrs), (0, 0))[:, 0]] == list(kat[0][2])
    got = philox_model.philox4x32_10(0x299f31d0a4093822, [0x85a308d3243f6a88], 0x0370734413198a2e)
    assert tuple(int(x) for x in got[:, 0]) == kat[2][2]
    got = philox_model.philox4x32_10(2 ** 64 - 1, [2 ** 64 - 1], 2 ** 64 - 1)
    assert tuple(int(x) for x in got[:, 0]) == kat[1][2]


def test_philox_model_draws():
    """The two constructions the kernels use, on the zero vector, and the row / stride / column indexing."""
    u = philox_model.uniform(0, 0, 3)
    assert u[0] == ((0x6627e8d5 >> 5) * 67108864.0 + (0xe169c58d >> 6)) / 9007199254740992.0
    assert philox_model.randint(0, 0, 1978, 1)[0] == (0x6627e8d5 * 1978) >> 32
    assert (philox_model.randint(0, 0, 1, 50) == 0).all()
    g = philox_model.uniform(11, 9, 5 * 111)
    for col0 in (0, 37, 74):
        s = philox_model.uniform(11, 9, 5 * 37, 37, 111, col0)
        np.testing.assert_array_equal(s.reshape(5, 37), g.reshape(5, 111)[:, col0:col0 + 37])
    assert list(philox_model.draw_index(5, 2, 7, 3)) == [3, 4, 10, 11, 17]
