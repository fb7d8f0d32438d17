"""Case tables for the replay-sampling edge tests (test infrastructure, shared by test_replay_edges_cpu.py and
test_replay_edges_gpu.py so that both walk the same cases).

Reward-prediction sampling (unreal_replay_sample_rp, csrc/replay.hip sample_rp_kernel).  The kernel walks the window
[lo, cnt) = [count - H + 3, count) in chunks of 64 frames, twice: a counting pass, then a ranked pick that carries a
running count `run` across chunks and takes lane `k = rank - run` of the chunk that holds the rank.  One actor is one
case; a case is (H, count, mode, reward pattern, coin, u).  What each axis is there for:

  H        40 is the control (window of 37: one partial chunk, what the older tests use); 67 -> 64 (exactly one full chunk),
           68 -> 65 (a tail chunk of one frame), 131 -> 128 (two full chunks, no tail), 200 -> 197 (four chunks, tail of 5),
           2000 -> 1997 (production: 32 chunks, tail of 13).  These are the chunk loop's first / middle / last chunk.
  count    H (ring just full, top = 0), H + 1 (wrapped once: every slot shifted by one), 2H + 1, 5H + 37 (wrapped several
           times) and 3(H+1) + (H+1)//2 (slot 0 lies inside the window): the `a % H1` of every read.
  mode     0: buckets split on r > 0; 1: on r != 0.
  pattern  zero / pos / neg: the empty-bucket overrides (npos == 0 -> from_neg, nneg == 0 -> from_pos), under both coins;
           one@...: a bucket of ONE member at the first frame, the last frame, lane 63 of chunk 0 and lane 0 of chunk 1
           (the ballot mask `(1 << lane) - 1` at its ends, `end = lo + c + ...` with c > 0);
           edges: +-1 at exactly offsets 63, 64, 127, 128 (last lane / first lane of neighbouring chunks, both signs);
           sparse / dense: many members per bucket, `run +=` over many chunks;
           tiny: rewards of +-1e-11, for which the mode-0 bucket (r > 0), the mode-1 bucket (r != 0) and the reward class
           (|r| < 1e-10 -> zero, trainer.py:427-434) all disagree: the bucket rule against the class rule.
  draws    coin 0 / 1; u = 0 (rank 0), 0.5, 1 - 2**-53 (int(u n) = n - 1: the rank clamp's edge) and two fixed random
           values; for every non-empty bucket also the u = (k + 0.5) / n of the first and of the last member of every chunk
           (the pick in each chunk, at both ends of its ballot mask).

The slot count % H1 is the one slot of the ring outside the live range; it holds a poison reward (7.0) so that a read of
it changes the answer, and the three live frames before the window hold a reward of the bucket the window's first frame
is NOT in, so that a window that starts early does too.

Sequence sampling (unreal_replay_sample_seq): terminals placed by hand, see seq_cases()."""
import functools
from collections import namedtuple

import numpy as np

from oracle.experience import OracleExperience, Frame

RP_H = (40, 67, 68, 131, 200, 2000)
RP_MODES = (0, 1)
POISON = 7.0
TINY = float(np.float32(1e-11))
CHUNK = 64                              # frames per trip of sample_rp_kernel's two loops (one per lane)
U_FIXED = (0.0, 0.5, 1.0 - 2.0 ** -53) + tuple(np.random.RandomState(5).random_sample(2))


def rp_counts(H):
    return (H, H + 1, 2 * H + 1, 5 * H + 37, 3 * (H + 1) + (H + 1) // 2)


class FrozenExperience(OracleExperience):
    """An OracleExperience whose frames are set once: bucket() is the oracle's own, computed once per side."""

    def bucket(self, positive):
        c = self.__dict__.setdefault("_buckets", {})
        if positive not in c:
            c[positive] = OracleExperience.bucket(self, positive)
        return c[positive]


def _frame(reward=0.0, terminal=False):
    return Frame(None, float(reward), 0, bool(terminal), None, 0, 0.0)


def _patterns(nw, seed):
    """name -> fp32 rewards over the window offsets [0, nw)."""
    rs = np.random.RandomState(seed)
    z = lambda: np.zeros(nw, np.float32)
    out = {"zero": z(), "pos": z() + 1, "neg": z() - 1}
    for name, off in (("one@lo", 0), ("one@last", nw - 1), ("one@63", 63), ("one@64", 64)):
        if off < nw:
            out[name] = z()
            out[name][off] = 1
    e = z()
    for off, v in ((63, 1), (64, -1), (127, 1), (128, -1)):
        if off < nw:
            e[off] = v
    if e.any():
        out["edges"] = e
    x = rs.rand(nw)
    out["sparse"] = np.where(x < 0.03, 1, np.where(x < 0.06, -1, 0)).astype(np.float32)
    out["dense"] = rs.randint(-1, 2, size=nw).astype(np.float32)
    x = rs.rand(nw)
    out["tiny"] = np.where(x < 0.1, TINY, np.where(x < 0.2, -TINY, 0)).astype(np.float32)
    return out


def _is_pos(r, mode):
    return (r != 0) if mode else (r > 0)


def make_experience(H, count, mode, window_rewards):
    """The oracle replay with `count` frames appended, built directly: one Frame per live absolute index."""
    exp = FrozenExperience(H, lab_ver=bool(mode))
    exp.count = count
    lo = exp.top + 3
    assert len(window_rewards) == count - lo
    before = 0.0 if _is_pos(float(window_rewards[0]), mode) else 1.0
    for i in range(exp.top, lo):
        exp.frames[i] = _frame(before)
    for k, r in enumerate(window_rewards):
        exp.frames[lo + k] = _frame(float(r))           # the exact fp32 value, as a Python float
    return exp


def reward_row(exp):
    """The actor's [H1] slice of r_reward: frame i in slot i % H1, the one free slot poisoned."""
    H1 = exp.H + 1
    row = np.zeros(H1, np.float32)
    for i in range(exp.top, exp.count):
        row[i % H1] = exp.frames[i].reward
    row[exp.count % H1] = POISON
    return row


RpCase = namedtuple("RpCase", "H count mode pattern coin u exp")


@functools.lru_cache(maxsize=None)
def rp_cases(H, mode):
    """Every case of one (H, mode): the actors of one launch."""
    cases = []
    for ci, count in enumerate(rp_counts(H)):
        lo = max(0, count - H) + 3
        nw = count - lo
        for name, w in _patterns(nw, 1000 * H + ci).items():
            exp = make_experience(H, count, mode, w)
            draws = [(coin, u) for coin in (0, 1) for u in U_FIXED]
            for coin, positive in ((1, True), (0, False)):
                b = exp.bucket(positive)
                n = len(b)
                chunk = [(i - lo) // CHUNK for i in b]
                for k in range(n):
                    if k == 0 or k == n - 1 or chunk[k] != chunk[k - 1] or chunk[k] != chunk[k + 1]:
                        draws.append((coin, (k + 0.5) / n))       # first / last member of its chunk
            cases += [RpCase(H, count, mode, name, coin, u, exp) for coin, u in draws]
    return tuple(cases)


def reference_class(r):
    """trainer.py:427-434."""
    return 0 if -1e-10 < r < 1e-10 else (1 if r > 0 else 2)


RpWant = namedtuple("RpWant", "slots cls offset chunk lane nchunks from_pos npos nneg n raw_rank reward")


def rp_expected(case):
    """What the oracle picks for a case: the three slots (without the actor's b * H1) and the class, and where in the
    chunk loop that pick lies."""
    exp, H1 = case.exp, case.H + 1
    seen = []

    def pick(n):
        seen.append((n, int(case.u * n)))
        return min(n - 1, int(case.u * n))
    rp = exp.rp_from_draws(case.coin, pick)
    (n, raw), = seen
    lo = exp.top + 3
    nw = exp.count - lo
    off = rp[3] - lo
    pos = exp.bucket(True)
    r = exp.frames[rp[3]].reward
    return RpWant([i % H1 for i in rp[:3]], reference_class(r), off, off // CHUNK, off % CHUNK,
                  (nw + CHUNK - 1) // CHUNK, _is_pos(r, case.mode), len(pos), nw - len(pos), n, raw, r)


def rp_device_inputs(cases):
    """count [B] i32, r_reward [B, H1] f32, coin [B] i32, u [B] f64 of one launch."""
    rows = {}
    for c in cases:
        if id(c.exp) not in rows:
            rows[id(c.exp)] = reward_row(c.exp)
    return (np.array([c.count for c in cases], np.int32), np.stack([rows[id(c.exp)] for c in cases]),
            np.array([c.coin for c in cases], np.int32), np.array([c.u for c in cases], np.float64))


# ---------------------------------------------------------------------------------------------------
# sequence sampling: terminals placed by hand (experience.py:100-118)
# ---------------------------------------------------------------------------------------------------
SEQ_H = (40, 2000)
SEQ_L = 21

SeqCase = namedtuple("SeqCase", "H L count start placement terminals exp")


@functools.lru_cache(maxsize=None)
def seq_cases(H, L=SEQ_L):
    """(count, start, terminal placement) with no two terminals in succession.  Placements, relative to s = top + start:
      none        length L, nothing special (control)
      on_start    terminal on s: the start shifts by one (experience.py:105-107)
      after       terminal on s + 1: length 2
      on_Lth      terminal on s + L - 1: length L, ending on the terminal
      one_past    terminal on s + L: length L, no terminal inside
      shift_Lth   terminal on s and on s + L: the shifted sequence ends on its L-th frame
      shift_past  terminal on s and on s + L + 1: shifted, length L, the second terminal one past it
    Starts: 0, 7, the largest legal draw H - L - 2 (randint(0, H - L - 1)), and at count = 3 H1 + L the start whose slots
    run H - 5 .. H, 0, 1, ...: through the end of the ring's storage."""
    H1 = H + 1
    place = {"none": (), "on_start": (0,), "after": (1,), "on_Lth": (L - 1,), "one_past": (L,),
             "shift_Lth": (0, L), "shift_past": (0, L + 1)}
    cases = []
    for count in (H, H + 1, 3 * H1 + L):
        top = count - H
        starts = [0, 7, H - L - 2]
        if count == 3 * H1 + L:
            starts.append(H - L - 6)
        for start in starts:
            for name, offs in place.items():
                term = tuple(top + start + o for o in offs)
                if any(t >= count for t in term):
                    continue
                exp = OracleExperience(H)
                exp.count = count
                for i in range(top, count):
                    exp.frames[i] = _frame(terminal=i in term)
                cases.append(SeqCase(H, L, count, start, name, term, exp))
    return tuple(cases)


def terminal_row(exp):
    H1 = exp.H + 1
    row = np.zeros(H1, np.int32)
    for i in range(exp.top, exp.count):
        row[i % H1] = int(exp.frames[i].terminal)
    row[exp.count % H1] = 1                              # the free slot: a read past the newest frame ends the sequence
    return row
