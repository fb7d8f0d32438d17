"""CPU tests of the versus step and the opponent pool: option validation and refusals, the entries'
declarations, binding table and wrappers, the launcher's host checks with fake pointers, the pool's snapshot rule and slot
assignment by value, the checkpoint's key, and, on the host model of tests/selfplay_model.py alone, that learner b of a
versus batch is HostSeat 2 (base + b) and the opponent's view HostSeat 2 (base + b) + 1."""
import os

import numpy as np
import pytest

try:
    import selfplay_model as SM
except ImportError:            # imported as tests.<module>
    from tests import selfplay_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("unreal_arcade_versus_reset", "unreal_arcade_versus_step", "unreal_arcade_versus_rollout_step",
           "unreal_arcade_versus_policy_rollout_step", "unreal_arcade_versus_rollout_step_tl",
           "unreal_arcade_versus_policy_rollout_step_tl")


def _sp(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeSelfPlay
    return ArcadeSelfPlay(**kw)


# ---- options ---------------------------------------------------------------------------------------------------------------
def test_opponent_options_and_their_refusals():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.train.trainer import Trainer
    from unreal_amd import options
    flags = options.get_options("training")
    assert (flags.opponent_pool, flags.opponent_snapshot_every) == (0, 100)
    flags = options.get_options("training", argv=["--opponent_pool", "4", "--opponent_snapshot_every", "200"])
    assert (flags.opponent_pool, flags.opponent_snapshot_every) == (4, 200)
    chk = Trainer.check_opponent_options
    try:
        Environment.register_arcade_selfplay("vscpu")
        Environment.register_arcade_config("vscpu_duel", game="duel")
        assert chk("arcade", "vscpu", 8, 2, 0) == (0, 100)
        assert chk("maze", "whatever", 7, 1, 0, 5) == (0, 5)          # no pool: any environment
        assert chk("arcade", "vscpu", 8, 2, 4, 3) == (4, 3)
        assert chk("arcade", "vscpu", 3, 1, 1) == (1, 100)            # every actor is a learner: odd counts are fine
        assert chk("arcade", "vscpu", 9, 3, 3, 1) == (3, 1)
        assert chk("arcade", "vscpu", 32, 2, 16) == (16, 100)
        with pytest.raises(ValueError, match="pairs"):                # ... while mirror self-play keeps its even rule
            Trainer.check_selfplay_options("arcade", "vscpu", 3, 1)
        for env_type, name in (("arcade", "vscpu_duel"), ("maze", "vscpu"), ("lab", "nav_maze_static_01"),
                               ("gym", "Pong"), ("indoor", "x")):     # no self-play name; host-fed environments
            with pytest.raises(ValueError, match="self-play"):
                chk(env_type, name, 8, 1, 2)
        for B, G, K in ((8, 1, 3), (8, 2, 8), (12, 3, 3), (6, 1, 4)):  # K does not divide batch_size // groups
            with pytest.raises(ValueError, match="divide"):
                chk("arcade", "vscpu", B, G, K)
        for K in (-1, 17, 2.0, True, None, "2"):
            with pytest.raises(ValueError, match="opponent_pool"):
                chk("arcade", "vscpu", 32, 1, K)
        for N in (0, -3, 1.5, True, None):
            with pytest.raises(ValueError, match="opponent_snapshot_every"):
                chk("arcade", "vscpu", 8, 1, 2, N)
            with pytest.raises(ValueError, match="opponent_snapshot_every"):
                chk("arcade", "vscpu", 8, 1, 0, N)
        tr = object.__new__(Trainer)                                  # the accessors refuse a trainer without a pool
        tr.opponent_pool, tr.environment = 0, None
        for call in (lambda: tr.opponent(0), tr.opponent_ages, tr.opponent_scores, tr.opponent_state,
                     lambda: tr.load_opponent_state(None)):
            with pytest.raises(ValueError, match="opponent pool"):
                call()
    finally:
        Environment.ARCADE_CONFIG.pop("vscpu", None)
        Environment.ARCADE_CONFIG.pop("vscpu_duel", None)


def test_versus_needs_a_selfplay_config_and_takes_odd_counts():
    from unreal_amd.environment.arcade_environment import (BatchedArcadeEnvironment, ArcadeConfig, ArcadeMix,
                                                           ArcadeOpponent)
    import torch
    for conf in (ArcadeConfig(game="duel"), ArcadeConfig(), ArcadeConfig(game="invaders"), ArcadeMix([ArcadeConfig()])):
        with pytest.raises(ValueError, match="versus"):
            BatchedArcadeEnvironment(4, 2, "cpu", config=conf, versus=True)
    with pytest.raises(ValueError, match="pairs"):                    # without versus the pairs' rule stands
        BatchedArcadeEnvironment(3, 2, "cpu", config=_sp())
    # the opponent's buffers and their views, odd bounds included (host memory: nothing is launched)
    o = ArcadeOpponent(6, torch.device("cpu"))
    assert o.frames.numel() == 6 * 21168 and o.frame_stride == 21168 and o.frame_shape == (84, 84)
    assert (o.actions.dtype, o.last_action.dtype, o.last_reward.dtype, o.frames.dtype) == \
        (torch.int32, torch.int32, torch.float32, torch.uint8)
    v = o.view(1, 4)
    assert v.B == 3 and v.frames.numel() == 3 * 21168 and v.frame_stride == 21168 and v.frame_shape == (84, 84)
    assert v.frames.data_ptr() == o.frames.data_ptr() + 21168 and v.frames.data_ptr() % 16 == 0
    for name in ("actions", "last_action", "last_reward"):
        assert getattr(v, name).data_ptr() == getattr(o, name).data_ptr() + 4 and getattr(v, name).numel() == 3
    env = object.__new__(BatchedArcadeEnvironment)                    # view() of a versus environment takes odd bounds
    env.config, env.opponent, env.B = _sp(), o, 6
    env.ring = __import__("unreal_amd.ops", fromlist=["Ring"]).Ring(6, 2, torch.device("cpu"), arcade=True)
    block = torch.zeros(24, dtype=torch.int32)
    env.arcade = (block, 5, "versus", o)
    w = env.view(1, 4)
    assert w.B == 3 and w.arcade[:3] == (block, 6, "versus") and w.arcade[3] is w.opponent and w.opponent.B == 3
    assert w.opponent.frames.data_ptr() == v.frames.data_ptr()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
class FakeCuda(object):                                           # what _chk reads of a tensor
    is_cuda = True

    def __init__(self, n, dtype, p=1 << 20):
        self.n, self.dtype, self.p = n, dtype, p

    def is_contiguous(self):
        return True

    def numel(self):
        return self.n

    def data_ptr(self):
        return self.p


def test_entries_are_declared_documented_and_wrapped():
    from unreal_amd import _lib, ops
    import ctypes
    import torch
    protos = _lib.parse_header()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    assert header.count("[1] action_repeat - 1") == 2
    for name in ENTRIES:
        plain = protos[name.replace("_versus", "")]
        assert name in protos and protos[name] == plain[:-1] + [ctypes.c_void_p] * 4 + plain[-1:], name
        assert name in text, name
    ring = ops.Ring(5, 2, torch.device("cpu"), arcade=True)
    for name in ("ep_steps", "episode", "arcade"):
        setattr(ring, name, FakeCuda(getattr(ring, name).numel(), torch.int32))

    def opp(**kw):
        o = type("O", (), {})()
        o.actions, o.last_action = FakeCuda(5, torch.int32, 1 << 21), FakeCuda(5, torch.int32, 1 << 22)
        o.last_reward, o.frames = FakeCuda(5, torch.float32, 1 << 23), FakeCuda(5 * 21168, torch.uint8, 1 << 24)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    block = FakeCuda(24, torch.int32)
    family, tail, rest = ops._arcade_args(ring, (block, 3, ops.ARCADE_VERSUS, opp()))
    assert family == "_versus" and len(tail) == 5 and tail[1] == 3
    assert rest == (1 << 21, 1 << 24, 1 << 22, 1 << 23)              # actions, frames, last_action, last_reward
    assert ops._arcade_args(ring, (block, 3, ops.ARCADE_VERSUS, opp()), stats=False)[2] == rest       # reset takes them too
    assert ops._arcade_args(ring, (block, 2))[0] == "" and ops._arcade_args(ring, (block, 2, ops.ARCADE_SELFPLAY))[0] == "_selfplay"
    with pytest.raises(ValueError, match="family"):
        ops._arcade_args(ring, (block, 3, ops.ARCADE_SELFPLAY, opp()))
    with pytest.raises(ValueError, match="arcade config"):
        ops._arcade_args(ring, (FakeCuda(23, torch.int32), 3, ops.ARCADE_VERSUS, opp()))
    for bad, what in ((dict(actions=FakeCuda(4, torch.int32)), "opponent.actions"),
                      (dict(actions=None), "opponent.actions"),
                      (dict(actions=FakeCuda(5, torch.float32)), "opponent.actions"),
                      (dict(frames=FakeCuda(5 * 21168 - 1, torch.uint8)), "opponent.frames"),
                      (dict(frames=FakeCuda(5 * 21168, torch.int32)), "opponent.frames"),
                      (dict(frames=FakeCuda(5 * 21168, torch.uint8, (1 << 24) + 8)), "16-byte"),
                      (dict(last_action=FakeCuda(5, torch.float32)), "opponent.last_action"),
                      (dict(last_action=None), "opponent.last_action"),
                      (dict(last_reward=FakeCuda(5, torch.int32)), "opponent.last_reward"),
                      (dict(last_reward=FakeCuda(4, torch.float32)), "opponent.last_reward")):
        with pytest.raises(ValueError, match=what):
            ops._arcade_args(ring, (block, 3, ops.ARCADE_VERSUS, opp(**bad)))


def test_entries_refuse_bad_arguments_without_a_launch():
    """Fake device pointers: every call below is refused by the host check, so none reaches a kernel."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    f = _lib.lib()._fn
    EINVAL = -22
    dev = 1 << 20
    ring = [None] + [dev] * 10 + [None, None] + [dev] * 3    # pos .. score_valid

    def heads(B):
        h = {ENTRIES[0]: [B, 3, None, None, dev, dev, dev, dev],
             ENTRIES[1]: [B, 3, dev, None] + ring + [1, 1],
             ENTRIES[2]: [B, 3, dev] + ring + [dev] * 4 + [None, None, 0, 0, 4, 0],
             ENTRIES[3]: [B, 3, dev, 256] + [dev] * 8 + ring + [dev] * 4 + [None, None, 0, 0, 4, 0]}
        h[ENTRIES[4]], h[ENTRIES[5]] = h[ENTRIES[2]], h[ENTRIES[3]]
        return h

    def call(name, B=3, tail=None, head=None, store=dev, opp=None):
        tail = [dev, 1, dev, dev, dev] if tail is None else tail       # cfg, actor_base, ep_steps, episode, records
        fin = [store] if name.endswith("_tl") else []
        opp = [dev, dev, dev, dev] if opp is None else opp             # opp_actions, opp_frames, opp_last_action, opp_last_reward
        return f[name](*(heads(B)[name] if head is None else head), *tail, *fin, *opp, None)

    for name in ENTRIES:
        for opp in ([dev, None, dev, dev], [dev, dev + 8, dev, dev], [dev, dev + 4, dev, dev], [dev, dev + 1, dev, dev],
                    [dev, dev, None, dev], [dev, dev, dev, None]):
            assert call(name, opp=opp) == EINVAL, (name, opp)
        if name != ENTRIES[0]:                                             # (reset reads no opponent action)
            assert call(name, opp=[None, dev, dev, dev]) == EINVAL, name
        # what the plain entries refuse
        for tail in ([None, 0, dev, dev, dev], [dev + 2, 0, dev, dev, dev], [dev, -2, dev, dev, dev],
                     [dev, 0, None, dev, dev], [dev, 0, dev, None, dev], [dev, 0, dev, dev, None],
                     [dev, 2 ** 30, dev, dev, dev]):                       # 2 (actor_base + b) would not fit an int
            assert call(name, tail=tail) == EINVAL, (name, tail)
        assert call(name, head=[0] + heads(4)[name][1:]) == EINVAL, name
        assert call(name, head=[4, 1] + heads(4)[name][2:]) == EINVAL, name
    for name in ENTRIES[2:]:                                               # A != 4 in the rollout forms
        assert call(name, head=heads(4)[name][:-2] + [6, 0]) == EINVAL, name
    for name in ENTRIES[4:]:                                               # the _tl forms: a null or misaligned store
        for store in (None, dev + 8):
            assert call(name, store=store) == EINVAL, (name, store)


# ---- the pool's rules, by value ---------------------------------------------------------------------------------------------------
def _simulate(K, N, calls):
    """The pool over process() calls that apply `calls[i]` updates each -> per call (slot written or None, s, ages)."""
    from unreal_amd.train.trainer import Trainer
    u = s = 0
    taken = [0] * K
    out = []
    for n in calls:
        taken[0] = u                                   # slot 0: the present self at the call's start
        u += n
        slot, s = Trainer.opponent_snapshot(K, N, u, s)
        if slot is not None:
            taken[slot] = u
        out.append((slot, s, [u - t for t in taken]))
    return out


def test_the_snapshot_rule_by_value():
    from unreal_amd.train.trainer import Trainer
    snap = Trainer.opponent_snapshot
    # one update a call
    assert [r[0] for r in _simulate(2, 1, [1] * 5)] == [1, 1, 1, 1, 1]
    assert [r[0] for r in _simulate(4, 1, [1] * 7)] == [1, 2, 3, 1, 2, 3, 1]
    assert [r[0] for r in _simulate(2, 3, [1] * 7)] == [None, None, 1, None, None, 1, None]
    assert [r[0] for r in _simulate(4, 3, [1] * 10)] == [None, None, 1, None, None, 2, None, None, 3, None]
    assert [r[1] for r in _simulate(4, 3, [1] * 10)] == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3]
    # four updates a call (two groups of 2 x 1 minibatch updates, say): N = 3 is crossed once in call 1, once in call 2,
    # TWICE in call 3 (u = 8 -> 12 passes 9 and 12): one snapshot, and s jumps to u // N
    r = _simulate(4, 3, [4] * 4)
    assert [x[0] for x in r] == [1, 2, 3, 2] and [x[1] for x in r] == [1, 2, 4, 5]
    r = _simulate(2, 3, [4] * 4)
    assert [x[0] for x in r] == [1, 1, 1, 1] and [x[1] for x in r] == [1, 2, 4, 5]
    assert [x[0] for x in _simulate(4, 1, [4] * 3)] == [1, 2, 3] and [x[1] for x in _simulate(4, 1, [4] * 3)] == [4, 8, 12]
    # ages: slot 0 is as old as the call's updates, a slot just written 0, the others grow
    r = _simulate(4, 1, [1] * 4)
    assert [x[2] for x in r] == [[1, 0, 1, 1], [1, 1, 0, 2], [1, 2, 1, 0], [1, 0, 2, 1]]
    assert [x[2] for x in _simulate(2, 3, [4] * 2)] == [[4, 0], [4, 0]]
    assert [x[2] for x in _simulate(4, 3, [1] * 4)] == [[1, 1, 1, 1], [1, 2, 2, 2], [1, 0, 3, 3], [1, 1, 4, 4]]
    # K = 1 never snapshots, whatever N
    for N in (1, 3):
        for calls in ([1] * 6, [4] * 3):
            assert all(x[0] is None and x[1] == 0 for x in _simulate(1, N, calls))
    assert snap(1, 1, 100, 0) == (None, 0)
    # the rule itself
    assert snap(4, 3, 2, 0) == (None, 0) and snap(4, 3, 3, 0) == (1, 1) and snap(4, 3, 5, 1) == (None, 1)
    assert snap(4, 3, 12, 2) == (3, 4) and snap(4, 3, 13, 4) == (None, 4) and snap(4, 3, 15, 4) == (2, 5)


def test_the_slot_assignment_by_value():
    from unreal_amd.train.trainer import Trainer
    slots = Trainer.opponent_slots
    assert slots(8, 1) == [0] * 8
    assert slots(8, 2) == [0, 0, 0, 0, 1, 1, 1, 1]
    assert slots(8, 4) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert slots(8, 8) == list(range(8))
    assert slots(3, 3) == [0, 1, 2] and slots(9, 3) == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    for Bg, K in ((8, 3), (8, 0), (8, 16), (4, 8), (8, 17), (8, True), (8, 2.0)):
        with pytest.raises(ValueError):
            slots(Bg, K)


def test_a_checkpoint_carries_the_pool_under_its_own_key(tmp_path):
    import torch
    import warnings
    from unreal_amd import checkpoint

    class Flat(object):
        def __init__(self, n):
            self.flat = torch.arange(n, dtype=torch.float32)
            self.offsets = {"w": (0, n, (n,))}

    class Net(object):
        spec = [("w", (5,), 5)]
        image_shape = (84, 84)

        def __init__(self):
            self.params = Flat(5)

    class Pool(object):
        got = "unset"

        def load_opponent_state(self, d):
            self.got = d
    net = Net()
    state = dict(params=[torch.full((5,), float(k)) for k in range(3)], updates=7, snapshots=3, taken=[7, 6, 5])
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    checkpoint.save(d1, net, None, 100, 1.5, opponents=state)
    checkpoint.save(d2, net, None, 100, 1.5)                          # the existing call form: no key
    p1 = torch.load(checkpoint.list_checkpoints(d1)[-1][1], weights_only=True)
    p2 = torch.load(checkpoint.list_checkpoints(d2)[-1][1], weights_only=True)
    assert "opponents" in p1 and "opponents" not in p2 and set(p1) - {"opponents"} == set(p2)
    pool = Pool()
    assert checkpoint.restore(d1, net, opponents=pool)[0] == 100
    assert pool.got["updates"] == 7 and pool.got["snapshots"] == 3 and pool.got["taken"] == [7, 6, 5]
    assert all(torch.equal(a, b) for a, b in zip(pool.got["params"], state["params"]))
    pool = Pool()
    assert checkpoint.restore(d2, net, opponents=pool)[0] == 100      # a file without the key: the pool is told so
    assert pool.got is None
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert checkpoint.restore(d1, net)[0] == 100                  # the existing call form reads either file
        assert checkpoint.restore(d2, net)[0] == 100
    assert not [w for w in seen if issubclass(w.category, UserWarning)]


# ---- the host model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 3])
def test_a_versus_batch_is_seat_zero_with_a_scripted_partner_and_the_opponent_view_is_seat_one(base):
    """Learner b of a versus batch (one game stepped once with both actions, keyed by 2 (base + b)) against HostSeat
    2 (base + b) with the opponent's actions as its script, and the opponent's view (M of the canonical record, its render,
    its reward) against HostSeat 2 (base + b) + 1 scripted with the learner's actions: an even and an odd base."""
    conf = _sp(**SM.TRACE_SETTINGS[1])
    B, steps, seed = 5, 200, 11
    rs = np.random.RandomState(base)
    games = [SM.TwoSeatDuel(conf, 2 * (base + b), seed) for b in range(B)]       # the versus step: ONE game per learner
    learners = [SM.HostSeat(conf, 2 * (base + b), seed, partner=[]) for b in range(B)]
    opps = [SM.HostSeat(conf, 2 * (base + b) + 1, seed, partner=[]) for b in range(B)]
    frames = [SM.render_record(conf, g.record()) for g in games]
    ends, rewards = 0, set()
    for s in range(steps):
        acts, oacts, active = rs.randint(0, 4, B), rs.randint(0, 4, B), rs.rand(B) < 0.9
        for b in range(B):
            if not active[b]:
                continue
            r0, r1, t = games[b].step(acts[b], oacts[b])
            learners[b].partner.append(oacts[b]); opps[b].partner.append(acts[b])
            _, lr, lt, lpc = learners[b].process(acts[b])
            _, orew, ot, _ = opps[b].process(oacts[b])
            assert (r0, t) == (lr, lt) and (r1, t) == (orew, ot), (s, b)
            rec = games[b].record()
            np.testing.assert_array_equal(rec, learners[b].record())
            np.testing.assert_array_equal(SM.mirror(rec), opps[b].record())
            frame = SM.render_record(conf, rec)
            np.testing.assert_array_equal(frame, learners[b].frame)
            np.testing.assert_array_equal(SM.pixel_change(frame, frames[b]), lpc)
            np.testing.assert_array_equal(SM.render_record(conf, SM.mirror(rec)), opps[b].frame)
            assert (opps[b].last_action, opps[b].last_reward) == (oacts[b], r1)
            frames[b] = frame
            rewards |= {r0, r1}
            if t:
                ends += 1
                games[b].reset(); learners[b].reset(); opps[b].reset()
                frames[b] = SM.render_record(conf, games[b].record())
                np.testing.assert_array_equal(SM.render_record(conf, SM.mirror(games[b].record())), opps[b].frame)
                assert (games[b].episode, games[b].ep_steps) == (learners[b].episode, learners[b].ep_steps)
    assert ends > 5 and {7, -3, 2, 0} <= rewards, (ends, rewards)
