"""CPU tests of the self-play duel: ArcadeSelfPlay and its registration, the refusals of odd actor counts, the
entries' declarations and host checks, and, on the host model of tests/selfplay_model.py alone, the mirror, the reduction
to the scripted duel, the zero sum, seat 1's frame, and that the traces of tests/test_selfplay_gpu.py hold every event."""
import os

import numpy as np
import pytest

try:
    import selfplay_model as SM
    import duel_model as DM
except ImportError:            # imported as tests.<module>
    from tests import selfplay_model as SM
    from tests import duel_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("unreal_arcade_selfplay_reset", "unreal_arcade_selfplay_step", "unreal_arcade_selfplay_rollout_step",
           "unreal_arcade_selfplay_policy_rollout_step", "unreal_arcade_selfplay_rollout_step_tl",
           "unreal_arcade_selfplay_policy_rollout_step_tl")


def _sp(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeSelfPlay
    return ArcadeSelfPlay(**kw)


# ---- the config ---------------------------------------------------------------------------------------------------------------
def test_the_config_is_the_duels_and_its_block_is_the_scripted_duels():
    from unreal_amd.environment.arcade_environment import ArcadeConfig, GAMES, GAME_IDS
    assert GAMES == {"breakout": 1, "duel": 3} and "selfplay" not in GAME_IDS
    conf = _sp()
    assert conf.game == "selfplay" and conf.action_size == 4
    assert isinstance(conf.scripted, ArcadeConfig) and conf.scripted.game == "duel"
    want = ArcadeConfig(game="duel")
    for name in ("points", "paddle_width", "paddle_speed", "ball_speed", "serve_wait", "win_reward", "lose_reward",
                 "max_episode_steps", "action_repeat", "return_reward", "opponent_speed"):
        assert getattr(conf, name) == getattr(want, name) == getattr(conf.scripted, name), name
    for kw in SM.TRACE_SETTINGS + [dict(paddle_width=20, opponent_speed=5)]:
        conf = _sp(**kw)
        assert conf.scripted.opponent_width == conf.paddle_width
        for seed in (0, 7, 2 ** 40 + 3):
            block = conf.block(seed)
            np.testing.assert_array_equal(block, conf.scripted.block(seed))
            np.testing.assert_array_equal(block, ArcadeConfig(game="duel", opponent_width=conf.paddle_width, **kw).block(seed))
            assert block[0] == 3 and block[9] == block[6]


def test_the_config_refuses_what_the_duel_refuses_and_an_opponent_width():
    for bad in (dict(points=0), dict(points=10), dict(paddle_width=5), dict(paddle_width=26), dict(ball_speed=5),
                dict(win_reward=-1), dict(lose_reward=1), dict(action_repeat=9), dict(return_reward=-1),
                dict(max_episode_steps=0), dict(opponent_speed=9), dict(paddle_speed=True)):
        with pytest.raises(ValueError):
            _sp(**bad)
    for bad in (dict(opponent_width=12), dict(game="duel"), dict(lives=3), dict(rows=2)):
        with pytest.raises((TypeError, ValueError)):
            _sp(**bad)


def test_registration_and_what_refuses_a_selfplay_task():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import ArcadeMix, ArcadeSelfPlay
    try:
        Environment.register_arcade_selfplay("spcpu", points=3, win_reward=7, lose_reward=-3)
        conf = Environment.arcade_config("spcpu")
        assert isinstance(conf, ArcadeSelfPlay) and (conf.points, conf.win_reward, conf.lose_reward) == (3, 7, -3)
        assert Environment.get_action_size("arcade", "spcpu") == 4
        with pytest.raises((TypeError, ValueError)):
            Environment.register_arcade_selfplay("spcpu_bad", opponent_width=12)
        assert "spcpu_bad" not in Environment.ARCADE_CONFIG
        with pytest.raises(ValueError):
            ArcadeMix([conf])
        with pytest.raises(ValueError):
            Environment.register_arcade_mix("spcpu_mix", ["spcpu"])
        assert "spcpu_mix" not in Environment.ARCADE_CONFIG
    finally:
        Environment.ARCADE_CONFIG.pop("spcpu", None)


def test_odd_batches_bases_and_view_bounds_are_refused_before_any_device_memory():
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    conf = _sp()
    for batch, base, total in ((3, 0, 3), (1, 0, 1), (4, 1, 6), (2, 3, 6)):
        with pytest.raises(ValueError, match="pairs"):
            BatchedArcadeEnvironment(batch, 2, "cpu", config=conf, actor_base=base, actors_total=total)
    env = object.__new__(BatchedArcadeEnvironment)              # view() checks the bounds before it touches the ring
    env.config = conf
    for b0, b1 in ((1, 4), (0, 3), (1, 3)):
        with pytest.raises(ValueError, match="odd"):
            env.view(b0, b1)


def test_the_trainer_and_evaluate_refusals():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.train.trainer import Trainer
    from unreal_amd.evaluate import Evaluate
    try:
        Environment.register_arcade_selfplay("spcpu_tr")
        Environment.register_arcade_config("spcpu_duel", game="duel")
        assert Trainer.check_selfplay_options("arcade", "spcpu_tr", 4, 2) is True
        assert Trainer.check_selfplay_options("arcade", "spcpu_tr", 8, 1) is True
        assert Trainer.check_selfplay_options("arcade", "spcpu_duel", 3, 3) is False
        assert Trainer.check_selfplay_options("maze", "whatever", 3, 1) is False
        for B, G in ((3, 1), (6, 2), (4, 4), (6, 6), (10, 2)):      # an odd rank, odd actors per group
            with pytest.raises(ValueError, match="pairs"):
                Trainer.check_selfplay_options("arcade", "spcpu_tr", B, G)
        # the options of a single game are accepted
        assert Trainer.check_rollout_options("arcade", "spcpu_tr", True, 0.95) == (True, 0.95)
        assert Trainer.check_reuse_options("arcade", 2, 0.2) == (2, 0.2)
        assert Trainer.check_minibatch_options("arcade", 4, 1, 2) == 2
        net = object()
        for kw in (dict(arcade="spcpu_duel"), dict(), dict(maze="nothing"), dict(arcade="spcpu_tr", simulator=object())):
            with pytest.raises(ValueError, match="versus"):
                Evaluate(net, batch_size=4, device="cpu", versus=net, **kw)
        with pytest.raises(ValueError, match="even"):
            Evaluate(net, batch_size=3, device="cpu", versus=net, arcade="spcpu_tr")
    finally:
        Environment.ARCADE_CONFIG.pop("spcpu_tr", None)
        Environment.ARCADE_CONFIG.pop("spcpu_duel", None)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_documented_and_wrapped():
    from unreal_amd import _lib, ops
    import torch
    protos = _lib.parse_header()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in protos and protos[name] == protos[name.replace("_selfplay", "")], name    # the plain argument lists
        assert name in text, name

    class FakeCuda(object):                                       # what _chk reads of a tensor
        is_cuda, dtype = True, torch.int32

        def __init__(self, n):
            self.n = n

        def is_contiguous(self):
            return True

        def numel(self):
            return self.n

        def data_ptr(self):
            return 1 << 20

    ring = ops.Ring(4, 2, torch.device("cpu"), arcade=True)
    for name in ("ep_steps", "episode", "arcade"):
        setattr(ring, name, FakeCuda(getattr(ring, name).numel()))
    family, tail, done = ops._arcade_args(ring, (FakeCuda(24), 2, ops.ARCADE_SELFPLAY))
    assert family == "_selfplay" and len(tail) == 5 and tail[1] == 2 and done == ()
    assert ops._arcade_args(ring, (FakeCuda(24), 2))[0] == "" and ops._arcade_args(ring, (FakeCuda(48), 2, 2))[0] == "_mix"
    with pytest.raises(ValueError):
        ops._arcade_args(ring, (FakeCuda(24), 2, "pairs"))
    with pytest.raises(ValueError, match="arcade config"):      # one whole block
        ops._arcade_args(ring, (FakeCuda(23), 0, ops.ARCADE_SELFPLAY))


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

    def call(name, B=4, tail=None, head=None, store=dev):
        tail = [dev, 0, dev, dev, dev] if tail is None else tail       # cfg, actor_base, ep_steps, episode, records
        fin = [store] if name.endswith("_tl") else []
        return f[name](*(heads(B)[name] if head is None else head), *tail, *fin, None)

    for name in ENTRIES:
        for B in (1, 3, 5, 63):                                            # odd B
            assert call(name, B=B) == EINVAL, (name, B)
        for base in (1, 3, 65):                                            # odd actor_base
            assert call(name, tail=[dev, base, dev, dev, dev]) == EINVAL, (name, base)
        # what the plain entries refuse
        for tail in ([None, 0, dev, dev, dev], [dev + 2, 0, dev, dev, dev], [dev, -2, dev, dev, dev],
                     [dev, 0, None, dev, dev], [dev, 0, dev, None, dev], [dev, 0, dev, dev, None]):
            assert call(name, tail=tail) == EINVAL, (name, tail)
        assert call(name, head=[0] + heads(4)[name][1:]) == EINVAL, name
        assert call(name, head=[4, 1] + heads(4)[name][2:]) == EINVAL, name
    for name in ENTRIES[2:]:                                               # A != 4 in the rollout forms
        assert call(name, head=heads(4)[name][:-2] + [6, 0]) == EINVAL, name
    for name in ENTRIES[4:]:                                               # the _tl forms: a null or misaligned store
        for store in (None, dev + 8):
            assert call(name, store=store) == EINVAL, (name, store)


# ---- the host model ---------------------------------------------------------------------------------------------------------------
def test_mirror_is_an_involution():
    rs = np.random.RandomState(0)
    rec = rs.randint(-100, 100, (50, 16)).astype(np.int32)
    m = SM.mirror(rec)
    np.testing.assert_array_equal(SM.mirror(m), rec)
    assert (m != rec).any()
    np.testing.assert_array_equal(m[:, [1, 3, 5, 9, 14, 15]], rec[:, [1, 3, 5, 9, 14, 15]])
    np.testing.assert_array_equal(m[:, 2], 86 - rec[:, 2])
    np.testing.assert_array_equal(m[:, [0, 6, 4, 7, 8, 10, 11, 12, 13]],
                                  np.stack([rec[:, 6], rec[:, 0], -rec[:, 4], rec[:, 8], rec[:, 7], rec[:, 11], rec[:, 10],
                                            rec[:, 13], rec[:, 12]], 1))
    one = SM.mirror(rec[3])
    np.testing.assert_array_equal(one, m[3])


@pytest.mark.parametrize("kw", [dict(), dict(points=2, paddle_width=8, ball_speed=4, win_reward=7, lose_reward=-3,
                                             max_episode_steps=60)])       # (HostDuel is the one-tick model of §7l)
def test_a_seat_one_that_stands_still_is_the_scripted_duel_with_a_standing_opponent(kw):
    """opponent_speed = 0: the script never moves the top paddle.  With seat 1 on noop (and no active flag of its own) seat 0
    of game i is HostDuel(conf.scripted, g = 2 i) step by step."""
    conf = _sp(opponent_speed=0, **kw)
    n_games, steps = 6, 250
    rs = np.random.RandomState(5)
    seats = [SM.HostSeat(conf, 2 * i, seed=9) for i in range(n_games)]              # partner=None: noop
    duels = [DM.HostDuel(conf.scripted, 2 * i, seed=9) for i in range(n_games)]
    ends = set()
    for s in range(steps):
        acts, active = rs.randint(0, 4, n_games), rs.rand(n_games) < 0.9
        for i in range(n_games):
            if not active[i]:
                continue
            got, want = seats[i].process(acts[i]), duels[i].process(acts[i])
            assert got[1:3] == want[1:3], (s, i)
            np.testing.assert_array_equal(got[3], want[3])
            np.testing.assert_array_equal(seats[i].frame, duels[i].frame)
            np.testing.assert_array_equal(seats[i].record()[:13], duels[i].record()[:13])
            assert (seats[i].ep_steps, seats[i].episode, seats[i].success) == (duels[i].ep_steps, duels[i].episode, duels[i].success)
            if want[2]:
                ends |= {e for e in duels[i].events if e.startswith("end_")}
                seats[i].reset(); duels[i].reset()
                np.testing.assert_array_equal(seats[i].frame, duels[i].frame)
    assert not kw or len(ends) >= 2, ends


def _run(conf, acts, active, frames_pairs=0, check=None):
    """The model over a trace -> the events seen and the canonical `by` values in flight."""
    B = acts.shape[1]
    seats = [SM.HostSeat(conf, b, SM.TRACE_SEED, frames=b < 2 * frames_pairs) for b in range(B)]
    seen, bys = set(), set()
    for s in range(acts.shape[0]):
        out = SM.step_pairs(seats, acts[s], active[s])
        for i in range(0, B, 2):
            if not out[i][3]:
                continue
            seen |= seats[i].events
            rec = seats[i].record()
            if rec[5] < 0:
                bys.add(int(rec[2]))
            if check is not None:
                check(s, seats[i], seats[i + 1], out[i], out[i + 1])
            assert out[i][1] == out[i + 1][1]                         # one terminal
            if out[i][1]:
                seats[i].reset(); seats[i + 1].reset()
    return seen, bys


def test_the_seats_rewards_sum_to_zero_in_a_zero_sum_setting():
    conf = _sp(points=2, ball_speed=4, win_reward=5, lose_reward=-5, return_reward=0, max_episode_steps=80, action_repeat=2)
    acts, active = SM.trace_inputs(1)
    rewards = set()

    def check(s, s0, s1, o0, o1):
        assert o0[0] + o1[0] == 0, s
        rewards.add(o0[0])
    _run(conf, acts[:200, :16], active[:200, :16], check=check)
    assert {5, -5, 0} <= rewards


def test_the_records_stay_mirror_images_and_seat_one_sees_the_mirrored_game():
    conf = _sp(**SM.TRACE_SETTINGS[1])
    acts, active = SM.trace_inputs(1)
    n = [0]

    def check(s, s0, s1, o0, o1):
        np.testing.assert_array_equal(s1.record(), SM.mirror(s0.record()))
        np.testing.assert_array_equal(s1.frame, SM.render_record(conf, SM.mirror(s0.record())))
        np.testing.assert_array_equal(s0.frame, SM.render_record(conf, s0.record()))
        # the paddles' and the ball's rows are exact images under y -> 87 - y, left and right stay
        np.testing.assert_array_equal((s1.frame[78:80] == DM.PADDLE).all(2), (s0.frame[8:10] == DM.OPPONENT).all(2)[::-1])
        np.testing.assert_array_equal((s1.frame[8:10] == DM.OPPONENT).all(2), (s0.frame[78:80] == DM.PADDLE).all(2)[::-1])
        n[0] += 1
    _run(conf, acts[:150, :8], active[:150, :8], frames_pairs=4, check=check)
    assert n[0] > 400


def test_the_traces_hold_every_event():
    """Both walls, all four return segments of each paddle, points both ways, a serve by either seat's fire and by
    serve_wait, a match ended by either seat and by the step limit: in the union of the four traces, so a GPU trace that
    never reached one cannot pass silently; the canonical by covers 6..82."""
    seen, bys = set(), set()
    per_trace = []
    for k, kw in enumerate(SM.TRACE_SETTINGS):
        acts, active = SM.trace_inputs(k)
        ev, by = _run(_sp(**kw), acts, active)
        per_trace.append(ev)
        seen |= ev
        bys |= by
    assert seen >= SM.EVERY_EVENT, SM.EVERY_EVENT - seen
    assert per_trace[1] >= SM.EVERY_EVENT, SM.EVERY_EVENT - per_trace[1]
    assert bys == set(range(6, 83)), set(range(6, 83)) ^ bys
