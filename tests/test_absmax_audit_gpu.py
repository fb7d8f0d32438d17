"""The absmax slot of every fp16-split operand, audited through whole training passes (GPU).

include/unreal_hip.h: "the slot handed to a GEMM must cover every element the GEMM reads".  The kernel tests reduce the
slot from the operand itself; here tests/absmax_audit.py intercepts every launch of Trainer.process() (and of the batch-1
runners and Evaluate) and compares the slot the HOST handed over with the operand's true maximum, reduced on the same
stream right before the launch (read slots) or right after it (committed slots).  Both checks are plain inequalities.

Each configuration runs the replay fill and two process() calls under the audit, then multiplies every parameter by
GROW in place and audits one more process(): a slot that is not reduced in the current pass (shadow wmax, workspace-owned
slots, net._one, ops._SCRATCH live outside the per-pass pool) then no longer covers.  The weight shadows' slots are
audited against the live fp32 weights (AbsmaxAudit.watch).

The over-cover of every read pair (binades the slot lies above the operand's maximum: bits of the 22 the split loses) is
written to absmax_audit.json (absmax_audit.REPORT: $ABSMAX_AUDIT_DIR, else runs/); no cap is asserted (profiles/absmax_audit.md holds the measured baseline)."""
import time

import numpy as np
import pytest
import torch

from tests import absmax_audit as AA
from tests import maze_model as MM
from tests import timelimit_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROW = 4.0
B, H, T = 4, 24, 5


# ---- 1. planted control ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def control():
    from unreal_amd import ops
    g = torch.Generator().manual_seed(3)
    A = torch.randn(64 * 64, generator=g).to(DEV)
    Wsrc = torch.randn(64 * 64, generator=g).to(DEV)
    W = ops.SplitWeights(Wsrc, 64, 64, 64, False)
    return ops, A, W, float(A.abs().max())


def _control_launch(control, slot):
    ops, A, W, _ = control
    C = torch.zeros(64 * 64, device=DEV)
    with AA.AbsmaxAudit("control", n_pairs=16) as audit:
        ops.gemm_split_nt(64, 64, 64, A, 64, W, C, 64, a_max=slot)
    assert ops._call.__name__ == "_call" and audit.launches >= 1         # restored
    return audit


def test_planted_half_slot_is_reported_as_under_covered(control):
    """a_max holds half the operand's true maximum (wrong numerics on a private buffer, no memory fault): exactly that
    pair is reported, with the entry, the operand, both values and one binade of gap."""
    true = control[3]
    audit = _control_launch(control, torch.tensor([true / 2], device=DEV))
    bad = audit.violations()
    assert [(p["entry"], p["operand"], p["kind"]) for p in bad] == [("unreal_gemm_f32_split_nt", "A", "read")]
    assert bad[0]["true"] == true and bad[0]["claimed"] == float(np.float32(true / 2))
    assert len(audit.pairs) == 1                                         # no c_max: no committed pair
    with pytest.raises(AssertionError) as e:
        audit.assert_clean()
    msg = str(e.value)
    assert "unreal_gemm_f32_split_nt A" in msg and "1 binade(s) short" in msg and "ops.py" in msg and "gemm_split_nt" in msg


def test_planted_256x_slot_is_eight_binades_of_over_cover(control):
    true = control[3]
    audit = _control_launch(control, torch.tensor([256.0 * true], device=DEV))
    audit.assert_clean()
    assert audit.overcover()[("unreal_gemm_f32_split_nt", "A")]["binades"] == 8


def test_slot_reduced_by_the_wrapper_covers_exactly(control):
    """a_max=None: ops.gemm_split_nt reduces the slot itself (ops._SCRATCH) -- the same value, 0 binades."""
    audit = _control_launch(control, None)
    audit.assert_clean()
    row = audit.overcover()[("unreal_gemm_f32_split_nt", "A")]
    assert row["binades"] == 0 and row["claimed"] == row["true"] == control[3]


def test_committed_slot_is_audited_after_the_launch(control):
    """c_max: the slot the launch commits to holds max |C| afterwards; a read pair and a committed pair are recorded."""
    ops, A, W, true = control
    C = torch.zeros(64 * 64, device=DEV)
    c_max = torch.zeros(1, device=DEV)
    with AA.AbsmaxAudit("control", n_pairs=16) as audit:
        ops.gemm_split_nt(64, 64, 64, A, 64, W, C, 64, c_max=c_max)
    audit.assert_clean()
    kinds = {p["kind"]: p for p in audit.pairs}
    assert sorted(kinds) == ["committed", "read"]
    assert kinds["committed"]["true"] == float(C.abs().max()) == kinds["committed"]["claimed"] > 0


# ---- 2. pass audit ---------------------------------------------------------------------------------------------------------
def _maze(monkeypatch, use_lstm=True, groups=1, B=B, patch=None, aux=True, seed=5):
    from tests.test_trainer_gpu import _build, _cfg
    from unreal_amd.train.trainer import Trainer
    for k, v in (patch or {}).items():
        monkeypatch.setattr(Trainer, k, v)
    net, applier, tr, draws = _build(_cfg(use_lstm, aux, H, T), B, seed=seed, groups=groups)
    return net, tr


def _maze_lstm(mp):
    return _maze(mp)


def _maze_groups2(mp):
    net, tr = _maze(mp, groups=2, B=8)
    assert tr.Bg == 4
    return net, tr


def _maze_ff(mp):
    return _maze(mp, use_lstm=False)


def _lab_overlap(mp):
    from tests.test_trainer_gpu import _build, _cfg
    from unreal_amd.environment.synthetic_sim import SyntheticBatchSimulator
    cfg = _cfg(True, True, H, T)
    cfg.update(action_size=6)
    sim = SyntheticBatchSimulator(B, seed=4, episode_len=7, reward_p=0.3, big_reward_p=0.1)
    net, applier, tr, draws = _build(cfg, B, seed=9, env_type="lab", simulator=sim, frame_scale=1.0 / 255.0, overlap_host=True)
    assert tr.overlap_host
    return net, tr


class LoudIndoor(object):
    """SyntheticBatchIndoorSimulator with the objective entries scaled to +-50 and the rewards to +-8 after the wrapper's
    division by termination_time (the simulator's own are within 1 and 0.5): the columns of the LSTM input beyond the
    kernel's floor of 1."""
    OBJ_GAIN, REWARD_GAIN = 50.0, 16.0

    def __init__(self, inner):
        self.inner, self.B, self.objective_size, self.image_shape = inner, inner.B, inner.objective_size, inner.image_shape

    def reset(self, mask=None):
        frames, obj = self.inner.reset(mask)
        return frames, obj * np.float32(self.OBJ_GAIN)

    def step(self, actions, active=None):
        frames, rewards, terminals, obj = self.inner.step(actions, active)
        return frames, rewards * np.float32(self.REWARD_GAIN), terminals, obj * np.float32(self.OBJ_GAIN)


def _indoor_objective(mp):
    from tests.test_trainer_gpu import _build, _cfg
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.synthetic_sim import SyntheticBatchIndoorSimulator
    OBJ = 5
    cfg = _cfg(True, True, H, T)
    cfg.update(action_size=3, objective_size=OBJ)
    Environment.register_indoor_config("synthetic_rooms", OBJ)
    sim = LoudIndoor(SyntheticBatchIndoorSimulator(B, seed=5, episode_len=7, reward_p=0.2, big_reward_p=0.15,
                                                   objective_size=OBJ, termination_time=50.0))
    net, applier, tr, draws = _build(cfg, B, seed=11, env_type="indoor", env_name="synthetic_rooms", simulator=sim,
                                     frame_scale=1.0 / 255.0, overlap_host=True)
    assert not net.lar_bounded and net.K_x == 256 + 3 + 1 + OBJ
    return net, tr, lambda truncated: _loud_enough(tr)


def _loud_enough(tr):
    """The magnitudes the configuration is there for did reach the ring."""
    assert 40.0 < float(tr.ring.r_objective.abs().max()) <= 50.0
    assert float(tr.ring.r_reward.abs().max()) == 8.0


def _indoor_120x160(mp):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.synthetic_sim import SyntheticBatchIndoorSimulator
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    shape, OBJ = (120, 160), 5
    name = "rooms_%dx%d" % shape
    Environment.register_indoor_config(name, OBJ, height=shape[0], width=shape[1])
    sim = SyntheticBatchIndoorSimulator(B, seed=5, height=shape[0], width=shape[1], episode_len=7, reward_p=0.2,
                                        big_reward_p=0.1, objective_size=OBJ, termination_time=50.0)
    Environment.action_size = -1
    A = Environment.get_action_size("indoor", name)
    net = UnrealModel(A, OBJ, -1, True, False, True, True, 0.05, 0.001, DEV, image_shape=shape, seed=12, frame_scale=1.0 / 255.0)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    tr = Trainer(0, net, 7.0711e-4, None, applier, "indoor", name, True, False, True, True, 0.05, 0.001, T, T, 0.99, 0.9,
                 H, 10 ** 6, DEV, batch_size=B, simulator=sim, overlap_host=False, image_shape=shape)
    tr.prepare()
    assert net.hw
    return net, tr


def _gym_a18(mp):
    from tests.test_trainer_gpu import _build, _cfg
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.gym_environment import synthetic_atari_batch
    A = 18
    name = "SyntheticAtari%d-v0" % A
    Environment.register_gym_config(name, A)
    cfg = _cfg(True, True, H, T)
    cfg.update(action_size=A)
    sim = synthetic_atari_batch(B, action_size=A, seed=6, episode_len=7)
    net, applier, tr, draws = _build(cfg, B, seed=13, env_type="gym", env_name=name, simulator=sim, frame_scale=1.0 / 255.0,
                                     overlap_host=True)
    assert net.K_x == 256 + A + 1
    return net, tr


def _breakout_reuse(mp):
    from tests.test_optim_gpu import _build, ADAM
    from unreal_amd.environment.environment import Environment
    name = "audit_breakout"
    Environment.register_arcade_config(name, **dict(TC.BREAKOUT, max_episode_steps=9))
    net, applier, tr = _build(B, T, H, True, aux=True, env=("arcade", name), adam=ADAM, fill=False, reuse_epochs=2,
                              reuse_minibatches=2, normalize_advantages=True)
    tr.prepare()
    assert tr.mb is not None and tr.reuse_epochs == 2
    return net, tr


def _fp7(name, **kw):
    from unreal_amd.environment.environment import Environment
    rs = np.random.RandomState(7)
    Environment.register_maze_config(name, [MM.random_layout(7, rs, marks="") for _ in range(2)], view="first_person",
                                     random_start=True, random_goal=True, max_episode_steps=3, **kw)


def _fp_depth(mp):
    from tests import test_depth_gpu as DG
    _fp7(DG.ENV_NAME)
    net, applier, tr = DG._trainer(B, T, H, True, True)          # (fills the replay: inside the audit too)
    assert tr.use_depth_prediction
    return net, tr


def _timelimit_gae(mp):
    from tests.test_optim_gpu import _build
    name = "audit_fp7_tl"
    _fp7(name)
    net, applier, tr = _build(B, T, H, True, aux=True, env=("maze", name), fill=False, bootstrap_timeouts=True,
                              gae_lambda=0.95)
    tr.prepare()
    assert tr.full_ring.final_obs is not None
    return net, tr, _saw_truncation


def _saw_truncation(truncated):
    """A rollout was cut off at the step limit: its bootstrap rows were encoded from the final-observation store."""
    assert truncated


def _versus_pool(mp):
    from tests.test_versus_gpu import _register, _build_pool, SHORT
    name = "audit_versus"
    _register(name, **SHORT)
    net, applier, tr = _build_pool(name, B, T, H, opponent_pool=2, opponent_snapshot_every=100)
    assert tr.opponent_pool == 2
    return net, tr


def _half_batch(mp):
    net, tr = _maze(mp, patch=dict(rollout_parts_default=2, ROLLOUT_SPLIT_MIN_ACTORS=2))
    assert tr._split is not None
    return net, tr


def _fused_encoder(mp):
    """(the step kernel takes any actor count: tests/test_rollout_fused_gpu.py runs it at 17)"""
    return _maze(mp, patch=dict(FUSE_ENV_ENCODER_MIN_ACTORS=2))


CONFIGS = [
    ("maze_lstm_aux", _maze_lstm), ("maze_lstm_aux_groups2", _maze_groups2), ("maze_ff_aux", _maze_ff),
    ("lab_overlap_host", _lab_overlap), ("indoor_objective_loud", _indoor_objective),
    ("indoor_120x160", _indoor_120x160), ("gym_a18", _gym_a18), ("breakout_reuse_minibatch_adam", _breakout_reuse),
    ("fp_maze_depth", _fp_depth), ("fp_maze_timelimit_gae", _timelimit_gae), ("duel_opponent_pool2", _versus_pool),
    ("maze_half_batch_streams", _half_batch), ("maze_fused_step_encoder", _fused_encoder),
]
# the entry each configuration is there to reach: it must have been audited
MUST_REACH = {
    "indoor_120x160": "unreal_encoder_hw_fwd", "maze_fused_step_encoder": "unreal_maze_policy_rollout_step_encode",
    "maze_lstm_aux": "unreal_pc_deconv_train", "maze_ff_aux": "unreal_pc_deconv_train",
    "gym_a18": "unreal_pc_deconv_train", "duel_opponent_pool2": "unreal_lstm_step_fwd",
}


def _zero_state(tr):
    """Every replay workspace the trainer holds (Trainer._replay_set: the path and the bootstrap workspace of each width)
    starts every replayed sequence from the zero LSTM state and trainer.py fills none of them: nothing may ever have
    written their c0 / h0 (bit for bit: -0.0 counts)."""
    n = 0
    for c in (tr, getattr(tr, "mb", None)):
        if c is None or not tr.use_lstm:
            continue
        for ws in [w for r in c.replay.values() for w in (r.boot_ws, r.ws)]:
            for name in ("c0", "h0"):
                t = getattr(ws, name)
                assert not bool(t.view(torch.int32).any()), "%s of a zero-state workspace was written" % name
                n += 1
    return n


def _finish(config, audits, t0, extra=None):
    table = AA.merge_overcover(*[a.overcover() for a in audits])
    info = dict(seconds=round(time.time() - t0, 2), pairs=sum(len(a.pairs) for a in audits),
                launches=sum(a.launches for a in audits), violations=sum(len(a.violations()) for a in audits),
                grow=GROW)
    info.update(extra or {})
    try:
        AA.write_report(config, table, extra=info)
    except OSError:                      # a read-only tree: the figures are still printed
        pass
    print("absmax audit %s: %s" % (config, info))
    for (e, o), r in sorted(table.items(), key=lambda kv: -kv[1]["binades"])[:5]:
        print("  over-cover %2d binades  %s %s  (%.6g vs %.6g)  %s:%d" % (r["binades"], e, o, r["claimed"], r["true"],
                                                                        r["site"][0], r["site"][1]))


@pytest.mark.parametrize("config,build", CONFIGS, ids=[c for c, _ in CONFIGS])
def test_every_slot_of_a_training_pass_covers_its_operand(config, build, monkeypatch):
    t0 = time.time()
    steady = AA.AbsmaxAudit(config)
    with steady:
        out = build(monkeypatch)
        net, tr, check = out if len(out) == 3 else out + (None,)
        nets = [net] + [tr.opponent(k) for k in range(tr.opponent_pool)]
        steady.watch(*nets)
        while not tr._full:
            tr.process(None, 0)
        g = 0
        truncated = False
        for _ in range(2):
            steps, _ = tr.process(None, g)
            g += steps
            truncated = truncated or bool((tr.terminal_end == 2).any())
    assert np.isfinite(tr.last_losses["total_loss"])
    # growth: every parameter x GROW in place; what is not reduced again in this pass no longer covers
    net.params.flat.mul_(GROW)
    net.mark_params_changed()
    grown = AA.AbsmaxAudit(config + " x%g" % GROW).watch(*nets)
    with grown:
        tr.process(None, g)
    _finish(config, [steady, grown], t0)
    assert np.isfinite(tr.last_losses["total_loss"]), "x%g drove the loss non-finite" % GROW
    steady.assert_clean()
    grown.assert_clean()
    reached = {p["entry"] for p in steady.pairs}
    assert MUST_REACH.get(config, "unreal_gemm_f32_split_nt") in reached, sorted(reached)
    assert len(grown.pairs) > 20
    assert any(p["operand"] == "W" for p in grown.pairs)                 # the weight shadows were audited as well
    if check is not None:
        check(truncated)
    if tr.use_lstm and tr.replay_width:
        assert _zero_state(tr) >= 4
    tr.stop()


def test_a_column_the_host_leaves_out_of_the_slot_is_caught_through_the_trainer(monkeypatch):
    """Planted control on the host side: gym actors feed raw rewards (sums up to 12) into the LSTM input, and
    net.lar_bounded -- "those columns stay within the kernel's floor of 1" -- is set although they do not.  encode_rows
    then skips their reduction, and the audit must name the LSTM step's x operand at model.py's lstm_step, nothing else.
    (Wrong numerics in a trainer that is thrown away, not a memory fault.)"""
    net, tr = _gym_a18(monkeypatch)
    while not tr._full:
        tr.process(None, 0)
    assert float(tr.ring.r_last_reward.abs().max()) > 1.0
    net.lar_bounded = True
    with AA.AbsmaxAudit("planted lar_bounded") as audit:
        tr.process(None, 0)
    bad = audit.violations()
    assert bad and {(p["entry"], p["operand"], p["site"][0], p["site"][2]) for p in bad} == {
        ("unreal_lstm_step_fwd", "x", "unreal_amd/model/model.py", "lstm_step")}
    assert all(p["claimed"] == 1.0 < p["true"] for p in bad)             # the floor was claimed, a reward lay above it
    tr.stop()


def test_batch1_runners_and_evaluate_on_the_trainers_network(monkeypatch):
    """The batch-1 runners stage frames at 1 / 255 on the network the trainer reads at the maze's own scale, and Evaluate
    runs its own workspace on it: all of them between and after the trainer's passes, then again on grown weights."""
    from oracle import maze as OM
    from unreal_amd.evaluate import Evaluate
    config = "maze_batch1_runners_evaluate"
    t0 = time.time()
    env = OM.OracleMaze()
    hist = [{'image': OM.render(0, 2)}, {'image': OM.render(1, 2)}, {'image': OM.render(1, 3)}]

    def runners(net, lar):
        net.reset_state()
        out = [net.run_base_value(None, env.last_state, lar), net.run_base_policy_and_value(None, env.last_state, lar)[1],
               net.run_vr_value(None, env.last_state, lar)]
        out += list(net.run_pc_q_max(None, env.last_state, lar).reshape(-1)) + list(net.run_rp_c(None, hist).reshape(-1))
        assert np.isfinite(out).all()

    lar = np.zeros(5)
    lar[2], lar[4] = 1.0, 6.5                   # an arbitrary caller's reward: beyond the kernel's floor of 1
    audits = []
    net = tr = ev = None
    g = 0
    for label, grow in ((config, None), (config + " x%g" % GROW, GROW)):
        audit = AA.AbsmaxAudit(label)
        with audit:
            if net is None:
                net, tr = _maze(monkeypatch)
                audit.watch(net)
                while not tr._full:
                    tr.process(None, 0)
                ev = Evaluate(net, batch_size=B, device=DEV, seed=3)
            else:
                audit.watch(net)
                net.params.flat.mul_(grow)
                net.mark_params_changed()
            runners(net, lar)
            steps, _ = tr.process(None, g)
            g += steps
            runners(net, lar)
            res = ev.process(1, max_episode_steps=6)
            assert res["episodes"] >= 1
            steps, _ = tr.process(None, g)
            g += steps
        audits.append(audit)
        assert np.isfinite(tr.last_losses["total_loss"])
    _finish(config, audits, t0)
    for audit in audits:
        audit.assert_clean()
        sites = {p["site"][2] for p in audit.pairs}
        assert "encode_rows" in sites and "run_pc_q_max" in sites, sorted(sites)
    assert _zero_state(tr) >= 4
    tr.stop()
