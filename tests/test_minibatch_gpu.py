"""Minibatched reuse epochs on the device: unreal_minibatch_gather against numpy slicing (bit for bit); the
trainer with the option off, the mean of a rollout's block gradients against the whole-rollout reuse gradient at unchanged
weights, every minibatch update rebuilt in fp64 from the twin's compact buffers, and one full-UNREAL run with the option on.
The bars are tests/test_reuse_gpu.py's."""
import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch

try:
    import margins
    import maze_model as MM
    import test_reuse_gpu as RG
    import timelimit_cases as TC
except ImportError:            # imported as tests.<module>
    from tests import margins
    from tests import maze_model as MM
    from tests import test_reuse_gpu as RG
    from tests import timelimit_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_I, SENT_F = -77, 9.25             # what the destinations hold before the launch


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(1, 1, 0), (3, 1, 2), (8, 2, 0), (8, 2, 6), (257, 1, 256), (260, 65, 130)]       # (Bg, Bm, j0)


@pytest.mark.parametrize("A", [3, 4, 18])
@pytest.mark.parametrize("Bg,Bm,j0", GEOMETRIES)
@pytest.mark.parametrize("T", [1, 5])
def test_gather_is_numpy_slicing_bit_for_bit(T, Bg, Bm, j0, A):
    """Every stream of the launch against src.reshape(T, Bg, ...)[:, j0:j0 + Bm]; destinations three rows (two actors)
    longer than the block and filled with a sentinel, which everything the launch must not write keeps.  (260, 65, 130) at
    T = 5 is 325 rows: more than one 256-thread block in every segment."""
    from unreal_amd import ops
    rs = np.random.RandomState(1000 * T + 10 * Bg + A)
    src_rows, rows, pad = T * Bg, T * Bm, 3
    ints = [rs.randint(-2 ** 31, 2 ** 31 - 1, src_rows).astype(np.int32) for _ in range(3)]      # frame_idx, actions, active
    flts = [rs.randint(0, 2 ** 32, src_rows * w, dtype=np.uint64).astype(np.uint32) for w in (1, 1, A)]    # adv, R, pi: any bits
    c0, h0 = (rs.randint(0, 2 ** 32, Bg * 256, dtype=np.uint64).astype(np.uint32) for _ in range(2))

    def take(a, w):                                               # the block's rows of a [T * Bg, w] stream
        return a.reshape(T, Bg, w)[:, j0:j0 + Bm].reshape(-1)

    for obj in (0, 3):
        side = A + 1 + obj
        for extra in (0, 1):
            xld = 256 + side + extra
            xcat = rs.randint(0, 2 ** 32, src_rows * xld, dtype=np.uint64).astype(np.uint32)
            for lstm in (True, False):
                d_int = [torch.full((rows + pad,), SENT_I, dtype=torch.int32, device=DEV) for _ in range(3)]
                d_flt = [torch.full(((rows + pad) * w,), SENT_F, dtype=torch.float32, device=DEV) for w in (1, 1, A)]
                s_int = [_dev(a, torch.int32) for a in ints]
                s_flt = [_dev(a.view(np.float32), torch.float32) for a in flts]
                kw = {}
                if lstm:
                    x_out = torch.full(((rows + pad) * xld,), SENT_F, dtype=torch.float32, device=DEV)
                    c_out, h_out = (torch.full(((Bm + 2) * 256,), SENT_F, dtype=torch.float32, device=DEV) for _ in range(2))
                    kw = dict(side=side, xcat=_dev(xcat.view(np.float32), torch.float32), xcat_out=x_out,
                              c0=_dev(c0.view(np.float32), torch.float32), h0=_dev(h0.view(np.float32), torch.float32),
                              c0_out=c_out, h0_out=h_out)
                ops.minibatch_gather(T, Bg, Bm, j0, A, s_int[0], s_int[1], s_int[2], s_flt[0], s_flt[1], s_flt[2], d_int[0],
                                     d_int[1], d_int[2], d_flt[0], d_flt[1], d_flt[2], ld=xld, **kw)
                what = "T=%d Bg=%d Bm=%d j0=%d A=%d obj=%d xld=%d lstm=%s" % (T, Bg, Bm, j0, A, obj, xld, lstm)
                for a, got in zip(ints, d_int):
                    want = np.full(rows + pad, SENT_I, np.int32)
                    want[:rows] = take(a, 1)
                    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=what)
                for a, got, w in zip(flts, d_flt, (1, 1, A)):
                    want = np.full((rows + pad) * w, SENT_F, np.float32).view(np.uint32)
                    want[:rows * w] = take(a, w)
                    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want, err_msg=what)
                for a, got in zip(s_int + s_flt, ints + flts):    # the sources are only read
                    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), got.view(np.uint32), err_msg=what)
                if lstm:
                    want = np.full((rows + pad, xld), SENT_F, np.float32).view(np.uint32)
                    want[:rows, 256:256 + side] = take(xcat, xld).reshape(rows, xld)[:, 256:256 + side]
                    np.testing.assert_array_equal(x_out.cpu().numpy().view(np.uint32).reshape(rows + pad, xld), want, err_msg=what)
                    for a, got in ((c0, c_out), (h0, h_out)):
                        want = np.full((Bm + 2) * 256, SENT_F, np.float32).view(np.uint32)
                        want[:Bm * 256] = a[j0 * 256:(j0 + Bm) * 256]
                        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want, err_msg=what)


# ---- 2-5. the trainer on a first-person maze -------------------------------------------------------------------------------------
ENV_NAME = "minibatch_gpu_fp7"
ADAM = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.01, clip_norm=40.0)
PRESENT_KEYS = ("total_loss", "base_loss", "policy_loss", "value_loss", "entropy", "pc_loss", "vr_loss", "rp_loss", "grad_norm")


@pytest.fixture
def fp7():
    """First-person N = 7 with a step limit of 3 (tests/test_reuse_gpu.py's configuration, under its own name): every actor
    ends inside a 5-step rollout, so rows past an episode's end exist."""
    from unreal_amd.environment.environment import Environment
    rs = np.random.RandomState(7)
    Environment.register_maze_config(ENV_NAME, [MM.random_layout(7, rs, marks="") for _ in range(2)], view="first_person",
                                     random_start=True, random_goal=True, max_episode_steps=3)
    yield Environment.MAZE_CONFIG[ENV_NAME]
    Environment.MAZE_CONFIG.pop(ENV_NAME, None)


def _build(Bn, T, Hn, lstm, aux=False, groups=1, depth=False, env=("maze", ENV_NAME), lr0=7.0711e-4, seed=21, adam=None,
           **options):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.adam_applier import AdamApplier
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    A = Environment.get_action_size(*env)
    net = UnrealModel(A, 0, -1, lstm, aux, aux, aux, 0.05, 0.001, DEV, seed=4, use_depth_prediction=depth)
    applier = AdamApplier(None, device=DEV, **adam) if adam is not None else \
        RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    if depth:
        options.update(use_depth_prediction=True, depth_lambda=0.7)
    tr = Trainer(0, net, lr0, None, applier, env[0], env[1], lstm, aux, aux, aux, 0.05, 0.001, T, T, 0.99, 0.9, Hn,
                 10 ** 6, DEV, batch_size=Bn, groups=groups, seed=seed, **options)
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    return net, applier, tr


def _hook_step(applier, before):
    """Wrap applier.step: `before(flat_grad)` runs on every update's gradient, the weights still those it was taken at."""
    inner = applier.step

    def step(flat_params, flat_grad, lr):
        before(flat_grad)
        return inner(flat_params, flat_grad, lr)
    applier.step = step


def test_option_off_is_todays_trainer(fp7):
    """reuse_minibatches=1 against no argument at all, one actor (the case in which two runs repeat bit for bit,
    tests/test_reuse_gpu.py): today's keys, no twin, no reuse buffer, the same bytes of device memory, and the same
    parameters bit for bit after three calls."""
    flats, keys, mem = [], [], []
    # (the first trainer only warms the process up: whatever the library caches on first use is allocated before the two
    # that are compared)
    for options in ({}, dict(reuse_minibatches=1), {}):
        gc.collect()
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        net, applier, tr = _build(1, 5, 16, True, **options)
        for it in range(3):
            steps, _ = tr.process(None, 0)
            assert steps > 0
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated() - m0)
        assert tr.reuse_minibatches == 1 and tr.mb is None
        assert not any(hasattr(tr, name) for name in RG.REUSE_BUFFERS)
        with pytest.raises(ValueError, match="reuse_minibatches"):
            tr.minibatch_gradients(0)
        flats.append(net.params.flat.cpu().numpy().copy())
        keys.append(sorted(tr.last_losses))
        del net, applier, tr
    assert keys[1] == keys[2] == sorted(PRESENT_KEYS)
    assert mem[1] == mem[2], mem
    np.testing.assert_array_equal(flats[1].view(np.uint32), flats[2].view(np.uint32))


@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("lstm", [True, False])
def test_block_gradients_average_to_the_whole_rollouts(fp7, lstm, M):
    """Learning rate 0, auxiliary heads off, 4 actors in one group.  Trainer A (reuse_epochs 2, M = 1): its update 2 is the
    reuse gradient of the whole rollout.  Trainer B (reuse_epochs 1, M blocks): the same rollout -- same seed, weights that
    never move -- consumed as M updates of 4 / M actors at grad_scale M / 4, so the mean of its M gradients is A's, and each
    block's re-evaluated heads are the rollout's rows (forward bar, not bit for bit: a block's fp16x2 scales are its own)."""
    T, Bg, A_ = 5, 4, 4
    Bm = Bg // M
    netA, applierA, trA = _build(Bg, T, 50, lstm, lr0=0.0, reuse_epochs=2)
    netB, applierB, trB = _build(Bg, T, 50, lstm, lr0=0.0, reuse_epochs=1, reuse_minibatches=M)
    startA, startB = netA.params.flat.clone(), netB.params.flat.clone()
    assert torch.equal(startA, startB)
    gradsA, gradsB, heads = [], [], []
    _hook_step(applierA, lambda g: gradsA.append(g.clone()))
    _hook_step(applierB, lambda g: (gradsB.append(g.clone()),
                                    heads.append((trB.mb.block, trB.mb.pi_new.clone(), trB.mb.v_new.clone()))))
    for call in range(2):
        del gradsA[:], gradsB[:], heads[:]
        sA, _ = trA.process(None, 0)
        sB, _ = trB.process(None, 0)
        assert len(gradsA) == 2 and len(gradsB) == M and sA == sB > 0
        assert torch.equal(trA.actions, trB.actions) and torch.equal(trA.active_log, trB.active_log)   # the same rollout
        assert [h[0] for h in heads] == list(range(M))
        want = netA.grads.make_views(gradsA[1])
        mean = netB.grads.make_views(torch.stack(gradsB).double().mean(0).float())
        for name, _, _ in netA.spec:
            w = want[name].cpu().numpy().astype(np.float64)
            g = mean[name].cpu().numpy().astype(np.float64)
            tol = RG.GRAD_REL * np.abs(w).max()
            err = np.abs(g - w).max()
            print("lstm=%s M=%d call %d g[%s]: max |d| %.3g, bar %.3g (%.3f of it)" % (lstm, M, call, name, err, tol, err / tol))
            margins.record("partition lstm=%s M=%d %s" % (lstm, M, name), err / tol, "2e-5 of the variable's largest")
            assert err <= tol, (name, err, tol)
        pi = trB.pi.cpu().numpy().astype(np.float64).reshape(T, Bg, A_)
        v = trB.v.cpu().numpy().astype(np.float64).reshape(T, Bg)
        for m, pi_new, v_new in heads:
            p_blk, v_blk = pi[:, m * Bm:(m + 1) * Bm].reshape(-1), v[:, m * Bm:(m + 1) * Bm].reshape(-1)
            got_p, got_v = pi_new.cpu().numpy().astype(np.float64), v_new.cpu().numpy().astype(np.float64)
            r = max(margins.record_close("partition pi_new lstm=%s M=%d" % (lstm, M), got_p, p_blk, RG.FWD_ATOL, RG.FWD_RTOL),
                    margins.record_close("partition v_new lstm=%s M=%d" % (lstm, M), got_v, v_blk, RG.FWD_ATOL, RG.FWD_RTOL))
            print("lstm=%s M=%d call %d block %d: heads at %.3f of the forward bar" % (lstm, M, call, m, r))
            assert r <= 1.0
        on = int(trB.active_log.sum())
        assert 0 < on < T * Bg                                    # rows past an episode's end were masked out
        assert trB.reuse_stats_i.cpu().numpy().tolist() == [0, 1 * on]      # E * (active rows), none clipped
        l = trB.last_losses
        assert l["clip_fraction"] == 0.0 and l["updates"] == M
        assert torch.equal(netA.params.flat, startA) and torch.equal(netB.params.flat, startB)


# ppo_clip, learning rate and trainer seed per case, found by search on the device (as tests/test_reuse_gpu.py's) so that the
# fp64 rebuild of at least one update after a group's first has clipped AND unclipped active rows and no row of any update is
# within RG.EDGE of a clip edge (both asserted below)
COMBINED = dict(bootstrap_timeouts=True, gae_lambda=0.9, normalize_advantages=True)
CASES = [
    # lstm, groups, depth, options, (ppo_clip, lr0, seed)
    (True, 1, False, {}, (0.01, 0.1, 21)),
    (False, 1, False, {}, (0.02, 0.1, 23)),
    (True, 2, False, {}, (0.02, 0.1, 23)),
    (False, 2, False, {}, (0.02, 0.1, 23)),
    (True, 2, True, COMBINED, (0.02, 0.05, 21)),
]


def run_case(lstm, groups, depth, options, picked, check=True):
    """One process() call with reuse_epochs = 2 and reuse_minibatches = 2 (4 actors in one group, 8 in two); every one of
    its G * 4 updates is rebuilt in fp64 from the twin's compact buffers, at the weights it was taken at -> records."""
    from unreal_amd.train.trainer import Trainer
    ppo_clip, lr0, seed = picked
    Bn, T, E, M = 4 * groups, 5, 2, 2
    net, applier, tr = _build(Bn, T, 50, lstm, groups=groups, depth=depth, lr0=lr0, seed=seed, reuse_epochs=E,
                              reuse_minibatches=M, ppo_clip=ppo_clip, **options)
    depth_lam = 0.7 if depth else 0.0
    Bg, Bm, A = tr.Bg, tr.mb.Bg, tr.action_size
    records, prev = [], [0, 0]

    def rebuild(flat_grad):
        mb, m = tr.mb, tr.mb.block
        k = len(records)
        # the compact buffers are the block's rows of the rollout, bit for bit (the advantages: the normalised ones if on)
        adv_src = tr.adv_norm if tr.normalize_advantages else tr.adv
        for got, src, w in ((mb.actions, tr.actions, 1), (mb.active_log, tr.active_log, 1), (mb.adv, adv_src, 1),
                            (mb.R, tr.R, 1), (mb.pi, tr.pi, A), (mb.base_ws.frame_idx, tr.base_ws.frame_idx, 1)):
            assert torch.equal(got[:T * Bm * w], src[:T * Bg * w].view(T, Bg, w)[:, m * Bm:(m + 1) * Bm].reshape(-1))
        shim = SimpleNamespace(Bg=Bm, base_ws=mb.base_ws, ring=mb.base_ring, actions=mb.actions, adv=mb.adv, R=mb.R,
                               active_log=mb.active_log, pi=mb.pi, ppo_clip=tr.ppo_clip)
        want_l, want_g, info = RG._rebuild(net, shim, T, lstm, True, depth_lam)
        got_l = tr.losses.cpu().numpy()[:3].astype(np.float64)
        stats = tr.reuse_stats_i.cpu().numpy().tolist()
        rec = dict(g=tr.group, k=k % (E * M), block=m, counted=info["counted"], ended=int((~info["on"]).sum()),
                   clipped=info["clipped"], edge=RG.PM.edge_distance(info["rho"], ppo_clip) if info["counted"] else 1.0,
                   stats=[stats[0] - prev[0], stats[1] - prev[1]])
        prev[:] = stats
        rec["loss_ratio"] = float((np.abs(got_l - want_l) / (RG.LOSS_RTOL * np.abs(want_l))).max()) if info["counted"] else 0.0
        views = net.grads.make_views(flat_grad)
        ratios = {}
        for name, gw in want_g.items():
            gd = views[name].cpu().numpy().astype(np.float64).reshape(gw.shape)
            ratios[name] = float(np.abs(gd - gw).max() / (RG.GRAD_REL * np.abs(gw).max())) if np.abs(gw).max() > 0 else \
                float(np.abs(gd).max() > 0)
        rec["grad_ratio"] = max(ratios.values())
        rec["grad_worst"] = max(ratios, key=ratios.get)
        print("lstm=%s groups=%d depth=%s %s: %s" % (lstm, groups, depth, sorted(options), rec))
        margins.record("minibatch rebuild lstm=%s G=%d depth=%s g=%d k=%d" % (lstm, groups, depth, rec["g"], rec["k"]),
                       max(rec["loss_ratio"], rec["grad_ratio"]), "losses rel 1e-4, gradients 2e-5 of the variable's largest")
        if check:
            assert rec["loss_ratio"] <= 1.0, (rec, got_l, want_l)
            assert rec["grad_ratio"] <= 1.0, rec
            assert rec["edge"] > RG.EDGE, rec                     # asserted, not skipped
            assert rec["stats"] == [info["clipped"], info["counted"]], rec          # clip_fraction is exact
        records.append(rec)

    _hook_step(applier, rebuild)
    tr.reuse_stats_i.zero_()
    steps, _ = tr.process(None, 0)
    assert steps > 0 and len(records) == groups * E * M
    order = [m for e in range(1, E + 1) for m in Trainer.minibatch_order(e, M)]
    for g in range(groups):
        assert [r["block"] for r in records if r["g"] == g] == order
    if check:
        l = tr.last_losses
        assert l["updates"] == groups * E * M
        n = sum(r["counted"] for r in records)
        assert n == E * steps and l["clip_fraction"] == sum(r["clipped"] for r in records) / float(n)
    return records


@pytest.mark.parametrize("lstm,groups,depth,options,picked", CASES)
def test_minibatch_updates_against_fp64(fp7, lstm, groups, depth, options, picked):
    """reuse_epochs = 2, reuse_minibatches = 2, T = 5, history 50, the other auxiliary heads off; the last case has time-limit
    bootstrapping, GAE(0.9), the depth head and advantage normalisation on together.  Measured with the picks above: the
    closest row is 2.5e-3 from a clip edge, 2 to 5 updates per case mix clipped and unclipped rows, and the worst error is
    0.07 of its bar; two runs of a case gave the same figures to four digits."""
    records = run_case(lstm, groups, depth, options, picked)
    assert sum(r["ended"] for r in records) > 0                  # rows past an episode's end were masked out
    assert any(r["k"] > 0 and 0 < r["clipped"] < r["counted"] for r in records), records


# ---- 6. full UNREAL ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_type", ["maze", "arcade"])
def test_full_unreal_with_minibatches(env_type):
    """reuse_epochs = 2, reuse_minibatches = 2, groups = 2 on 8 actors with Adam, the exploration bonus and GAE(0.95), LSTM +
    pixel control + value replay + reward prediction, on a first-person maze and on Breakout."""
    from unreal_amd.environment.environment import Environment
    name = "minibatch_full_" + env_type
    if env_type == "arcade":
        Environment.register_arcade_config(name, **dict(TC.BREAKOUT, max_episode_steps=9))
    else:
        rs = np.random.RandomState(7)
        Environment.register_maze_config(name, [MM.random_layout(7, rs, marks="")], view="first_person", random_start=True,
                                         random_goal=True, max_episode_steps=3)
    try:
        G, E, M, Bn, T = 2, 2, 2, 8, 5
        net, applier, tr = _build(Bn, T, 50, True, aux=True, groups=G, env=(env_type, name), adam=ADAM, reuse_epochs=E,
                                  reuse_minibatches=M, explore_beta=0.0625, gae_lambda=0.95)
        Bg, Bm = Bn // G, Bn // G // M
        rolled, drawn = [], []
        inner = tr.compute_gradients

        def counting():
            inner()
            rolled.append(int(tr.active_log.sum()))
        tr.compute_gradients = counting
        for fn in ("uniform", "randint"):                         # every draw: (actors served, first column, elements drawn)
            def wrap(f=getattr(tr.draws, fn)):
                def call(*a):
                    drawn.append((tr.draws.batch, tr.draws.col0, a[-1].numel()))
                    return f(*a)
                return call
            setattr(tr.draws, fn, wrap())
        # one auxiliary set: the pixel-control and value-replay sequence starts, the reward-prediction coin and its uniform
        AUX = 4
        for call in range(3):
            del rolled[:], drawn[:]
            c0 = tr.draws.counter
            steps, _ = tr.process(None, call * 40)
            assert len(rolled) == G and steps == sum(rolled) and 0 < steps <= Bn * T, (steps, rolled)
            assert tr.draws.counter - c0 == G * (1 + E * M * AUX) == len(drawn)
            per_group = 1 + E * M * AUX
            for g in range(G):
                d = drawn[g * per_group:(g + 1) * per_group]
                assert d[0] == (Bg, g * Bg, T * Bg)               # the rollout's action draws: the group's actors
                blocks = [m for e in range(1, E + 1) for m in tr.minibatch_order(e, M)]
                for k, m in enumerate(blocks):                    # then E * M auxiliary sets at Bm actors, at the block's columns
                    assert d[1 + k * AUX:1 + (k + 1) * AUX] == [(Bm, g * Bg + m * Bm, Bm)] * AUX, (g, k, d)
            assert (tr.draws.batch, tr.draws.col0) == (Bg, 0)
            l = tr.last_losses
            assert all(np.isfinite(v) for v in l.values()), l
            assert all(k in l for k in PRESENT_KEYS + RG.REUSE_KEYS + ("updates", "explore_bonus")), l
            assert l["updates"] == 8 and applier.t == (call + 1) * 8
            assert l["policy_loss"] == l["reuse_policy_loss"] and l["value_loss"] == l["reuse_value_loss"]
            assert l["entropy"] == l["reuse_entropy"] > 0.0 and l["pc_loss"] > 0.0 and l["vr_loss"] > 0.0
            si = tr.reuse_stats_i.cpu().numpy()
            assert si[1] == E * steps and 0.0 <= l["clip_fraction"] == float(si[0]) / si[1] <= 1.0 and l["approx_kl"] >= 0.0
        assert bool(torch.isfinite(net.params.flat).all()) and bool(torch.isfinite(applier.m).all())
        assert bool(torch.isfinite(applier.v).all()) and float(applier.v.min()) >= 0.0
    finally:
        (Environment.ARCADE_CONFIG if env_type == "arcade" else Environment.MAZE_CONFIG).pop(name, None)
