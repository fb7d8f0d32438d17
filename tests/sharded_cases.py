"""Shards of a multi-rank job on one GPU in one process (tests/test_sharded_gpu.py): plain functions, no fixtures.

A rank > 0 is `Trainer(rank=r, world_size=W, batch_size=B)`; the other ranks are stood in for through the `grad_sync`
callable, and no process group exists (`parallel.all_true` then answers with the local flag).  Three harnesses:

* shard_against_oracle: the per-update loop of every test_process_on_*_matches_oracle (recorded device draws replayed into
  OracleTrainer, fp64) for a shard whose host models are those of the global actors [r B, (r + 1) B).  The device gradient
  is the rank's share, 1 / W of the mean over its own actors: W * g is compared, and the gradient buffer is multiplied by W
  before the step (a job whose other ranks sent the same gradient), so the weights follow the oracle's.
* run_job / compare_ranks_with_whole: W ranks one after the other against one process holding all W * B actors, every
  trainer on its own PhiloxDraws columns; each rank's exchange hands it the one-process gradient.
* run_scaled_pair: world_size = 2 with an exchange that doubles the gradient against world_size = 1 on the same actors.

Every tolerance is one the suite already asserts (tests/test_trainer_gpu.py, tests/test_distributed_gpu.py)."""
import numpy as np
import torch

try:
    import margins
    import test_trainer_gpu as TT
except ImportError:            # imported as tests.<module>
    from tests import margins
    from tests import test_trainer_gpu as TT

DEV = "cuda:0"
FB = 21168
LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL = TT.LOSS_ATOL, TT.LOSS_RTOL, TT.GRAD_ATOL, TT.GRAD_REL
PARAM_RTOL, PARAM_ATOL = 2e-5, 2e-6                    # tests/test_distributed_gpu.py: ranks against one process
FWD_ATOL, FWD_RTOL = 1e-5, 1e-5                        # SURVEY 8d's forward bar
LOSS_KEYS = ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss")
ADAM = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.01, clip_norm=40.0)
# per-actor arrays of a ring, compared exactly between a rank and its columns of the one-process run (those a ring has)
RING_PER_ACTOR = ("count", "episode", "ep_steps", "last_action", "last_reward", "r_action", "r_terminal", "r_reward",
                  "r_last_action")
# and those of a kind of environment (build()'s `state`): every name must be an array of the ring
RING_ARCADE = ("actor_records",)
RING_TOPDOWN = ("pos", "goal", "layout")
RING_GENERATED = ("pos", "goal", "heading", "actor_records")


# ---- A. a shard against the fp64 oracle -------------------------------------------------------------------------------------------
def shard_against_oracle(case, rank, world, B, H=40, T=5, updates=4):
    """case: dict(id, env_type, register(name) -> config, hosts(config, B, seed, actor_base, actors_total) -> host models,
    check(tr, hosts, what): the family's exact state comparison, [A], [net_seed], [partner: "selfplay" | "pool"]).
    -> dict(n_term, ended: episodes ended per actor, rewards, tr, hosts) after `updates` updates, every comparison of the
    family's own oracle test made."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.train.trainer import PhiloxDraws
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "sharded_%s_r%dw%d" % (case["id"], rank, world)
    registry = Environment.MAZE_CONFIG if case["env_type"] == "maze" else Environment.ARCADE_CONFIG
    conf = case["register"](name)
    partner = case.get("partner")
    try:
        cfg = TT._cfg(True, True, H, T)
        cfg["action_size"] = case.get("A", 4)
        cfg["initial_learning_rate"] = 7.0711e-4
        if case.get("objective_size"):
            cfg["objective_size"] = case["objective_size"]
        if partner == "pool":
            try:
                import test_versus_gpu as TV
            except ImportError:
                from tests import test_versus_gpu as TV
            draws = TT.RecordingDraws(PhiloxDraws(0xA3C, 0))
            net, applier, tr = TV._build_pool(name, B, T, H, True, True, draws=draws, seed=0xA3C, net_seed=3,
                                              opponent_pool=2, opponent_snapshot_every=1, rank=rank, world_size=world)
        else:
            net, applier, tr, draws = TT._build(cfg, B, seed=case.get("net_seed", 3), env_type=case["env_type"],
                                                env_name=name, rank=rank, world_size=world)
        assert (tr.rank, tr.world_size, tr.B) == (rank, world, B) and tr.grad_scale == 1.0 / (B * world)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = case["hosts"](conf, B, tr.seed, rank * B, world * B)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)

        # ---- replay fill ----------------------------------------------------------------------------------------------
        played = []
        if partner == "pool":
            fill = tr._fill_group

            def filling():
                fill()
                played.append(tr.opponent_actions[:B].cpu().numpy().copy())
            tr._fill_group = filling
        while not tr._full:
            assert tr.process(None, 0) == (0, None)
        # the device fills all actors in lock-step, the oracle each actor to exactly its history: the two agree only while no
        # actor discards a successive terminal frame (an episode that ends on its first step), which costs it one more call
        # (tests/test_fp_maze_gpu.py, above FP_ROOM).  The case's net_seed is picked so that none does.
        assert len(draws.log) == H, "the fill took %d calls: an episode ended on its first step" % len(draws.log)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        count = tr.ring.count.cpu().numpy()
        if partner == "selfplay":
            r_action = tr.ring.r_action.view(B, tr.ring.H1).cpu().numpy()
            assert (count == H).all()
            for b in range(B):
                hosts[b].partner.extend(int(a) for a in r_action[b ^ 1, :count[b ^ 1]])
        elif partner == "pool":
            for b in range(B):
                hosts[b].partner.extend(int(row[b]) for row in played)
        orc.fill()
        assert all(len(e.action_u) == 0 for e in edraws)
        assert not partner or not any(h.partner for h in hosts)
        np.testing.assert_array_equal(count, [a.exp.count for a in orc.actors])
        case["check"](tr, hosts, "after the fill")

        rewards, n_term, ended = set(), 0, np.zeros(B, np.int64)
        for it in range(updates):
            what = "update %d" % it
            draws.log.clear()
            lr = tr._anneal_learning_rate(0)
            tr.compute_gradients()
            # the rank's share of the job's gradient: 1 / world of the mean over its own actors
            g_dev = {k: world * v.detach().cpu().double().numpy() for k, v in net.g.items()}
            net.grads.flat.mul_(world)               # the other ranks sent the same: the step is the oracle's
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, lr)
            losses_dev = tr._publish_losses()
            TT._feed_draws(cfg, draws.log, edraws, T, B)
            n_dev = tr.n_steps.cpu().numpy()
            acts = tr.actions.cpu().numpy().reshape(T, B)
            rews = tr.rewards.cpu().numpy().reshape(T, B)
            if partner == "selfplay":
                assert (n_dev[0::2] == n_dev[1::2]).all()
                for b in range(B):
                    hosts[b].partner.extend(int(a) for a in acts[:n_dev[b ^ 1], b ^ 1])
            elif partner == "pool":
                opp = tr.opponent_actions.cpu().numpy().reshape(T, B)
                for b in range(B):
                    hosts[b].partner.extend(int(a) for a in opp[:n_dev[b], b])
            steps_o, infos, losses_o, mean_g, norm_o = orc.process_batched(0)
            assert not partner or not any(h.partner for h in hosts)

            # ---- exact: step counts, actions, rewards, terminals ---------------------------------------------------------
            assert int(n_dev.sum()) == steps_o
            te = tr.terminal_end.cpu().numpy()
            for b in range(B):
                n = infos[b]["n"]
                assert n_dev[b] == n, (what, b)
                assert list(acts[:n, b]) == infos[b]["actions"], (what, b)
                assert list(rews[:n, b]) == [float(r) for r in infos[b]["rewards"]], (what, b)
                assert bool(te[b]) == infos[b]["terminal_end"], (what, b)
                rewards |= set(float(r) for r in infos[b]["rewards"])
                n_term += infos[b]["terminal_end"]
                ended[b] += infos[b]["terminal_end"]
            # ---- losses: the mean over the rank's own actors --------------------------------------------------------------
            for key in LOSS_KEYS + ("entropy",):
                assert key in losses_dev, (what, key)
                if key == "entropy":
                    want = np.mean([l["entropy"].sum() for l in losses_o])
                elif key in losses_o[0]:
                    want = np.mean([l[key] for l in losses_o])
                else:
                    assert losses_dev[key] == 0.0, (what, key, losses_dev[key])    # a task that is off contributes nothing
                    continue
                bar = LOSS_ATOL + LOSS_RTOL * abs(want)
                margins.record("A %s" % key, abs(losses_dev[key] - want) / bar, "%g abs + %g rel" % (LOSS_ATOL, LOSS_RTOL))
                assert abs(losses_dev[key] - want) <= bar, (what, key, losses_dev[key], want)
            # ---- world * (the rank's gradient) against the oracle's mean gradient ------------------------------------------
            for (pname, _), gref in zip(orc.params.items(), mean_g):
                gr = gref.numpy().reshape(-1)
                tol = GRAD_ATOL + GRAD_REL * np.abs(gr).max()
                err = np.abs(g_dev[pname] - gr).max()
                margins.record("A world * g[%s]" % pname, err / tol, "%g + %g of max |g|" % (GRAD_ATOL, GRAD_REL))
                assert err <= tol, (what, pname, err, np.abs(gr).max())
            norm_dev = float(tr.last_grad_norm.cpu()[0])
            margins.record("A grad norm", abs(norm_dev - norm_o) / (1e-4 * max(1.0, norm_o)), "1e-4 rel")
            assert abs(norm_dev - norm_o) <= 1e-4 * max(1.0, norm_o), (what, norm_dev, norm_o)
            # ---- parameters after the step (tests/test_trainer_gpu.py: 2e-6 + 1e-5 of max |p|) -----------------------------
            for pname, ref in orc.params.items():
                got = net.p[pname].cpu().double().numpy()
                want = ref.numpy().reshape(-1)
                bar = 2e-6 + 1e-5 * np.abs(want).max()
                margins.record("A param %s after the step" % pname, np.abs(got - want).max() / bar, "2e-6 + 1e-5 of max |p|")
                assert np.abs(got - want).max() <= bar, (what, pname)
            case["check"](tr, hosts, what)
        assert all(len(e.seq_starts) == 0 and len(e.rp_u) == 0 for e in edraws)
        return dict(n_term=n_term, ended=ended, rewards=rewards, tr=tr, hosts=hosts)
    finally:
        registry.pop(name, None)
        Environment.action_size = -1


# ---- B, C. trainers on their own or on injected draws ---------------------------------------------------------------------------
class PlainDraws(object):
    """A draw stream that keeps its own columns: Trainer._point_draws' batch / col0 land on the wrapper and are not read."""

    def __init__(self, inner):
        self.inner = inner

    def uniform(self, out):
        return self.inner.uniform(out)

    def randint(self, high, out):
        return self.inner.randint(high, out)


def build(env_type, env_name, B, T, H, state=RING_ARCADE, rank=0, world_size=1, grad_sync=None, draws=None, adam=None,
          depth=False, seed=0xA3C, net_seed=5, **options):
    """A prepared full-UNREAL LSTM trainer, handed back before the replay fills (the caller hooks it first).  `state`: the
    ring arrays of its kind of environment that per_actor_state() compares beside RING_PER_ACTOR."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.adam_applier import AdamApplier
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    A = Environment.get_action_size(env_type, env_name)
    net = UnrealModel(A, Environment.get_objective_size(env_type, env_name), -1, True, True, True, True, 0.05, 0.001, DEV,
                      seed=net_seed, use_depth_prediction=depth)
    applier = AdamApplier(None, device=DEV, **adam) if adam is not None else \
        RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    if depth:
        options.update(use_depth_prediction=True, depth_lambda=0.7)
    tr = Trainer(rank, net, 7.0711e-4, None, applier, env_type, env_name, True, True, True, True, 0.05, 0.001, T, T, 0.99, 0.9,
                 H, 10 ** 6, DEV, batch_size=B, world_size=world_size, rank=rank, seed=seed, grad_sync=grad_sync, draws=draws,
                 **options)
    tr.prepare()
    tr.state_names = tuple(state)
    return net, applier, tr


def _np(t):
    return t.detach().cpu().numpy().copy()


def current_frames(ring):
    return ring.frames.view(-1, FB)[ring.cur_idx().long()].cpu().numpy()


def per_actor_state(tr):
    """The per-actor arrays of the trainer's ring (RING_PER_ACTOR and tr.state_names, each of which must exist) and of its
    environment -> {name: array [B, ...]}."""
    ring, B = tr.full_ring, tr.B
    out = {}
    for n in RING_PER_ACTOR + tuple(tr.state_names):
        t = getattr(ring, n)
        assert torch.is_tensor(t) and t.numel() and t.numel() % B == 0, (n, type(t))
        out[n] = _np(t).reshape(B, -1)
    out["frames of the current slot"] = current_frames(ring)
    conf = getattr(tr.full_environment, "config", None)
    if getattr(conf, "generate", None) is not None:
        out["current_layouts"] = tr.full_environment.current_layouts()[0].reshape(B, -1)
    if hasattr(tr.full_environment, "current_records"):
        out["current_records"] = tr.full_environment.current_records().reshape(B, -1)
    return out


def snapshot(tr, steps=None):
    """What one process() call left, per actor where it is per actor (rows t * Bg + b -> [T, Bg, ...])."""
    T, Bg, A = tr.n_step_TD, tr.Bg, tr.action_size
    s = dict(actions=_np(tr.actions).reshape(T, Bg), rewards=_np(tr.rewards).reshape(T, Bg),
             terminals=_np(tr.terminals).reshape(T, Bg), active_log=_np(tr.active_log).reshape(T, Bg),
             n_steps=_np(tr.n_steps), terminal_end=_np(tr.terminal_end), pi=_np(tr.pi).reshape(T, Bg, A),
             u_act=_np(tr.u_act).reshape(T, Bg), state=per_actor_state(tr), params=_np(tr.local_network.params.flat),
             losses=dict(tr.last_losses), steps=steps)
    if tr.opponent_pool:
        s["opp_u"] = _np(tr.opp_u).reshape(T, Bg)
    return s


def cdf_distance(pi, u):
    """The smallest distance of a draw to a step of its own row's CDF (the last step, 1, decides nothing)."""
    cdf = np.cumsum(pi.astype(np.float64), axis=-1)[..., :-1]
    return float(np.abs(u.astype(np.float64)[..., None] - cdf).min())


def run_job(make, rank, world, B, T, updates, whole_grads=None, whole_fill_calls=None):
    """One trainer of a job through its fill and `updates` process() calls.  make(rank, world, B, grad_sync) -> (net,
    applier, tr).  whole_grads None: the exchange only records the gradient (the one-process run); else it records the
    rank's own and hands back whole_grads[k], the update the one-process run applied, and the ranks' agreement on the end
    of the fill (parallel.all_true: the AND of every rank's "full" flag) is stood in for by the one-process run's own:
    all of its actors were full after whole_fill_calls calls, so the other ranks' flags are set from that call on.
    -> dict(grads: the recorded gradients, syncs: exchanges per process() call, fill: (pi, u, actions) of every fill step,
    snaps: snapshot() per call, offsets)."""
    grads = []

    def sync(flat):
        grads.append(flat.detach().clone())
        if whole_grads is not None:
            flat.copy_(whole_grads[len(grads) - 1])
    net, applier, tr = make(rank, world, B, sync)
    assert tr.groups == 1
    A, fill_rows, fill = tr.action_size, [], tr._fill_group

    def filling():
        fill()
        fill_rows.append((_np(tr.pi[:B * A]).reshape(B, A), _np(tr.u_act[:B]), _np(tr.actions[:B])))
    tr._fill_group = filling
    from unreal_amd import parallel
    all_true = parallel.all_true

    def job_is_full(flag, device):
        job = tr._fill_calls >= whole_fill_calls
        assert bool(flag) or not job, "rank %d is not full after the one-process run's %d calls" % (rank, whole_fill_calls)
        return bool(flag) and job
    if whole_fill_calls is not None:
        parallel.all_true = job_is_full
    try:
        while not tr._full:
            assert tr.process(None, 0) == (0, None)
    finally:
        parallel.all_true = all_true
    assert not grads
    snaps, syncs = [], []
    for k in range(updates):
        before = len(grads)
        steps, _ = tr.process(None, k * T * B * world)
        syncs.append(len(grads) - before)
        snaps.append(snapshot(tr, steps))
    torch.cuda.synchronize()
    return dict(grads=[_np(g) for g in grads], dev_grads=grads, syncs=syncs, fill=fill_rows, snaps=snaps,
                offsets=net.grads.offsets)


def compare_ranks_with_whole(make, B, T, updates=3, world=2, syncs_per_call=1):
    """Family B: `world` ranks of B actors, one after the other, against one process holding all world * B actors.
    -> the closest distance of an action draw of the one-process run to a step of its row's CDF."""
    whole = run_job(make, 0, 1, world * B, T, updates)
    assert whole["syncs"] == [syncs_per_call] * updates
    # the condition of the exact comparisons below, on the one-process run alone and on every row of it
    closest = min([cdf_distance(pi, u) for pi, u, _ in whole["fill"]] +
                  [cdf_distance(s["pi"], s["u_act"]) for s in whole["snaps"]])
    assert closest > FWD_ATOL, "an action draw lies %.3g from a step of its CDF: pick another seed" % closest
    ranks = [run_job(make, r, world, B, T, updates, whole_grads=whole["dev_grads"], whole_fill_calls=len(whole["fill"]))
             for r in range(world)]
    for r, job in enumerate(ranks):
        cols = slice(r * B, (r + 1) * B)
        assert job["syncs"] == whole["syncs"], (r, job["syncs"])
        assert len(job["fill"]) == len(whole["fill"])
        for step, ((pi, u, a), (wpi, wu, wa)) in enumerate(zip(job["fill"], whole["fill"])):
            np.testing.assert_array_equal(u, wu[cols], err_msg="rank %d fill step %d draws" % (r, step))
            np.testing.assert_array_equal(a, wa[cols], err_msg="rank %d fill step %d actions" % (r, step))
        for k, (s, w) in enumerate(zip(job["snaps"], whole["snaps"])):
            what = "rank %d call %d " % (r, k)
            for key in ("actions", "rewards", "terminals", "active_log", "u_act"):
                np.testing.assert_array_equal(s[key], w[key][:, cols], err_msg=what + key)
            for key in ("n_steps", "terminal_end"):
                np.testing.assert_array_equal(s[key], w[key][cols], err_msg=what + key)
            assert sorted(s["state"]) == sorted(w["state"])
            for key, v in s["state"].items():
                np.testing.assert_array_equal(v, w["state"][key][cols], err_msg=what + key)
            margins.record_close("B pi rows of a rank against the one-process rows", s["pi"], w["pi"][:, cols], FWD_ATOL,
                                 FWD_RTOL)
            np.testing.assert_allclose(s["pi"], w["pi"][:, cols], rtol=FWD_RTOL, atol=FWD_ATOL, err_msg=what + "pi")
        last, wlast = job["snaps"][-1]["params"], whole["snaps"][-1]["params"]
        margins.record_close("B parameters of a rank after the last call", last, wlast, PARAM_ATOL, PARAM_RTOL, survey=None)
        np.testing.assert_allclose(last, wlast, rtol=PARAM_RTOL, atol=PARAM_ATOL)
    for k in range(updates):
        assert sum(j["snaps"][k]["steps"] for j in ranks) == whole["snaps"][k]["steps"]
    # the ranks' gradients add up to the one-process gradient, per variable
    for k, G in enumerate(whole["grads"]):
        total = np.sum([j["grads"][k].astype(np.float64) for j in ranks], axis=0)
        for name, (o, n, _) in whole["offsets"].items():
            ref = G[o:o + n].astype(np.float64)
            ratio = grad_ratio(total[o:o + n], ref)
            print("B update %d g[%s]: %.3f of the bar, max |G| %.3g" % (k, name, ratio, np.abs(ref).max()))
            margins.record("B sum of the ranks' g[%s] against the one-process gradient" % name, ratio,
                           "%g of the variable's largest |G|" % GRAD_REL)
            assert ratio <= 1.0, (k, name, ratio, np.abs(ref).max())
    assert np.abs(whole["snaps"][-1]["params"] - whole["snaps"][0]["params"]).max() > 1e-6      # the updates moved the weights
    return closest


def grad_ratio(got, ref):
    """|got - ref| against GRAD_REL of the variable's largest |ref| element (tests/test_minibatch_gpu.py's bar for one device
    gradient against another: no absolute term); a variable whose reference is exactly zero must be exactly zero."""
    top = np.abs(ref).max()
    if top == 0:
        return float(np.abs(got).max() > 0)
    return float(np.abs(got - ref).max() / (GRAD_REL * top))


def hook_step(applier, log):
    """Wrap applier.step (tests/test_minibatch_gpu.py's _hook_step): the gradient every update receives goes to `log`."""
    inner = applier.step

    def step(flat_params, flat_grad, lr):
        log.append(_np(flat_grad))
        return inner(flat_params, flat_grad, lr)
    applier.step = step


def run_scaled_pair(env_type, env_name, B, T, H, steps_per_call, calls=3, seed=0x5EED, **options):
    """Family C: Trainer(rank=0, world_size=2) whose exchange doubles the gradient against Trainer(world_size=1), both on
    the same injected plain draws (and, with a pool, the same plain opponent draws), the same actors and weights.
    last_losses: every key at LOSS_RTOL; the LOSS_ATOL beside it is the suite's own guard for a value that is exactly 0
    (tests/test_trainer_gpu.py), which clip_fraction and a task without rows are."""
    from unreal_amd.train.trainer import PhiloxDraws
    runs = []
    for world in (2, 1):
        sync = (lambda flat: flat.mul_(2)) if world == 2 else None
        net, applier, tr = build(env_type, env_name, B, T, H, rank=0, world_size=world, grad_sync=sync,
                                 draws=PhiloxDraws(seed, 0), **options)
        assert tr.world_size == world and tr.grad_scale == 1.0 / (tr.Bg * world)
        if tr.opponent_pool:
            tr.opp_draws = PlainDraws(PhiloxDraws(seed ^ 0x4F505053, 0))
        got = []
        hook_step(applier, got)
        while not tr._full:
            assert tr.process(None, 0) == (0, None)
        assert not got
        snaps = []
        for k in range(calls):
            steps, _ = tr.process(None, k * T * B)
            snaps.append(snapshot(tr, steps))
        torch.cuda.synchronize()
        runs.append(dict(grads=got, snaps=snaps, offsets=net.grads.offsets))
    two, one = runs
    assert len(two["grads"]) == len(one["grads"]) == calls * steps_per_call
    for k, (s, w) in enumerate(zip(two["snaps"], one["snaps"])):
        what = "call %d " % k
        for key in ("actions", "rewards", "terminals", "active_log", "n_steps", "terminal_end", "u_act"):
            np.testing.assert_array_equal(s[key], w[key], err_msg=what + key)
        assert s["steps"] == w["steps"]
        for key, v in s["state"].items():
            np.testing.assert_array_equal(v, w["state"][key], err_msg=what + key)
        assert sorted(s["losses"]) == sorted(w["losses"]) and s["losses"]
        for key, want in w["losses"].items():
            got = s["losses"][key]
            if want is None or got is None:
                assert got == want, (what, key)
                continue
            bar = LOSS_ATOL + LOSS_RTOL * abs(want)
            margins.record("C %s" % key, abs(got - want) / bar, "%g abs + %g rel" % (LOSS_ATOL, LOSS_RTOL))
            assert abs(got - want) <= bar, (what, key, got, want)
    for k, (g2, g1) in enumerate(zip(two["grads"], one["grads"])):
        for name, (o, n, _) in one["offsets"].items():
            ref = g1[o:o + n].astype(np.float64)
            ratio = grad_ratio(g2[o:o + n].astype(np.float64), ref)
            print("C update %d g[%s]: %.3f of the bar, max |g| %.3g" % (k, name, ratio, np.abs(ref).max()))
            margins.record("C g[%s] at world_size 2 (doubled) against world_size 1" % name, ratio,
                           "%g of the variable's largest |g|" % GRAD_REL)
            assert ratio <= 1.0, (k, name, ratio, np.abs(ref).max())
    margins.record_close("C parameters after the last call", two["snaps"][-1]["params"], one["snaps"][-1]["params"],
                         PARAM_ATOL, PARAM_RTOL, survey=None)
    np.testing.assert_allclose(two["snaps"][-1]["params"], one["snaps"][-1]["params"], rtol=PARAM_RTOL, atol=PARAM_ATOL)
    assert np.abs(one["snaps"][-1]["params"] - one["snaps"][0]["params"]).max() > 1e-6
    return two, one
