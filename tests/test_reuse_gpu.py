"""Sample reuse on the device: unreal_ppo_heads_loss_grad against unreal_policy_step (bit for bit), the fp64
loss model of tests/ppo_model.py and unreal_base_loss_grad; the trainer with the option off, with unchanged weights, and its
reuse updates rebuilt in fp64 from its own buffers."""
import numpy as np
import pytest
import torch

try:
    import maze_model as MM
    import ppo_model as PM
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM
    from tests import ppo_model as PM
from oracle import model as OM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB = 21168
LOSS_RTOL = 1e-4                      # the project's loss bar (tests/test_trainer_gpu.py)
GRAD_REL = 2e-5                       # of the variable's largest |gradient|
FWD_ATOL, FWD_RTOL = 1e-5, 1e-5       # the project's forward bar (tests/test_kernels_gpu.py)
EDGE = 1e-4                           # no row's rho may be this close to a clip edge: the fp32 decision is then the fp64 one
EPS, BETA, SCALE = 0.2, 0.01, 0.37
RHOS = (0.3, 0.79, 0.81, 1.0, 1.19, 1.21, 3.0)


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


# ---- 1-3. the kernel ---------------------------------------------------------------------------------------------------------------
class _Case(object):
    """Feature rows, head weights and the per-row inputs of the loss; the two special rows sit at the end."""

    def __init__(self, rows, A, ldx, seed=0):
        rs = np.random.RandomState(1000 * A + rows + ldx + seed)
        self.rows, self.A, self.ldx = rows, A, ldx
        X = rs.uniform(-1, 1, (rows, ldx)).astype(np.float32)
        self.tiny = rows - 2 if rows > 2 else None               # a row whose features put a new probability below 1e-12
        self.floor = rows - 3 if rows > 2 else None              # a row whose old probability is below the clip floor
        if self.tiny is not None:
            X[self.tiny] *= 30.0
        self.X = _dev(X.reshape(-1), torch.float32)
        self.Wp = _dev(rs.uniform(-.3, .3, 256 * A), torch.float32)
        self.bp = _dev(rs.uniform(-.1, .1, A), torch.float32)
        self.Wv = _dev(rs.uniform(-.3, .3, 256), torch.float32)
        self.bv = _dev(rs.uniform(-.1, .1, 1), torch.float32)
        self.action = rs.randint(0, A, rows).astype(np.int32)
        i = np.arange(rows)
        self.factor = np.array(RHOS)[i % len(RHOS)]
        sign = np.where((i // len(RHOS)) % 2 == 0, 1.0, -1.0)
        self.adv = (sign * rs.uniform(0.2, 1.5, rows)).astype(np.float32)
        self.R = rs.normal(0, 1, rows).astype(np.float32)
        self.active = (i % 5 != 3).astype(np.int32)
        for r in (self.tiny, self.floor):
            if r is not None:
                self.active[r] = 1
        if self.floor is not None:
            self.adv[self.floor] = abs(self.adv[self.floor])     # (clipped: the row's loss stays of the others' size)
        f = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
        self.pi, self.v = f(rows * A), f(rows)

    def launch(self, pi_old, ld_old, active, dlogits, dv, losses, stats_i, stats_f, eps=EPS):
        from unreal_amd import ops
        ops.ppo_heads_loss_grad(self.rows, self.A, self.X, self.ldx, self.Wp, self.bp, self.Wv, self.bv, pi_old, ld_old,
                                _dev(self.action, torch.int32), _dev(self.adv, torch.float32), _dev(self.R, torch.float32),
                                _dev(active, torch.int32), eps, BETA, SCALE, self.pi, self.v, dlogits, dv, losses, stats_i,
                                stats_f)

    def forward_only(self):
        """pi_out / v_out of the rows (old policy: anything valid) -> numpy [rows, A], [rows]."""
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
        self.launch(torch.full((self.rows * self.A,), 0.5, device=DEV), self.A, self.active, None, None, z(3),
                    z(2, torch.int32), z(2))
        return self.pi.cpu().numpy().reshape(self.rows, self.A).copy(), self.v.cpu().numpy().copy()


@pytest.mark.parametrize("ldx", [256, 264])
@pytest.mark.parametrize("A", [3, 4, 6, 18])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_kernel_heads_are_policy_step_bit_for_bit(rows, A, ldx):
    """257 rows: one past a 256-thread block, and with 4 rows per workgroup a ragged last workgroup."""
    from unreal_amd import ops
    c = _Case(rows, A, ldx)
    pi, v = c.forward_only()
    f = lambda n: torch.full((n,), 9.0, dtype=torch.float32, device=DEV)
    pi_ref, v_ref, act = f(rows * A), f(rows), torch.zeros(rows, dtype=torch.int32, device=DEV)
    ops.policy_step(rows, A, c.X, ldx, c.Wp, c.bp, c.Wv, c.bv, None, pi_ref, v_ref, act)
    np.testing.assert_array_equal(pi.view(np.uint32), pi_ref.cpu().numpy().reshape(rows, A).view(np.uint32))
    np.testing.assert_array_equal(v.view(np.uint32), v_ref.cpu().numpy().view(np.uint32))
    assert np.isfinite(pi).all() and np.abs(pi.sum(1) - 1).max() < 1e-5


def _check_against_model(c, pi, v, pi_old, ld_old, active, what):
    """One launch with gradients from non-zero accumulators, held against the fp64 model fed the kernel's own pi / v."""
    rows, A = c.rows, c.A
    po = pi_old.reshape(rows, ld_old)[:, :A]
    want = PM.ppo_loss(pi.astype(np.float64), v.astype(np.float64), po.astype(np.float64), c.action, c.adv, c.R, active, EPS,
                       BETA, SCALE)
    assert PM.edge_distance(want["rho"], EPS) > EDGE             # every row, active or not: none is left out
    dl = torch.full((rows * A,), 7.0, device=DEV)
    dv = torch.full((rows,), 7.0, device=DEV)
    losses = torch.full((3,), 0.5, device=DEV)                    # the kernel adds to what is there
    stats_i = _dev(np.array([3, 7], np.int32), torch.int32)
    stats_f = torch.full((2,), 0.5, device=DEV)
    c.launch(_dev(pi_old.reshape(-1), torch.float32), ld_old, active, dl, dv, losses, stats_i, stats_f)
    np.testing.assert_array_equal(c.pi.cpu().numpy().reshape(rows, A), pi)      # the same heads again
    got_l = losses.cpu().numpy().astype(np.float64) - 0.5
    got_d = dl.cpu().numpy().reshape(rows, A).astype(np.float64)
    got_dv = dv.cpu().numpy().astype(np.float64)
    got_f = stats_f.cpu().numpy().astype(np.float64) - 0.5
    print("%s: losses %s want %s rel %s; max |d dlogits| %.3g, |d dv| %.3g; kl %.9g want %.9g; clipped %d of %d" % (
        what, got_l, want["losses"], np.abs(got_l - want["losses"]) / np.abs(want["losses"]),
        np.abs(got_d - want["dlogits"]).max(), np.abs(got_dv - want["dv"]).max(), got_f[0], want["kl_sum"], want["clipped"],
        want["counted"]))
    assert (np.abs(got_l - want["losses"]) <= LOSS_RTOL * np.abs(want["losses"])).all()
    assert (np.abs(got_d - want["dlogits"]) <= 1e-5 + 1e-5 * np.abs(want["dlogits"])).all()
    assert (np.abs(got_dv - want["dv"]) <= 1e-5 + 1e-5 * np.abs(want["dv"])).all()
    on = active.astype(bool)
    assert (got_d[~on] == 0).all() and (got_dv[~on] == 0).all() and np.isfinite(got_d).all()
    assert (stats_i.cpu().numpy() - [3, 7]).tolist() == [want["clipped"], want["counted"]]
    assert abs(got_f[0] - want["kl_sum"]) <= LOSS_RTOL * abs(want["kl_sum"])
    assert abs(got_f[1] - want["abs_sum"]) <= LOSS_RTOL * abs(want["abs_sum"])
    return want


@pytest.mark.parametrize("A", [3, 4, 6, 18])
def test_kernel_loss_against_fp64(A):
    rows, ldx, ld_old = 257, 264, A + 2
    c = _Case(rows, A, ldx)
    pi, v = c.forward_only()
    # the tiny row acts on its least likely action, which the heads put below 1e-12
    c.action[c.tiny] = int(pi[c.tiny].argmin())
    assert pi[c.tiny].min() < 1e-12
    c.factor[c.tiny] = 1.0
    rs = np.random.RandomState(A)
    pi_old = rs.uniform(0.01, 1, (rows, ld_old)).astype(np.float32)
    r = np.arange(rows)
    pi_old[r, c.action] = (pi[r, c.action].astype(np.float64) / c.factor).astype(np.float32)   # rho = factor, but for rounding
    pi_old[c.floor, c.action[c.floor]] = 1e-25                    # below the floor: p_old = 1e-20
    want = _check_against_model(c, pi, v, pi_old, ld_old, c.active, "A=%d all rows" % A)
    on = c.active.astype(bool)
    assert 0 < on.sum() < rows and 0 < want["clipped"] < want["counted"]
    rho = want["rho"]
    for sgn in (1, -1):                                           # every (sign of A) x (rho value) among the active rows
        for f in RHOS:
            assert (on & (np.sign(c.adv) == sgn) & (np.abs(rho - f) < 1e-6)).any(), (sgn, f)
    assert rho[c.floor] > 1e15 and not want["unclipped"][c.floor]
    assert want["unclipped"][on & (rho == 1.0)].all()            # ties at rho = 1 and everything between the edges
    # the same rows with the floor row switched off: the KL and |rho - 1| sums are then those of ordinary rows
    active2 = c.active.copy()
    active2[c.floor] = 0
    want2 = _check_against_model(c, pi, v, pi_old, ld_old, active2, "A=%d without the floor row" % A)
    assert want2["kl_sum"] < 1e3 and want2["counted"] == want["counted"] - 1
    # forward only: the same sums, and no gradient is written anywhere
    dl = torch.full((rows * A,), 7.0, device=DEV)
    dv = torch.full((rows,), 7.0, device=DEV)
    losses, stats_i, stats_f = torch.zeros(3, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV)
    c.launch(_dev(pi_old.reshape(-1), torch.float32), ld_old, active2, None, None, losses, stats_i, stats_f)
    assert (np.abs(losses.cpu().numpy() - want2["losses"]) <= LOSS_RTOL * np.abs(want2["losses"])).all()
    assert stats_i.cpu().numpy().tolist() == [want2["clipped"], want2["counted"]]
    assert (dl == 7.0).all() and (dv == 7.0).all()


@pytest.mark.parametrize("A", [4, 18])
def test_kernel_at_rho_1_is_base_loss_grad(A):
    from unreal_amd import ops
    rows, ldx = 257, 256
    c = _Case(rows, A, ldx, seed=1)
    pi, v = c.forward_only()
    f = lambda n, x=7.0: torch.full((n,), x, dtype=torch.float32, device=DEV)
    dl, dv, losses = f(rows * A), f(rows), f(3, 0.0)
    stats_i, stats_f = torch.zeros(2, dtype=torch.int32, device=DEV), f(2, 0.0)
    pi_old = c.pi.clone()
    c.launch(pi_old, A, c.active, dl, dv, losses, stats_i, stats_f)
    dl_ref, dv_ref, losses_ref = f(rows * A), f(rows), f(3, 0.0)
    ops.base_loss_grad(rows, A, pi_old, A, c.v, _dev(c.action, torch.int32), _dev(c.adv, torch.float32),
                       _dev(c.R, torch.float32), _dev(c.active, torch.int32), BETA, SCALE, dl_ref, dv_ref, losses_ref)
    got, want = dl.cpu().numpy().astype(np.float64), dl_ref.cpu().numpy().astype(np.float64)
    print("rho = 1, A=%d: max |d dlogits| %.3g, max |d dv| %.3g" % (A, np.abs(got - want).max(),
                                                                    float((dv - dv_ref).abs().max())))
    assert (np.abs(got - want) <= 1e-5 + 1e-5 * np.abs(want)).all()
    gv, wv = dv.cpu().numpy().astype(np.float64), dv_ref.cpu().numpy().astype(np.float64)
    assert (np.abs(gv - wv) <= 1e-5 + 1e-5 * np.abs(wv)).all()
    assert stats_i.cpu().numpy().tolist() == [0, int(c.active.sum())]
    assert stats_f.cpu().numpy().tolist() == [0.0, 0.0]          # rho is 1 exactly: the KL sum is 0 exactly
    lg, lw = losses.cpu().numpy().astype(np.float64), losses_ref.cpu().numpy().astype(np.float64)
    assert (np.abs(lg[1:] - lw[1:]) <= LOSS_RTOL * np.abs(lw[1:])).all()       # value and entropy sums are the same sums


# ---- 4-6. the trainer on a first-person maze ----------------------------------------------------------------------------------------
ENV_NAME = "reuse_gpu_fp7"


@pytest.fixture
def fp7():
    """First-person N = 7 with a step limit of 3: every actor ends inside a 5-step rollout, so rows past an episode's end
    exist (the configuration of tests/test_depth_gpu.py's trainer tests, under its own name)."""
    from unreal_amd.environment.environment import Environment
    rs = np.random.RandomState(7)
    Environment.register_maze_config(ENV_NAME, [MM.random_layout(7, rs, marks="") for _ in range(2)], view="first_person",
                                     random_start=True, random_goal=True, max_episode_steps=3)
    yield Environment.MAZE_CONFIG[ENV_NAME]
    Environment.MAZE_CONFIG.pop(ENV_NAME, None)


def _trainer(Bn, T, Hn, lstm, aux=False, groups=1, depth=False, env=("maze", ENV_NAME), lr0=7.0711e-4, seed=21, **options):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    A = Environment.get_action_size(*env)
    net = UnrealModel(A, 0, -1, lstm, aux, aux, aux, 0.05, 0.001, DEV, seed=4, use_depth_prediction=depth)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    if depth:
        options.update(use_depth_prediction=True, depth_lambda=0.7)
    tr = Trainer(0, net, lr0, None, applier, env[0], env[1], lstm, aux, aux, aux, 0.05, 0.001, T, T, 0.99, 0.9, Hn,
                 10 ** 6, DEV, batch_size=Bn, groups=groups, seed=seed, **options)
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    return net, applier, tr


REUSE_BUFFERS = ("pi_new", "v_new", "reuse_stats_i", "reuse_stats_f", "reuse_loss_sum")
REUSE_KEYS = ("reuse_policy_loss", "reuse_value_loss", "reuse_entropy", "clip_fraction", "approx_kl")


def test_option_off_is_todays_trainer(fp7):
    """reuse_epochs=1 and no argument at all: the same parameters bit for bit after three calls, none of the new buffers
    and none of the new keys.  Bit for bit is asked where today's trainer itself repeats bit for bit from run to run: one
    actor, the auxiliary heads off (measured: 32 of 32 pairs of runs identical; with more actors or the replay branches the
    float atomics of the weight-gradient kernels make two runs of the SAME trainer differ in a few hundred last bits, so
    full UNREAL with groups = 2 is held to the 1e-5 that tests/test_trainer_gpu.py asks of two schedules of one algorithm)."""
    for (Bn, aux, groups), exact in (((1, False, 1), True), ((4, True, 2), False)):
        flats = []
        for options in (dict(reuse_epochs=1), {}):
            net, applier, tr = _trainer(Bn, 5, 16, True, aux=aux, groups=groups, **options)
            for it in range(3):
                steps, _ = tr.process(None, 0)
                assert steps > 0
            assert tr.reuse_epochs == 1 and not any(hasattr(tr, name) for name in REUSE_BUFFERS)
            assert not any(k in tr.last_losses for k in REUSE_KEYS)
            with pytest.raises(ValueError, match="reuse_epochs"):
                tr.reuse_gradients()
            flats.append(net.params.flat.cpu().numpy().copy())
        if exact:
            np.testing.assert_array_equal(flats[0].view(np.uint32), flats[1].view(np.uint32))
        else:
            np.testing.assert_allclose(flats[0], flats[1], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("lstm", [True, False])
def test_reuse_pass_with_unchanged_weights_is_the_rollouts_pass(fp7, lstm):
    """compute_gradients(), then the reuse pass WITHOUT an update in between: the trunk re-run over all T * B rows at once
    gives the policy the rollout computed step by step, and at rho = 1 the clipped surrogate's gradient is A3C's."""
    T = 5
    net, applier, tr = _trainer(3, T, 12, lstm, depth=True, reuse_epochs=2)
    ended = 0
    for it in range(2):
        tr._select_group(0)
        tr.compute_gradients()
        saved = net.grads.flat.clone()
        carried = (tr.lstm_c.clone(), tr.lstm_h.clone(), tr.pi.clone(), tr.v.clone(), tr.boot_v.clone())
        tr.reuse_stats_i.zero_()
        tr.reuse_gradients()
        for a, b in zip(carried, (tr.lstm_c, tr.lstm_h, tr.pi, tr.v, tr.boot_v)):
            assert torch.equal(a, b)                              # the carried state and the behaviour policy are not touched
        pi, pi_new = tr.pi.cpu().numpy().astype(np.float64), tr.pi_new.cpu().numpy().astype(np.float64)
        v, v_new = tr.v.cpu().numpy().astype(np.float64), tr.v_new.cpu().numpy().astype(np.float64)
        print("lstm=%s it=%d: max |d pi| %.3g, max |d v| %.3g" % (lstm, it, np.abs(pi_new - pi).max(), np.abs(v_new - v).max()))
        assert (np.abs(pi_new - pi) <= FWD_ATOL + FWD_RTOL * np.abs(pi)).all()
        assert (np.abs(v_new - v) <= FWD_ATOL + FWD_RTOL * np.abs(v)).all()
        on = tr.active_log.cpu().numpy().astype(bool)
        ended += int((~on).sum())
        assert tr.reuse_stats_i.cpu().numpy().tolist() == [0, int(on.sum())]
        saved = net.grads.make_views(saved)
        for name, _, _ in net.spec:
            want = saved[name].cpu().numpy().astype(np.float64)
            got = net.grads.shaped(name).cpu().numpy().astype(np.float64).reshape(-1)
            tol = GRAD_REL * np.abs(want).max()
            err = np.abs(got - want).max()
            print("  g[%s]: max |d| %.3g, bar %.3g (%.3f of it)" % (name, err, tol, err / tol))
            assert err <= tol, (name, err, tol)
        tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, tr._anneal_learning_rate(0))
        net.mark_params_changed()
    assert ended > 0                                              # rows past an episode's end were masked out


def _rebuild(net, tr, T, lstm, reuse, depth_lam):
    """The base pass of the selected group in fp64 from the trainer's buffers and current weights, as
    tests/test_depth_gpu.py's _rebuild; `reuse`: with the clipped surrogate against the rollout's policy tr.pi.
    -> ((policy, value, entropy) as tr.losses holds them, {name: mean gradient}, info)."""
    Bg, A, ws, ring = tr.Bg, 4, tr.base_ws, tr.ring
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in net.export_named().items()}
    idx = ws.frame_idx[:T * Bg].cpu().numpy().astype(np.int64)
    frames = ring.frames[:ring.B * ring.H1 * FB].view(-1, FB).cpu().numpy()[idx].reshape(T, Bg, 84, 84, 3)
    labels = ring.r_depth.view(-1, 12).cpu().numpy()[idx].reshape(T, Bg, 12) if depth_lam else None
    xcat = ws.xcat[:T * Bg * ws.xld].view(T, Bg, ws.xld).cpu().numpy().astype(np.float64)
    acts = tr.actions.cpu().numpy().reshape(T, Bg)
    adv = tr.adv.cpu().numpy().reshape(T, Bg).astype(np.float64)
    R = tr.R.cpu().numpy().reshape(T, Bg).astype(np.float64)
    on = tr.active_log.cpu().numpy().reshape(T, Bg).astype(bool)
    pi_old = tr.pi.cpu().numpy().reshape(T, Bg, A).astype(np.float64)
    total, sums = 0.0, np.zeros(3)
    rho, clipped = [], 0
    for b in range(Bg):
        x = torch.tensor(frames[:, b].astype(np.float64) / 255.0)
        lar = torch.tensor(xcat[:, b, 256:256 + A + 1])
        state = None
        if lstm:
            state = (torch.tensor(ws.c0[b * 256:(b + 1) * 256].cpu().numpy().astype(np.float64)),
                     torch.tensor(ws.h0[b * 256:(b + 1) * 256].cpu().numpy().astype(np.float64)))
        feat, _ = OM.trunk(x, lar, p, lstm, state)
        feat = feat[torch.tensor(np.flatnonzero(on[:, b]))]
        pi, v = OM.policy_value(feat, p)
        a = acts[on[:, b], b]
        onehot = torch.tensor(np.eye(A)[a])
        adv_b, R_b = torch.tensor(adv[on[:, b], b]), torch.tensor(R[on[:, b], b])
        if reuse:
            po = pi_old[on[:, b], b][np.arange(len(a)), a]
            pl, vl, ent = PM.surrogate_torch(pi, v, torch.tensor(po), onehot, adv_b, R_b, tr.ppo_clip, 0.001)
            m = PM.ppo_loss(pi.detach().numpy(), v.detach().numpy(), po, a, adv_b.numpy(), R_b.numpy(), np.ones(len(a)),
                            tr.ppo_clip, 0.001, 1.0)
            rho += m["rho"].tolist()
            clipped += m["clipped"]
        else:
            pl, vl, ent = OM.base_loss(pi, v, onehot, adv_b, R_b, 0.001)
        total = total + pl + vl
        sums += [pl.item(), vl.item(), ent.sum().item()]
        if depth_lam:
            h = torch.relu(feat @ p["W_dp_fc1"] + p["b_dp_fc1"])
            z = (h @ p["W_dp_fc2"] + p["b_dp_fc2"]).reshape(-1, 12, 8)
            lab = torch.tensor(labels[on[:, b], b].astype(np.int64))
            total = total - depth_lam * torch.log_softmax(z, dim=2).gather(2, lab[:, :, None]).sum()
    (total / Bg).backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()}
    return sums / Bg, grads, dict(on=on, rho=np.array(rho), clipped=clipped, counted=int(on.sum()))


# ppo_clip, learning rate and trainer seed per case, found by search on the device so that the fp64 rebuild of at least one
# reuse update has clipped AND unclipped active rows and no row within EDGE of a clip edge (asserted below)
CASES = [
    # lstm, groups, depth, options, (ppo_clip, lr0, seed)
    (True, 1, False, {}, (0.01, 0.1, 21)),
    (False, 1, False, {}, (0.01, 0.1, 21)),
    (True, 2, False, {}, (0.01, 0.1, 21)),
    (False, 2, False, {}, (0.05, 0.02, 21)),
    (True, 2, False, dict(bootstrap_timeouts=True, gae_lambda=0.9), (0.01, 0.1, 21)),
    (True, 1, True, {}, (0.01, 0.1, 21)),
]


def run_case(lstm, groups, depth, options, picked, check=True):
    """The three updates of every group, each rebuilt in fp64 -> per-update records (the search prints them)."""
    ppo_clip, lr0, seed = picked
    Bn, T, E = (3 if groups == 1 else 4), 5, 3
    net, applier, tr = _trainer(Bn, T, 12, lstm, groups=groups, depth=depth, lr0=lr0, seed=seed, reuse_epochs=E,
                                ppo_clip=ppo_clip, **options)
    depth_lam = 0.7 if depth else 0.0
    records, worst = [], 0.0
    for g in range(groups):
        tr._select_group(g)
        for e in range(E):
            tr.reuse_stats_i.zero_()
            if e == 0:
                tr.compute_gradients()
            else:
                tr.reuse_gradients()
            want_l, want_g, info = _rebuild(net, tr, T, lstm, e > 0, depth_lam)
            got_l = tr.losses.cpu().numpy()[:3].astype(np.float64)
            rec = dict(g=g, e=e, counted=info["counted"], ended=int((~info["on"]).sum()))
            rec["loss_ratio"] = float((np.abs(got_l - want_l) / (LOSS_RTOL * np.abs(want_l))).max())
            if e > 0:
                rec.update(clipped=info["clipped"], edge=PM.edge_distance(info["rho"], ppo_clip),
                           rho_min=float(info["rho"].min()), rho_max=float(info["rho"].max()),
                           stats=tr.reuse_stats_i.cpu().numpy().tolist())
            ratios = {}
            for name, gw in want_g.items():
                gd = net.grads.shaped(name).cpu().numpy().astype(np.float64)
                ratios[name] = float(np.abs(gd - gw).max() / (GRAD_REL * np.abs(gw).max()))
            rec["grad_ratio"] = max(ratios.values())
            rec["grad_worst"] = max(ratios, key=ratios.get)
            worst = max(worst, rec["grad_ratio"], rec["loss_ratio"])
            print("lstm=%s groups=%d depth=%s %s: %s" % (lstm, groups, depth, sorted(options), rec))
            if check:
                assert rec["loss_ratio"] <= 1.0, (rec, got_l, want_l)
                assert rec["grad_ratio"] <= 1.0, rec
                if e > 0:
                    assert rec["edge"] > EDGE, rec                # asserted, not skipped
                    assert rec["stats"] == [info["clipped"], info["counted"]], rec      # clip_fraction is exact
            records.append(rec)
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, tr._anneal_learning_rate(0))
            net.mark_params_changed()
    print("worst error / bar: %.3f" % worst)
    return records


@pytest.mark.parametrize("lstm,groups,depth,options,picked", CASES)
def test_reuse_updates_against_fp64(fp7, lstm, groups, depth, options, picked):
    """reuse_epochs = 3, B = 3 actors (4 with groups = 2), T = 5, history 12, the other auxiliary heads off: after every one
    of the three updates of a group the pass is rebuilt in fp64 from the trainer's buffers with pi_old = tr.pi."""
    records = run_case(lstm, groups, depth, options, picked)
    assert sum(r["ended"] for r in records) > 0                  # rows past an episode's end were masked out
    assert any(r["e"] > 0 and 0 < r["clipped"] < r["counted"] for r in records), records


# ---- 7. full UNREAL ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [("maze", ""), ("arcade", "reuse_gpu_breakout")])
def test_full_unreal_with_reuse(env):
    """reuse_epochs = 2, groups = 2, LSTM + pixel control + value replay + reward prediction, on the reference's top-down
    maze and the arcade's default Breakout, next to the same trainer with the option off."""
    from unreal_amd.environment.environment import Environment
    if env[0] == "arcade":
        Environment.register_arcade_config(env[1])
    try:
        out = {}
        for E in (1, 2):
            net, applier, tr = _trainer(4, 5, 16, True, aux=True, groups=2, env=env, reuse_epochs=E)
            rolled = []                                           # env steps of every rollout, counted on its own
            inner = tr.compute_gradients

            def counting():
                inner()
                rolled.append(int(tr.active_log.sum()))
            tr.compute_gradients = counting
            steps, draws = [], []
            for it in range(3):
                c0 = tr.draws.counter
                del rolled[:]
                s, _ = tr.process(None, 0)
                # the steps of the call's two rollouts, whatever E: a reuse pass takes no environment step
                assert len(rolled) == 2 and s == sum(rolled) and 0 < s <= 4 * 5, (s, rolled)
                steps.append(s)
                draws.append(tr.draws.counter - c0)
                l = tr.last_losses
                assert all(np.isfinite(v) for v in l.values()), l
                if E > 1:
                    assert all(k in l for k in REUSE_KEYS), l
                    assert 0.0 <= l["clip_fraction"] <= 1.0 and l["approx_kl"] >= 0.0 and l["reuse_entropy"] > 0.0
                    si = tr.reuse_stats_i.cpu().numpy()
                    assert si[1] == s and l["clip_fraction"] == float(si[0]) / max(int(si[1]), 1)   # one reuse update per group
                else:
                    assert not any(k in l for k in REUSE_KEYS)
            assert bool(torch.isfinite(net.params.flat).all())
            out[E] = (steps, draws)
        G = 2
        # the first rollout of the first call sees the same weights and draws in both trainers
        assert out[1][0][0] > 0 and out[2][0][0] > 0
        for d1, d2 in zip(out[1][1], out[2][1]):
            aux = d1 // G - 1                                     # per group: one rollout draw + the auxiliary draws
            assert d1 == G * (1 + aux) and aux > 0
            assert d2 == G * (1 + 2 * aux), (d1, d2)              # twice the auxiliary draws plus one rollout's
    finally:
        Environment.ARCADE_CONFIG.pop(env[1], None)
