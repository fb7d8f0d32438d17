"""Time-limit bootstrapping and GAE(lambda) on the device: the _tl rollout entries of the arcade and of the
first-person mazes against the host models through the scripted traces of tests/timelimit_cases.py (which
tests/test_timelimit_cpu.py checks for their cases), group views, unreal_base_returns_tl against the scan in numpy fp64,
unreal_boot_gather, and the Trainer end to end."""
import numpy as np
import pytest
import torch

try:
    import timelimit_cases as TC
    from test_trainer_gpu import _cfg
except ImportError:            # imported as tests.<module>
    from tests import timelimit_cases as TC
    from tests.test_trainer_gpu import _cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
SENTINEL = 0xAB
A, XLD = 4, 264
H = TC.STEPS + 2             # no ring slot is written twice: the ring keeps every step of a trace
RING = ("r_reward", "r_action", "r_last_action", "r_last_reward", "r_pc", "pos", "count", "last_action", "last_reward",
        "episode_reward", "score_out", "score_valid", "ep_steps", "episode")


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _arcade_env(conf, n, final_obs, **kw):
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    return _fresh(BatchedArcadeEnvironment(n, H, DEV, config=conf, seed=TC.SEED, final_obs=final_obs, **kw), final_obs)


def _maze_env(conf, n, final_obs):
    from unreal_amd.environment.maze_environment import batched_maze_environment
    return _fresh(batched_maze_environment(n, H, DEV, config=conf, seed=TC.SEED, final_obs=final_obs), final_obs)


def _fresh(env, final_obs):
    env.ring.frames.zero_()
    env.ring.r_pc.zero_()
    env.reset()                        # (episode 1, as the host models of TC.arcade_models / TC.maze_models)
    assert (env.ring.final_obs is not None) == final_obs
    if final_obs:
        assert env.ring.frames.numel() == (env.ring.B * env.ring.H1 + env.ring.B) * FB
        assert env.ring.final_obs.data_ptr() == env.ring.frames.data_ptr() + env.ring.final_base * FB
        env.ring.final_obs.fill_(SENTINEL)
    else:
        assert env.ring.frames.numel() == env.ring.B * env.ring.H1 * FB       # what a ring has always allocated
    return env


class _Scripted(object):
    """A policy head that draws the scripted action: feature row e_a, logit 100 for action a, u = 0.5."""

    def __init__(self):
        Wp = np.zeros((256, A), np.float32)
        Wp[np.arange(A), np.arange(A)] = 100.0
        self.p = dict(W_base_fc_p=_dev(Wp.reshape(-1), torch.float32), b_base_fc_p=torch.zeros(A, device=DEV),
                      W_base_fc_v=torch.zeros(256, device=DEV), b_base_fc_v=torch.zeros(1, device=DEV))

    def features(self, actions):
        X = np.zeros((len(actions), 256), np.float32)
        X[np.arange(len(actions)), actions] = 1.0
        return _dev(X.reshape(-1), torch.float32)


def _drive(envs, actions, fused, parts=None):
    """Step every environment of `envs` through actions [S, n] with its rollout entry (`fused`: the policy form), all
    actors re-armed before every step.  `parts`: [(b0, b1)] the actors of each item of an environment given as a list of
    views (index_parent).  -> per environment a dict of per-step logs [S, n]: r, t, te, n, log, idx, lar, act and `final`
    [S, n, FB], the final-observation slots after every step (None without a store)."""
    S, n = actions.shape
    net = _Scripted()
    u = torch.full((n,), 0.5, dtype=torch.float64, device=DEV)
    outs = []
    for env in envs:
        views = env if isinstance(env, list) else [env]
        spans = parts if isinstance(env, list) else [(0, n)]
        z = lambda dt=torch.int32, m=n: torch.zeros(m, dtype=dt, device=DEV)
        st = dict(r=z(torch.float32), t=z(), te=z(), n=z(), log=z(), idx=z(), active=z(), a=z(), v=z(torch.float32),
                  pi=z(torch.float32, n * A), lar=z(torch.float32, n * XLD))
        logs = {k: [] for k in ("r", "t", "te", "n", "log", "idx", "lar", "act", "final")}
        parent = getattr(views[0], "_parent_ring", views[0].ring)
        for s in range(S):
            st["active"].fill_(1); st["te"].zero_(); st["n"].zero_(); st["t"].fill_(-7); st["r"].fill_(-7.5)
            acts = _dev(actions[s], torch.int32)
            X = net.features(actions[s])
            for v, (b0, b1) in zip(views, spans):
                sl = {k: t[b0:b1] for k, t in st.items() if k not in ("pi", "lar")}
                nxt = dict(next_idx=sl["idx"], next_lar=st["lar"][b0 * XLD:b1 * XLD], lar_ld=XLD, lar_col0=256, A=A)
                ip = dict(index_parent=True) if isinstance(env, list) else {}
                if fused:
                    v.policy_rollout_step(net, X[b0 * 256:b1 * 256], 256, u[b0:b1], st["pi"][b0 * A:b1 * A], sl["v"], sl["a"],
                                          sl["r"], sl["t"], sl["active"], sl["log"], sl["n"], sl["te"], **ip, **nxt)
                else:
                    sl["a"].copy_(acts[b0:b1])
                    v.rollout_step(sl["a"], sl["r"], sl["t"], sl["active"], sl["log"], sl["n"], sl["te"], **ip, **nxt)
            for k, src in (("r", "r"), ("t", "t"), ("te", "te"), ("n", "n"), ("log", "log"), ("idx", "idx"), ("lar", "lar"),
                           ("act", "a")):
                logs[k].append(st[src].clone())
            if parent.final_obs is not None:
                logs["final"].append(parent.final_obs.clone())
        out = {k: torch.stack(v).cpu().numpy() for k, v in logs.items() if v}
        out["final"] = out["final"].reshape(S, -1, FB) if "final" in out else None
        outs.append(out)
    return outs


def _check_against_trace(got, tr, env, what):
    """The store's flags, rewards and final-observation slots against the host trace; the ring's r_terminal at every step."""
    S, n = tr["actions"].shape
    np.testing.assert_array_equal(got["act"], tr["actions"], err_msg=what)          # (the fused form drew the script)
    np.testing.assert_array_equal(got["t"], tr["flags"], err_msg=what + ": out_terminal")
    np.testing.assert_array_equal(got["te"], tr["flags"], err_msg=what + ": terminal_end")
    np.testing.assert_array_equal(got["r"], tr["rewards"], err_msg=what + ": rewards")
    assert (got["n"] == 1).all() and (got["log"] == 1).all()
    ring = env.ring
    np.testing.assert_array_equal(ring.count.cpu().numpy(), np.full(n, S), err_msg=what)      # (no two ends in a row)
    r_term = ring.r_terminal.view(n, ring.H1)[:, :S].cpu().numpy()
    np.testing.assert_array_equal(r_term.T, tr["flags"], err_msg=what + ": r_terminal")
    # slot b holds the last observation the limit cut off for actor b, byte for byte; the sentinel until then
    want = np.full((n, FB), SENTINEL, np.uint8)
    for s in range(S):
        for b in range(n):
            if (s, b) in tr["final"]:
                want[b] = tr["final"][(s, b)].reshape(-1)
        bad = np.flatnonzero((got["final"][s] != want).any(1))
        assert not len(bad), "%s step %d: final-observation slots of actors %s differ" % (what, s, bad)
    assert (tr["flags"] == 2).any(), what


def _check_against_plain(got, plain, env, env_plain, what, extra=()):
    """Everything but the three flag words is what the existing entry writes on the same inputs; without the store the
    flags are 0 / 1."""
    assert set(np.unique(plain["t"])) <= {0, 1} and set(np.unique(plain["te"])) <= {0, 1}
    np.testing.assert_array_equal(np.minimum(got["t"], 1), plain["t"], err_msg=what)
    np.testing.assert_array_equal(np.minimum(got["te"], 1), plain["te"], err_msg=what)
    for k in ("r", "n", "log", "idx", "lar", "act"):
        np.testing.assert_array_equal(got[k], plain[k], err_msg="%s: %s" % (what, k))
    a, b = env.ring, env_plain.ring
    n = a.B * a.H1
    assert torch.equal(a.frames[:n * FB], b.frames), what + ": frames"
    assert torch.equal(a.r_terminal.clamp(max=1), b.r_terminal) and int(b.r_terminal.max()) == 1, what
    for name in RING + tuple(extra):
        assert torch.equal(getattr(a, name), getattr(b, name)), "%s: %s" % (what, name)
    rec_a, rec_b = a.actor_records, b.actor_records
    assert rec_a is None and rec_b is None or torch.equal(rec_a, rec_b), what + ": records"


# ---- 1. the step kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["rollout", "policy"])
@pytest.mark.parametrize("k", range(len(TC.ARCADE_CASES)), ids=TC.ARCADE_NAMES)
def test_arcade_steps_flag_truncations_and_keep_their_final_observation(k, fused):
    conf, tr = TC.arcade_trace(k)
    env, plain = _arcade_env(conf, TC.B, True), _arcade_env(conf, TC.B, False)
    got, ref = _drive([env, plain], tr["actions"], fused)
    what = "%s %s" % (TC.ARCADE_NAMES[k], "policy" if fused else "rollout")
    _check_against_trace(got, tr, env, what)
    _check_against_plain(got, ref, env, plain, what, extra=("arcade",))


@pytest.mark.parametrize("fused", [False, True], ids=["rollout", "policy"])
@pytest.mark.parametrize("k", range(len(TC.MAZE_CASES)), ids=TC.MAZE_NAMES)
def test_maze_steps_flag_truncations_and_keep_their_final_observation(k, fused):
    conf, tr = TC.maze_trace(k)
    env, plain = _maze_env(conf, TC.B, True), _maze_env(conf, TC.B, False)
    got, ref = _drive([env, plain], tr["actions"], fused)
    what = "%s %s" % (TC.MAZE_NAMES[k], "policy" if fused else "rollout")
    _check_against_trace(got, tr, env, what)
    _check_against_plain(got, ref, env, plain, what, extra=("goal", "layout", "heading"))


def test_the_store_is_refused_out_of_scope():
    from unreal_amd import ops
    from unreal_amd.environment.maze_environment import MazeConfig, batched_maze_environment
    lay = TC.NAV_LAYOUTS[0]
    z = lambda dt=torch.int32: torch.zeros(2, dtype=dt, device=DEV)
    store = torch.zeros(2 * FB, dtype=torch.uint8, device=DEV)
    for conf in (None, MazeConfig([lay.replace("A", "-")], max_episode_steps=5),
                 MazeConfig([lay], goal_sense=True, **TC.NAV_KW)):
        env = batched_maze_environment(2, 3, DEV, config=conf)
        with pytest.raises(ValueError, match="out of scope"):
            ops.maze_rollout_step(env.ring, z(), z(torch.float32), z(), z(), z(), z(), z(), maze=env.maze, final_obs=store)


# ---- 2. group views ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["rollout", "policy"])
@pytest.mark.parametrize("kind,k", [("arcade", 0), ("maze", 0)], ids=["breakout-20", "nav-respawn"])
def test_views_write_the_parents_slots(kind, k, fused):
    """Four actors as two views of two: a truncated actor sits in the second view, so a view that wrote slot b of the
    parent instead of b0 + b, or indexed its own ring, shows."""
    n = 4
    if kind == "arcade":
        conf, tr = TC.arcade_trace(k, n)
        env, whole = _arcade_env(conf, n, True), _arcade_env(conf, n, True)
    else:
        conf, tr = TC.maze_trace(k, n)
        env, whole = _maze_env(conf, n, True), _maze_env(conf, n, True)
    assert (tr["flags"][:, 2:] == 2).any()
    views = [env.view(0, 2), env.view(2, 4)]
    for v, b0 in zip(views, (0, 2)):
        assert v.ring.final_base == env.ring.final_base == n * env.ring.H1
        assert v.ring.final_obs.data_ptr() == env.ring.final_obs.data_ptr() + b0 * FB and v.ring.final_obs.numel() == 2 * FB
        v._parent_ring = env.ring
    got, ref = _drive([views, whole], tr["actions"], fused, parts=[(0, 2), (2, 4)])
    _check_against_trace(got, tr, env, "views")
    for key in ("r", "t", "te", "idx", "lar", "final"):
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    assert torch.equal(env.ring.frames, whole.ring.frames) and torch.equal(env.ring.r_terminal, whole.ring.r_terminal)
    # the next step's frame indices are the parent's
    cnt = np.arange(1, TC.STEPS + 1)[:, None] % env.ring.H1
    np.testing.assert_array_equal(got["idx"], np.arange(n)[None, :] * env.ring.H1 + cnt)


# ---- 3. the scan ---------------------------------------------------------------------------------------------------------------
def _scan_inputs(seed=0):
    rs = np.random.RandomState(seed)
    Bn, T = 5, 6
    return dict(B=Bn, T=T, r=rs.randint(-2, 8, (T, Bn)).astype(np.float32), v=rs.uniform(-3, 3, (T, Bn)).astype(np.float32),
                boot=rs.uniform(-3, 3, Bn).astype(np.float32), n=np.array([1, 3, 6, 6, 3], np.int32),
                te=np.array([2, 1, 0, 2, 0], np.int32))


@pytest.mark.parametrize("lam", [1.0, 0.95, 0.0])
def test_base_returns_tl_is_the_fp64_scan(lam):
    """Within one fp32 ulp of the expected value: the kernel's scan is fp64 and differs from numpy's at most by fused
    multiply-adds before the one rounding to fp32."""
    from unreal_amd import ops
    c = _scan_inputs()
    Bn, T, gamma = c["B"], c["T"], 0.99
    for te in [np.roll(c["te"], k) for k in range(Bn)]:                   # every flag meets every n_steps in {1, 3, 6}
        R, adv = (torch.full((T * Bn,), 9.0, device=DEV) for _ in range(2))
        ops.base_returns_tl(Bn, T, _dev(c["r"], torch.float32).view(-1), _dev(c["v"], torch.float32).view(-1),
                            _dev(c["n"], torch.int32), _dev(c["boot"], torch.float32), _dev(te, torch.int32), gamma, lam, R, adv)
        wR, wadv = TC.gae_scan(c["r"], c["v"], c["n"], c["boot"], te, gamma, lam)
        for got, want, name in ((R, wR, "R"), (adv, wadv, "adv")):
            got = got.cpu().numpy().reshape(T, Bn).astype(np.float64)
            err, bound = np.abs(got - want), TC.ulp32(want)
            print("lambda %g %s: max error %.3g ulp" % (lam, name, (err / bound).max()))
            assert (err <= bound).all(), (lam, name, (err / bound).max())
            for b in range(Bn):
                assert (got[c["n"][b]:, b] == 0).all()
    seen = {(int(n), int(f)) for k in range(Bn) for n, f in zip(c["n"], np.roll(c["te"], k))}
    assert seen == {(n, f) for n in (1, 3, 6) for f in (0, 1, 2)}


def test_base_returns_tl_at_lambda_one_is_base_returns():
    from unreal_amd import ops
    c = _scan_inputs(1)
    Bn, T = c["B"], c["T"]
    te = np.array([1, 1, 0, 0, 1], np.int32)                                # no flag 2: the existing kernel's cases
    args = (Bn, T, _dev(c["r"], torch.float32).view(-1), _dev(c["v"], torch.float32).view(-1), _dev(c["n"], torch.int32),
            _dev(c["boot"], torch.float32), _dev(te, torch.int32), 0.99)
    out = [torch.zeros(T * Bn, device=DEV) for _ in range(4)]
    ops.base_returns(*args, out[0], out[1])
    ops.base_returns_tl(*args, 1.0, out[2], out[3])
    for old, new in ((out[0], out[2]), (out[1], out[3])):
        old, new = old.cpu().numpy().astype(np.float64), new.cpu().numpy().astype(np.float64)
        assert (np.abs(new - old) <= TC.ulp32(old)).all()
    with pytest.raises(ValueError):
        ops.base_returns_tl(*args, 1.5, out[2], out[3])


# ---- 4. the gather -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lstm", [True, False])
def test_boot_gather_is_exact(lstm):
    from unreal_amd import ops
    Bn, T, Hn, base, parent = 5, 4, 6, 3, 11               # a group of five whose first actor is actor 3 of eleven
    ring = ops.Ring(parent, Hn, torch.device(DEV), arcade=True, final_obs=True)
    view = ops.ring_view(ring, base, base + Bn)
    rs = np.random.RandomState(5)
    te = np.array([2, 0, 1, 2, 2], np.int32)
    n = np.array([1, T, 2, T, 3], np.int32)               # a truncation at rollout step 0 and one at the last step
    count = rs.randint(0, 50, Bn).astype(np.int32)
    la, lr = rs.randint(0, A, Bn).astype(np.int32), rs.randint(-3, 9, Bn).astype(np.float32)
    acts, rews = rs.randint(0, A, (T, Bn)).astype(np.int32), rs.randint(-3, 9, (T, Bn)).astype(np.float32)
    view.count.copy_(_dev(count, torch.int32)); view.last_action.copy_(_dev(la, torch.int32))
    view.last_reward.copy_(_dev(lr, torch.float32))
    f = lambda *s: rs.uniform(-1, 1, s).astype(np.float32)
    cc, ch, wc, wh = f(Bn, 256), f(Bn, 256), f(T, Bn, 256), f(T, Bn, 256)
    idx = torch.full((Bn,), -1, dtype=torch.int32, device=DEV)
    c0, h0 = torch.full((Bn * 256,), 7.0, device=DEV), torch.full((Bn * 256,), 7.0, device=DEV)
    xcat = torch.full((Bn * XLD,), 7.0, device=DEV)
    d = lambda a: _dev(a, torch.float32).view(-1)
    kw = dict(carried_c=d(cc), carried_h=d(ch), ws_c=d(wc), ws_h=d(wh), c0=c0, h0=h0, xcat=xcat, ld=XLD, col0=256) if lstm else {}
    ops.boot_gather(view, T, A, _dev(te, torch.int32), _dev(n, torch.int32), _dev(acts, torch.int32).view(-1), d(rews), idx,
                    base_actor=base, **kw)
    cut = te == 2
    want_idx = np.where(cut, parent * (Hn + 1) + base + np.arange(Bn), (base + np.arange(Bn)) * (Hn + 1) + count % (Hn + 1))
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    assert want_idx.max() < ring.frames.numel() // FB
    if not lstm:
        assert (c0 == 7).all() and (xcat == 7).all()
        return
    rows = n - 1
    np.testing.assert_array_equal(c0.cpu().numpy().reshape(Bn, 256), np.where(cut[:, None], wc[rows, np.arange(Bn)], cc))
    np.testing.assert_array_equal(h0.cpu().numpy().reshape(Bn, 256), np.where(cut[:, None], wh[rows, np.arange(Bn)], ch))
    x = xcat.cpu().numpy().reshape(Bn, XLD)
    want_a = np.where(cut, acts[rows, np.arange(Bn)], la)
    np.testing.assert_array_equal(x[:, 256:256 + A], np.eye(A, dtype=np.float32)[want_a])
    np.testing.assert_array_equal(x[:, 256 + A], np.where(cut, rews[rows, np.arange(Bn)], lr))
    assert (x[:, :256] == 7).all() and (x[:, 256 + A + 1:] == 7).all()
    with pytest.raises(ValueError, match="final-observation"):
        ops.boot_gather(ops.Ring(Bn, Hn, torch.device(DEV)), T, A, _dev(te, torch.int32), _dev(n, torch.int32),
                        _dev(acts, torch.int32).view(-1), d(rews), idx)


# ---- 5. the trainer --------------------------------------------------------------------------------------------------------------
def _trainer(env_type, env_name, Bn, T, Hn, groups=1, fuse=True, **options):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    cfg = _cfg(True, False, Hn, T)
    Environment.action_size = -1
    net = UnrealModel(Environment.get_action_size(env_type, env_name), 0, -1, True, False, False, False, 0.05, 0.001, DEV, seed=4)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    tr = Trainer(0, net, 7.0711e-4, None, applier, env_type, env_name, True, False, False, False, 0.05, 0.001, T, T,
                 cfg["gamma"], cfg["gamma_pc"], Hn, 10 ** 6, DEV, batch_size=Bn, groups=groups, seed=TC.SEED, **options)
    tr.fuse_policy_env = fuse
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    return net, applier, tr


def _independent_value(net, tr, b, frame_index, row):
    """V of the network on frame `frame_index` of the whole ring, from the LSTM state of workspace row `row` and that
    row's action and reward: a one-row workspace through encode_rows / lstm_step / value_forward, none of which this
    option touches."""
    from unreal_amd.model.model import PathWS
    ws1 = PathWS(1, 1, DEV, save_c1=False, lstm=True, xld=net.xld, **net.ws_kw)
    ws1.frame_idx[0] = int(frame_index)
    last = type("Last", (), {})()
    last.last_action, last.last_reward = tr.actions[row:row + 1].clone(), tr.rewards[row:row + 1].clone()
    ws1.c0.copy_(tr.base_ws.c[row * 256:(row + 1) * 256]); ws1.h0.copy_(tr.base_ws.h[row * 256:(row + 1) * 256])
    net.begin_pass()
    net.encode_rows(tr.full_ring, ws1, 0, 1, lar_from_ring=False, save_c1=False, actor_ring=last, lstm_x=False)
    net.lstm_step(ws1, 0, 1, fused_x=True)
    feat, ld = net.features(ws1)
    v = torch.zeros(1, device=DEV)
    net.value_forward(1, feat, ld, v)
    return float(v.cpu()[0])


def _breakout(name):
    from unreal_amd.environment.environment import Environment
    Environment.register_arcade_config(name, **dict(TC.BREAKOUT, max_episode_steps=20))
    return Environment.ARCADE_CONFIG[name]


@pytest.mark.parametrize("groups,fuse", [(1, True), (1, False), (2, True), (2, False)])
def test_trainer_bootstraps_truncated_actors(groups, fuse):
    from unreal_amd.environment.environment import Environment
    name = "tl_breakout_%d%d" % (groups, fuse)
    conf = _breakout(name)
    try:
        Bn, T, Hn = 4, 5, 12
        net, applier, tr = _trainer("arcade", name, Bn, T, Hn, groups, fuse, bootstrap_timeouts=True)
        assert tr.full_ring.final_obs is not None and tr.Bg == Bn // groups and tr._split is None
        # the fill has just reset every actor: the host models start the same episodes
        models = TC.arcade_models(conf, Bn, seed=tr.seed)
        for m, e in zip(models, tr.full_ring.episode.cpu().numpy()):
            m.episode = int(e) - 1
            m.reset()
        np.testing.assert_array_equal(tr.full_environment.current_records()[:, :10], [m.record()[:10] for m in models])
        tr.full_ring.final_obs.fill_(SENTINEL)
        Bg, seen = tr.Bg, set()
        for it in range(30):
            for g in range(groups):
                tr._select_group(g)
                tr.compute_gradients()
                b0 = g * Bg
                n, te = tr.n_steps.cpu().numpy(), tr.terminal_end.cpu().numpy()
                acts, rews = tr.actions.cpu().numpy().reshape(T, Bg), tr.rewards.cpu().numpy().reshape(T, Bg)
                vals, boot = tr.v.cpu().numpy().reshape(T, Bg), tr.boot_v.cpu().numpy()
                final = tr.full_ring.final_obs.view(Bn, FB).cpu().numpy()
                for b in range(Bg):
                    m, flag = models[b0 + b], 0
                    for t in range(n[b]):
                        assert flag == 0                                   # the rollout stopped at the first end
                        _, r, term, _ = m.process(acts[t, b])
                        assert r == rews[t, b]
                        flag = TC.arcade_flag(m, term)
                    assert te[b] == flag and (flag != 0 or n[b] == T), (it, g, b, te[b], flag)
                    seen.add(flag)
                    if flag == 2:
                        np.testing.assert_array_equal(final[b0 + b], m.frame.reshape(-1))
                        row = (n[b] - 1) * Bg + b
                        want = _independent_value(net, tr, b, tr.full_ring.final_base + b0 + b, row)
                        assert abs(boot[b] - want) <= 1e-5 + 1e-5 * abs(want), (it, g, b, boot[b], want)
                    if flag:
                        m.reset()
                wR, wadv = TC.gae_scan(rews, vals, n, boot, te, tr.gamma, 1.0)
                for got, want in ((tr.R, wR), (tr.adv, wadv)):
                    got = got.cpu().numpy().reshape(T, Bg).astype(np.float64)
                    assert (np.abs(got - want) <= TC.ulp32(want)).all(), (it, g, n, te, np.abs(got - want).max())
                state = torch.stack([tr.lstm_c.view(Bg, 256), tr.lstm_h.view(Bg, 256)])
                assert (state[:, te != 0] == 0).all()              # reset_state: flag 1 and flag 2 alike
                if (te == 0).any():
                    assert (state[:, te == 0] != 0).any()
                tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, tr._anneal_learning_rate(0))
                net.mark_params_changed()
            if seen == {0, 1, 2} and it >= 3:
                break
        assert seen == {0, 1, 2}, seen
        np.testing.assert_array_equal(tr.full_environment.current_records()[:, :10], [m.record()[:10] for m in models])
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_trainer_without_the_option_ends_every_episode_alike():
    """The same trainer with the flag off: a time-out is flag 1, its return starts from 0, nothing is allocated."""
    from unreal_amd.environment.environment import Environment
    name = "tl_breakout_off"
    conf = _breakout(name)
    try:
        Bn, T = 4, 5
        net, applier, tr = _trainer("arcade", name, Bn, T, 12)
        assert tr.full_ring.final_obs is None and tr.bootstrap_timeouts is False and tr.gae_lambda is None
        models = TC.arcade_models(conf, Bn, seed=tr.seed)
        for m, e in zip(models, tr.full_ring.episode.cpu().numpy()):
            m.episode = int(e) - 1
            m.reset()
        cuts = 0
        for it in range(30):
            if cuts and it >= 3:
                break
            tr.compute_gradients()
            n, te = tr.n_steps.cpu().numpy(), tr.terminal_end.cpu().numpy()
            acts, rews = tr.actions.cpu().numpy().reshape(T, Bn), tr.rewards.cpu().numpy().reshape(T, Bn)
            R = tr.R.cpu().numpy().reshape(T, Bn)
            assert set(te) <= {0, 1}
            for b, m in enumerate(models):
                for t in range(n[b]):
                    _, _, term, _ = m.process(acts[t, b])
                assert te[b] == int(term)
                if term:
                    cuts += "end_timeout" in m.events
                    assert R[n[b] - 1, b] == rews[n[b] - 1, b]
                    m.reset()
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, tr._anneal_learning_rate(0))
            net.mark_params_changed()
        assert cuts > 0
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_trainer_with_gae_on_the_reference_maze():
    """gae_lambda = 0.95 with the flag off, on the reference's maze: R and adv are the scan of the logged rollout."""
    Bn, T = 4, 5
    net, applier, tr = _trainer("maze", "", Bn, T, 12, gae_lambda=0.95)
    assert tr.full_ring.final_obs is None and tr.gae_lambda == 0.95
    for it in range(4):
        tr.compute_gradients()
        n, te = tr.n_steps.cpu().numpy(), tr.terminal_end.cpu().numpy()
        assert set(te) <= {0, 1}
        rews, vals = tr.rewards.cpu().numpy().reshape(T, Bn), tr.v.cpu().numpy().reshape(T, Bn)
        wR, wadv = TC.gae_scan(rews, vals, n, tr.boot_v.cpu().numpy(), te, tr.gamma, 0.95)
        for got, want in ((tr.R, wR), (tr.adv, wadv)):
            got = got.cpu().numpy().reshape(T, Bn).astype(np.float64)
            assert (np.abs(got - want) <= TC.ulp32(want)).all(), it
        nR, _ = TC.gae_scan(rews, vals, n, tr.boot_v.cpu().numpy(), te, tr.gamma, 1.0)
        assert np.abs(nR - wR).max() > 1e-4                  # (and it is not the n-step return)
        tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, tr._anneal_learning_rate(0))
        net.mark_params_changed()
