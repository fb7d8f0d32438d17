"""Depth prediction for first-person mazes on the device: unreal_maze_depth_labels byte for byte against the
host model of tests/depth_model.py, unreal_depth_loss_grad and the head's products against fp64, and the trainer's pass
rebuilt in fp64 from its own buffers."""
import numpy as np
import pytest
import torch

try:
    import depth_model as DM
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import depth_model as DM
    from tests import maze_model as MM
from oracle import model as OM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB = 21168
SENTINEL = 0xEE
LOSS_RTOL = 1e-4                      # the project's loss bar (tests/test_trainer_gpu.py)
GRAD_REL = 2e-5                       # of the variable's largest |gradient|
FWD_ATOL, FWD_RTOL = 1e-5, 1e-5       # the project's forward bar (tests/test_kernels_gpu.py)


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


# ---- 1. labels ---------------------------------------------------------------------------------------------------------------
def _static(N, seed, L=3, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed)
    return MazeConfig([MM.random_layout(N, rs, marks="") for _ in range(L)], view="first_person", random_start=True,
                      random_goal=True, max_episode_steps=7, **kw)


def _forage(N, seed):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed)
    return MazeConfig([MM.random_layout(N, rs, marks="AABBC") for _ in range(2)], view="first_person", random_start=True,
                      random_goal=True, max_episode_steps=9, pickups=[(2, (250, 20, 20), False), (-1, (20, 20, 250), True)],
                      wall_styles=None)


def _generated(N, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    return MazeConfig(view="first_person", generate=N, random_start=True, random_goal=True, max_episode_steps=6,
                      gen_loops=2, gen_apples=3, **kw)


CONFIGS = {
    "static7": lambda: _static(7, 1),
    "static21": lambda: _static(21, 2),
    "generated12": lambda: _generated(12),
    "generated14_styled": lambda: _generated(14, wall_styles=[(200, 30, 30, 0x33)], gen_landmark_density=64),
    "forage14": lambda: _forage(14, 3),
    "sense12": lambda: _static(12, 4, goal_sense=True, progress_reward=1),
    "nav7_lab": lambda: _static(7, 5, action_set="lab", goal_reward=10),
}


def _env(conf, B, H=3, seed=5):
    from unreal_amd.environment.maze_environment import batched_maze_environment
    env = batched_maze_environment(B, H, DEV, config=conf, seed=seed, depth_labels=True)
    assert env.depth_labels and env.ring.r_depth.numel() == B * (H + 1) * 12 and env.ring.r_depth.dtype == torch.uint8
    return env


def _host_labels(env):
    """[B, 12] labels of the actors' current views by the host model, from the device's own cell, heading and walls."""
    ring, conf = env.ring, env.config
    N, B = conf.N, ring.B
    pos = ring.pos.cpu().numpy().reshape(B, 2)
    head = ring.heading.cpu().numpy()
    if conf.generate is not None:
        walls = env.current_layouts()[0].reshape(B, N * N)
    else:
        walls = np.stack(conf.walls)[ring.layout.cpu().numpy()]
    return np.stack([DM.labels(walls[b], N, int(pos[b, 0]), int(pos[b, 1]), int(head[b]) & 3) for b in range(B)])


class _Book(object):
    """The expected r_depth of a ring: the sentinel everywhere but the slots the label launch has written."""

    def __init__(self, env):
        self.env, ring = env, env.ring
        self.want = np.full((ring.B, ring.H1, 12), SENTINEL, dtype=np.uint8)
        self.classes = set()

    def start(self):
        """After the constructor's reset: wipe the array, reset again (no slot moves), expect the current slot alone."""
        self.env.ring.r_depth.fill_(SENTINEL)
        self.env.reset()
        self.check("reset")

    def check(self, what):
        ring = self.env.ring
        lab = _host_labels(self.env)
        slot = ring.count.cpu().numpy() % ring.H1
        self.want[np.arange(ring.B), slot] = lab
        self.classes |= set(lab.reshape(-1))
        got = ring.r_depth.cpu().numpy().reshape(ring.B, ring.H1, 12)
        bad = np.argwhere(got != self.want)
        assert not len(bad), "%s: r_depth differs at (actor, slot, position) %s: got %s want %s" % (
            what, bad[:4].tolist(), got[tuple(bad[0])], self.want[tuple(bad[0])])


def _rollout_state(B, A, xld=264):
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=DEV)
    return dict(active=torch.ones(B, dtype=torch.int32, device=DEV), log=z(B), n=z(B), te=z(B), r=z(B, torch.float32),
                t=z(B), a=z(B), pi=z(B * A, torch.float32), v=z(B, torch.float32), idx=z(B),
                lar=torch.zeros(B * xld, device=DEV))


def _step(env, entry, rs, st, A, net, step):
    B = env.ring.B
    st["active"].fill_(1)                 # (a terminal clears it: every actor keeps stepping)
    nxt = dict(next_idx=st["idx"], next_lar=st["lar"], lar_ld=264, lar_col0=256, A=A) if step % 2 else {}
    if env.ring.objective_size and nxt:
        nxt = dict(next_idx=st["idx"])
    if entry == "process":
        st["a"].copy_(_dev(rs.randint(0, A, B).astype(np.int32), torch.int32))
        env.process(st["a"], None, st["r"], st["t"], reset_on_terminal=True, track_score=True)
    elif entry == "rollout":
        st["a"].copy_(_dev(rs.randint(0, A, B).astype(np.int32), torch.int32))
        env.rollout_step(st["a"], st["r"], st["t"], st["active"], st["log"], st["n"], st["te"], **nxt)
    else:
        feat = _dev(rs.uniform(-1, 1, (B, 256)), torch.float32).view(-1)
        u = _dev(rs.uniform(0, 1, B), torch.float64)
        env.policy_rollout_step(net, feat, 256, u, st["pi"], st["v"], st["a"], st["r"], st["t"], st["active"], st["log"],
                                st["n"], st["te"], **nxt)


def _fake_net(A, rs):
    return type("Net", (), {"p": dict(W_base_fc_p=_dev(rs.uniform(-.3, .3, 256 * A), torch.float32),
                                      b_base_fc_p=_dev(rs.uniform(-.1, .1, A), torch.float32),
                                      W_base_fc_v=_dev(rs.uniform(-.3, .3, 256), torch.float32),
                                      b_base_fc_v=_dev(rs.uniform(-.1, .1, 1), torch.float32))})


@pytest.mark.parametrize("name,B", [("static7", 1), ("static7", 17), ("static21", 1), ("static21", 17),
                                    ("generated12", 17), ("generated14_styled", 3), ("forage14", 17), ("sense12", 3),
                                    ("nav7_lab", 17)])
def test_labels_match_the_host_model_in_lock_step(name, B):
    """60 steps, 20 through each of the plain, rollout and policy-fused entries, with a history of 3 so that the ring
    wraps many times: after every launch the whole of r_depth is the host model's labels in the slots the launches wrote
    and the sentinel byte everywhere else.  Episodes end (step limits of 6 to 9) and the label is then that of the new
    episode's first view."""
    conf = CONFIGS[name]()
    env = _env(conf, B)
    A = conf.action_size
    rs = np.random.RandomState(B + conf.N)
    book = _Book(env)
    book.start()
    st, net = _rollout_state(B, A), _fake_net(A, rs)
    for step in range(60):
        entry = ("process", "rollout", "policy")[(step // 4) % 3]
        _step(env, entry, rs, st, A, net, step)
        book.check("%s step %d (%s)" % (name, step, entry))
    assert int(env.ring.episode.max()) >= 3                       # episodes ended on the way
    assert int(env.ring.count.min()) > 2 * env.ring.H1            # ... and the ring wrapped
    if B == 17:
        assert len(book.classes) >= (4 if conf.N == 7 else 5), sorted(book.classes)
    mask = _dev((np.arange(B) % 2 == 0).astype(np.int32), torch.int32)
    env.reset(mask)
    book.check("masked reset")


def test_two_views_write_the_parents_array():
    conf = CONFIGS["static21"]()
    env = _env(conf, 17)
    book = _Book(env)
    book.start()
    cut = 6
    views = [env.view(0, cut), env.view(cut, 17)]
    assert all(v.depth_labels for v in views)
    assert views[1].ring.r_depth.data_ptr() == env.ring.r_depth.data_ptr() + cut * env.ring.H1 * 12
    rs = np.random.RandomState(0)
    sts = [_rollout_state(v.ring.B, 4) for v in views]
    net = _fake_net(4, rs)
    for step in range(12):
        for v, st in zip(views, sts):
            _step(v, ("process", "rollout", "policy")[step % 3], rs, st, 4, net, step)
        book.check("views step %d" % step)
    gconf = CONFIGS["generated12"]()
    genv = _env(gconf, 5)
    gbook = _Book(genv)
    gbook.start()
    gviews = [genv.view(0, 2), genv.view(2, 5)]
    gsts = [_rollout_state(v.ring.B, 4) for v in gviews]
    for step in range(9):
        for v, st in zip(gviews, gsts):
            _step(v, ("process", "rollout", "policy")[step % 3], rs, st, 4, net, step)
        gbook.check("generated views step %d" % step)


def test_wrong_block_writes_nothing_and_ops_refuses():
    """A launch whose N is not the block's, or whose layout argument does not fit the block's kind, writes nothing."""
    from unreal_amd import ops, _lib
    from unreal_amd._lib import ptr
    env = _env(CONFIGS["static7"](), 4)
    ring = env.ring
    ring.r_depth.fill_(SENTINEL)
    L = _lib.lib()
    view, N, block = env.maze[:3]
    for n, layout, words in ((12, ring.layout, 0), (7, None, 8 + 18 + 49 + 65)):
        L.call("unreal_maze_depth_labels", 4, ring.H1, n, ptr(ring.count), ptr(ring.pos), ptr(ring.heading), words,
               ptr(block), ptr(layout), ptr(ring.r_depth), None)
    torch.cuda.synchronize()
    assert (ring.r_depth == SENTINEL).all()
    from unreal_amd.environment.maze_environment import batched_maze_environment, MazeConfig, REFERENCE_MAP
    plain = batched_maze_environment(2, 2, DEV, config=MazeConfig([REFERENCE_MAP], view="first_person"))
    assert plain.ring.r_depth is None and not plain.depth_labels
    with pytest.raises(ValueError, match="depth"):
        ops.maze_depth_labels(plain.ring, plain.maze)             # a ring without the array
    with pytest.raises(ValueError, match="first_person"):
        batched_maze_environment(2, 2, DEV, config=MazeConfig([REFERENCE_MAP]), depth_labels=True)


# ---- 2. the loss kernel ------------------------------------------------------------------------------------------------------------
def _loss_case(rows, seed):
    rs = np.random.RandomState(seed)
    ld, frames = 104, rows + 3
    logits = rs.normal(0, 3, (rows, ld)).astype(np.float32)
    big = rs.uniform(size=(rows, 12)) < 0.3                       # groups of magnitude 80: a plain softmax overflows
    big[0, 3] = True
    z = logits[:, :96].reshape(rows, 12, 8)
    z[big] = np.sign(z[big]) * 80 + z[big] * 0.01
    labels = rs.randint(0, 8, (frames, 12)).astype(np.uint8)
    labels[:, 0] = np.arange(frames) % 8                          # every class, whatever the draw
    frame_idx = rs.permutation(frames)[:rows].astype(np.int32)
    active = (rs.uniform(size=rows) < 0.7).astype(np.int32)
    active[0] = 1
    if rows > 1:
        active[1] = 0
    # constructed ties on active row 0: positions 1 and 2 have two equal maxima at classes 2 and 5
    z[0, 1] = [0, 1, 4, -1, 2, 4, 0, 3]
    z[0, 2] = [0, 1, 4, -1, 2, 4, 0, 3]
    labels[frame_idx[0], 1] = 2                                   # the lowest index wins: a hit
    labels[frame_idx[0], 2] = 5                                   # ... and the higher one is a miss
    logits[:, :96] = z.reshape(rows, 96)
    return logits, ld, labels, frame_idx, active


@pytest.mark.parametrize("rows", [1, 5, 257])
def test_loss_kernel_against_fp64(rows):
    from unreal_amd import ops
    logits, ld, labels, frame_idx, active = _loss_case(rows, rows)
    scale = 0.37
    zt = torch.tensor(logits[:, :96].astype(np.float64).reshape(rows, 12, 8), requires_grad=True)
    lab = torch.tensor(labels[frame_idx].astype(np.int64))
    logp = torch.log_softmax(zt, dim=2)
    nll = -logp.gather(2, lab[:, :, None])[:, :, 0]
    m = torch.tensor(active.astype(np.float64))[:, None]
    want_loss = scale * (nll * m).sum()
    want_loss.backward()
    want_d = zt.grad.numpy().reshape(rows, 96)
    arg = logits[:, :96].reshape(rows, 12, 8).argmax(2)           # numpy: the first maximum
    on = active.astype(bool)
    want_hits = [int((arg == labels[frame_idx])[on].sum()), int(on.sum()) * 12]
    assert arg[0, 1] == 2 and arg[0, 2] == 2 and labels[frame_idx[0], 2] == 5
    assert np.abs(logits[:, :96]).max() > 79
    if rows == 257:
        assert set(labels[frame_idx][on].reshape(-1)) == set(range(8)) and 0 < on.sum() < rows

    d_logits, d_lab = _dev(logits.reshape(-1), torch.float32), _dev(labels.reshape(-1), torch.uint8)
    d_idx, d_act = _dev(frame_idx, torch.int32), _dev(active, torch.int32)
    dl = torch.full((rows * 96,), 7.0, device=DEV)
    loss = torch.full((1,), 0.5, device=DEV)                      # the kernel adds to what is there
    hits = _dev(np.array([3, 7], np.int32), torch.int32)
    ops.depth_loss_grad(rows, d_logits, ld, d_lab, d_idx, d_act, scale, dl, loss, hits)
    got_loss = float(loss.cpu()[0]) - 0.5
    got_d = dl.cpu().numpy().reshape(rows, 96).astype(np.float64)
    print("depth_loss_grad rows=%d: loss %.9g want %.9g rel %.3g; max |d dlogits| %.3g" % (
        rows, got_loss, float(want_loss), abs(got_loss - float(want_loss)) / abs(float(want_loss)),
        np.abs(got_d - want_d).max()))
    assert abs(got_loss - float(want_loss)) <= LOSS_RTOL * abs(float(want_loss))
    assert (np.abs(got_d - want_d) <= 1e-5 + 1e-5 * np.abs(want_d)).all()
    assert (got_d[~on] == 0).all() and np.isfinite(got_d).all()
    assert (hits.cpu().numpy() - [3, 7]).tolist() == want_hits
    # forward only: the same loss and hits, and no gradient is written anywhere
    loss2 = torch.zeros(1, device=DEV)
    hits2 = torch.zeros(2, dtype=torch.int32, device=DEV)
    dl.fill_(7.0)
    ops.depth_loss_grad(rows, d_logits, ld, d_lab, d_idx, d_act, scale, None, loss2, hits2)
    assert abs(float(loss2.cpu()[0]) - float(want_loss)) <= LOSS_RTOL * abs(float(want_loss))
    assert hits2.cpu().numpy().tolist() == want_hits and (dl == 7.0).all()


# ---- 3. the head's products at N = 96 ---------------------------------------------------------------------------------------------
def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) - (FWD_ATOL + FWD_RTOL * np.abs(want))
    print("%s: max |d| %.3g (max |want| %.3g)" % (what, np.abs(got - want).max(), np.abs(want).max()))
    assert (err <= 0).all(), (what, float(err.max()))


@pytest.mark.parametrize("rows", [5, 300])
@pytest.mark.parametrize("K", [256, 128])
def test_gemm_entry_at_n_96(rows, K):
    """unreal_gemm_f32 at N = 96 (a 64-wide tile and a half-empty one), the three orientations the head uses."""
    from unreal_amd import ops
    rs = np.random.RandomState(rows + K)
    X = rs.uniform(-1, 1, (rows, K + 8)).astype(np.float32)              # a row stride beyond K
    W = rs.uniform(-1, 1, (K, 96)).astype(np.float32) / np.sqrt(K)
    b = rs.uniform(-1, 1, 96).astype(np.float32)
    dO = rs.uniform(-.1, .1, (rows, 96)).astype(np.float32)
    dX, dW, dO_ = _dev(X, torch.float32).view(-1), _dev(W, torch.float32).view(-1), _dev(dO, torch.float32).view(-1)
    Xd, Wd = X[:, :K].astype(np.float64), W.astype(np.float64)
    out = torch.full((rows * 96,), 9.0, device=DEV)
    ops.gemm(False, False, rows, 96, K, dX, K + 8, dW, 96, out, 96, bias=_dev(b, torch.float32))
    _close(out.cpu().numpy().reshape(rows, 96), Xd @ Wd + b, "forward rows=%d K=%d" % (rows, K))
    out.fill_(9.0)
    ops.gemm(False, False, rows, 96, K, dX, K + 8, dW, 96, out, 96, bias=_dev(b, torch.float32), flags=ops.GEMM_RELU)
    _close(out.cpu().numpy().reshape(rows, 96), np.maximum(Xd @ Wd + b, 0), "forward + relu rows=%d K=%d" % (rows, K))
    # dgrad: [rows, 96] @ W^T, added into what is there
    base = rs.uniform(-1, 1, (rows, K)).astype(np.float32)
    dx = _dev(base, torch.float32).view(-1)
    ops.gemm(False, True, rows, K, 96, dO_, 96, dW, 96, dx, K, flags=ops.GEMM_ACCUM)
    _close(dx.cpu().numpy().reshape(rows, K), base + dO.astype(np.float64) @ Wd.T, "dgrad rows=%d K=%d" % (rows, K))
    # wgrad: X^T @ dO, split-K atomics into a zeroed gradient
    gW = torch.zeros(K * 96, device=DEV)
    ops.gemm(True, False, K, 96, rows, dX, K + 8, dO_, 96, gW, 96, flags=ops.GEMM_ATOMIC, splitk=4)
    _close(gW.cpu().numpy().reshape(K, 96), Xd.T @ dO.astype(np.float64), "wgrad rows=%d K=%d" % (rows, K))


@pytest.mark.parametrize("rows", [5, 300])
def test_head_forward_and_backward_against_fp64(rows):
    from unreal_amd.model.model import UnrealModel
    net = UnrealModel(4, 0, -1, False, False, False, False, 0.05, 0.001, DEV, seed=3, use_depth_prediction=True)
    assert [n for n, _, _ in net.spec][-4:] == ["W_dp_fc1", "b_dp_fc1", "W_dp_fc2", "b_dp_fc2"]
    rs = np.random.RandomState(rows)
    ld = 264
    feat = rs.uniform(0, 1, (rows, ld)).astype(np.float32)
    dlog = rs.uniform(-.1, .1, (rows, 96)).astype(np.float32)
    d0 = rs.uniform(-1, 1, (rows, 256)).astype(np.float32)
    f = lambda n: torch.zeros(n, device=DEV)
    hidden, logits, d_hidden = f(rows * 128), f(rows * 96), f(rows * 128)
    d_feat = _dev(d0, torch.float32).view(-1)
    dfeat_in, dlog_in = _dev(feat, torch.float32).view(-1), _dev(dlog, torch.float32).view(-1)
    net.grads.flat.zero_()
    net.depth_head_forward(rows, dfeat_in, ld, hidden, logits)
    net.depth_head_backward(rows, dfeat_in, ld, hidden, dlog_in, d_hidden, d_feat, 256)
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in net.export_named().items()
         if k.endswith("_dp_fc1") or k.endswith("_dp_fc2")}
    x = torch.tensor(feat[:, :256].astype(np.float64), requires_grad=True)
    h = torch.relu(x @ p["W_dp_fc1"] + p["b_dp_fc1"])
    z = h @ p["W_dp_fc2"] + p["b_dp_fc2"]
    (z * torch.tensor(dlog.astype(np.float64))).sum().backward()
    _close(hidden.cpu().numpy().reshape(rows, 128), h.detach().numpy(), "hidden")
    _close(logits.cpu().numpy().reshape(rows, 96), z.detach().numpy(), "logits")
    _close(d_feat.cpu().numpy().reshape(rows, 256), d0 + x.grad.numpy(), "d_feat (accumulated)")
    for k, v in p.items():
        _close(net.grads.shaped(k).cpu().numpy(), v.grad.numpy(), "g[%s]" % k)


# ---- 4. the trainer ----------------------------------------------------------------------------------------------------------------
ENV_NAME = "depth_gpu_fp7"


@pytest.fixture
def fp7():
    from unreal_amd.environment.environment import Environment
    rs = np.random.RandomState(7)
    Environment.register_maze_config(ENV_NAME, [MM.random_layout(7, rs, marks="") for _ in range(2)], view="first_person",
                                     random_start=True, random_goal=True, max_episode_steps=3)
    yield Environment.MAZE_CONFIG[ENV_NAME]
    Environment.MAZE_CONFIG.pop(ENV_NAME, None)


def _trainer(Bn, T, Hn, lstm, aux, groups=1, lam=0.7, **options):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    net = UnrealModel(4, 0, -1, lstm, aux, aux, aux, 0.05, 0.001, DEV, seed=4, use_depth_prediction=True)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    tr = Trainer(0, net, 7.0711e-4, None, applier, "maze", ENV_NAME, lstm, aux, aux, aux, 0.05, 0.001, T, T, 0.99, 0.9, Hn,
                 10 ** 6, DEV, batch_size=Bn, groups=groups, seed=21, use_depth_prediction=True, depth_lambda=lam,
                 **options)
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    return net, applier, tr


def _rebuild(net, tr, T, lstm, lam):
    """The base pass of the selected group in fp64 from the trainer's buffers -> (depth loss, {name: mean gradient})."""
    Bg, A, ws, ring = tr.Bg, 4, tr.base_ws, tr.ring
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in net.export_named().items()}
    idx = ws.frame_idx[:T * Bg].cpu().numpy().astype(np.int64)
    frames = ring.frames[:ring.B * ring.H1 * FB].view(-1, FB).cpu().numpy()[idx].reshape(T, Bg, 84, 84, 3)
    labels = ring.r_depth.view(-1, 12).cpu().numpy()[idx].reshape(T, Bg, 12)
    assert labels.max() < 8                                       # every slot the rollout read carries labels
    xcat = ws.xcat[:T * Bg * ws.xld].view(T, Bg, ws.xld).cpu().numpy().astype(np.float64)
    acts = tr.actions.cpu().numpy().reshape(T, Bg)
    adv = tr.adv.cpu().numpy().reshape(T, Bg).astype(np.float64)
    R = tr.R.cpu().numpy().reshape(T, Bg).astype(np.float64)
    on = tr.active_log.cpu().numpy().reshape(T, Bg).astype(bool)
    total, depth = 0.0, 0.0
    for b in range(Bg):
        x = torch.tensor(frames[:, b].astype(np.float64) / 255.0)
        lar = torch.tensor(xcat[:, b, 256:256 + A + 1])
        state = None
        if lstm:
            state = (torch.tensor(ws.c0[b * 256:(b + 1) * 256].cpu().numpy().astype(np.float64)),
                     torch.tensor(ws.h0[b * 256:(b + 1) * 256].cpu().numpy().astype(np.float64)))
        feat, _ = OM.trunk(x, lar, p, lstm, state)
        rows = torch.tensor(np.flatnonzero(on[:, b]))
        feat = feat[rows]
        pi, v = OM.policy_value(feat, p)
        onehot = torch.tensor(np.eye(A)[acts[on[:, b], b]])
        pl, vl, _ = OM.base_loss(pi, v, onehot, torch.tensor(adv[on[:, b], b]), torch.tensor(R[on[:, b], b]), 0.001)
        h = torch.relu(feat @ p["W_dp_fc1"] + p["b_dp_fc1"])
        z = (h @ p["W_dp_fc2"] + p["b_dp_fc2"]).reshape(-1, 12, 8)
        lab = torch.tensor(labels[on[:, b], b].astype(np.int64))
        ce = -torch.log_softmax(z, dim=2).gather(2, lab[:, :, None]).sum()
        total = total + pl + vl + lam * ce
        depth = depth + lam * ce
    (total / Bg).backward()
    return float(depth) / Bg, {k: v.grad.numpy() for k, v in p.items()}, on


@pytest.mark.parametrize("lstm,groups,options", [(True, 1, {}), (False, 1, {}), (True, 2, {}), (False, 2, {}),
                                                 (True, 2, dict(bootstrap_timeouts=True, gae_lambda=0.9))])
def test_trainer_pass_against_fp64(fp7, lstm, groups, options):
    """First-person N = 7 with a step limit of 3, so every actor ends inside the 5-step rollout; the other auxiliary heads
    off.  B = 3 actors (4 with groups = 2, which must divide the batch)."""
    Bn, T, lam = (3 if groups == 1 else 4), 5, 0.7
    net, applier, tr = _trainer(Bn, T, 12, lstm, False, groups, lam, **options)
    assert len(net.spec) == (12 if lstm else 10) + 4 and tr.full_ring.r_depth is not None
    ended = 0
    for it in range(2):
        hits = np.zeros(2, np.int64)
        for g in range(groups):
            tr._select_group(g)
            tr.compute_gradients()
            want_loss, want_g, on = _rebuild(net, tr, T, lstm, lam)
            ended += int((~on).sum())
            got_loss = float(tr.losses.cpu()[6])
            print("lstm=%s groups=%d it=%d g=%d: depth_loss %.9g want %.9g" % (lstm, groups, it, g, got_loss, want_loss))
            assert abs(got_loss - want_loss) <= LOSS_RTOL * abs(want_loss)
            for name, gw in want_g.items():
                gd = net.grads.shaped(name).cpu().numpy().astype(np.float64)
                tol = GRAD_REL * np.abs(gw).max()
                err = np.abs(gd - gw).max()
                print("  g[%s]: max |d| %.3g, bar %.3g (%.3f of it)" % (name, err, tol, err / tol))
                assert err <= tol, (name, err, tol)
            h = tr.dp_hits.cpu().numpy()
            assert h[1] - hits[1] == int(on.sum()) * 12 and 0 <= h[0] - hits[0] <= h[1] - hits[1]
            hits = h.copy()
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, tr._anneal_learning_rate(0))
            net.mark_params_changed()
    assert ended > 0                                              # rows past an episode's end were masked out


def test_full_unreal_run_checkpoint_and_run_depth(fp7, tmp_path):
    from unreal_amd import checkpoint, ops
    from unreal_amd.model.model import UnrealModel, PathWS
    net, applier, tr = _trainer(4, 5, 16, True, True, groups=2, lam=1.0)
    assert len(net.spec) == 24
    for it in range(3):
        steps, _ = tr.process(None, 0)
        l = tr.last_losses
        assert steps > 0 and all(np.isfinite(v) for v in l.values()), l
        assert l["depth_loss"] > 0 and 0.0 <= l["depth_accuracy"] <= 1.0 and net.depth_loss == l["depth_loss"]
        want = l["base_loss"] + l["pc_loss"] + l["vr_loss"] + l["rp_loss"] + l["depth_loss"]
        assert abs(l["total_loss"] - want) <= 1e-6 * abs(want)
    # a checkpoint carries the head
    checkpoint.save(str(tmp_path), net, applier, 123, 4.5)
    other = UnrealModel(4, 0, -1, True, True, True, True, 0.05, 0.001, DEV, seed=99, use_depth_prediction=True)
    assert checkpoint.restore(str(tmp_path), other)[0] == 123
    a, b = net.export_named(), other.export_named()
    assert list(a) == list(b) and len(a) == 24
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    plain = UnrealModel(4, 0, -1, True, True, True, True, 0.05, 0.001, DEV, seed=99)
    with pytest.raises(ValueError, match="different variable list"):
        checkpoint.restore(str(tmp_path), plain)
    with pytest.raises(ValueError, match="depth"):
        plain.run_depth(None, {"image": np.zeros((84, 84, 3))}, np.zeros(5))
    # run_depth against the batched head on the same observation
    ring = tr.full_ring
    slot = int(ring.count.cpu()[0]) % ring.H1
    image = ring.frames[slot * FB:(slot + 1) * FB].cpu().numpy().reshape(84, 84, 3).astype(np.float64) / 255.0
    lar = np.zeros(5, np.float32)
    lar[int(ring.last_action.cpu()[0])] = 1.0
    lar[4] = float(ring.last_reward.cpu()[0])
    net.reset_state()
    got = net.run_depth(None, {"image": image}, lar)
    ws = PathWS(1, 1, DEV, save_c1=False, lstm=True, xld=net.xld, **net.ws_kw)
    ws.frame_idx[0] = slot
    net.refresh_shadows()
    net.begin_pass()
    feat, ld = net.trunk_forward(ring, ws, 1, 1, lar_from_ring=False, save_c1=False)
    hidden, logits = torch.zeros(128, device=DEV), torch.zeros(96, device=DEV)
    net.depth_head_forward(1, feat, ld, hidden, logits)
    z = logits.cpu().numpy().reshape(12, 8)
    assert got.shape == (12,) and got.tolist() == z.argmax(1).tolist()
    assert ((got >= 0) & (got < ops.DEPTH_CLASSES)).all()


def test_option_off_allocates_and_reports_nothing(fp7):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    net = UnrealModel(4, 0, -1, True, False, False, False, 0.05, 0.001, DEV, seed=4)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    args = (0, net, 7.0711e-4, None, applier, "maze", ENV_NAME, True, False, False, False, 0.05, 0.001, 5, 5, 0.99, 0.9, 12,
            10 ** 6, DEV)
    with pytest.raises(ValueError, match="use_depth_prediction"):
        Trainer(*args, batch_size=2, use_depth_prediction=True)          # the network has no head
    tr = Trainer(*args, batch_size=2)
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    tr.process(None, 0)
    assert tr.full_ring.r_depth is None and not hasattr(tr, "dp_logits") and net.depth_loss is None
    assert sorted(tr.last_losses) == sorted(["total_loss", "base_loss", "policy_loss", "value_loss", "entropy", "pc_loss",
                                             "vr_loss", "rp_loss", "grad_norm"])
    assert float(tr.losses.cpu()[6]) == 0.0
