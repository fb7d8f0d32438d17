"""Indoor environments at any frame size H x W (main.py:196 of the reference: image_shape from the MINOS config): the
runtime-size conv encoder (csrc/encoder_hw.hip) against float64 torch conv2d, the frame-size-aware host-fed ingest against
a numpy mirror, and Trainer(env_type='indoor') end to end against the oracle trainer, whose two 2592-wide reshapes
(fc1, rp_head) are replaced by shape-generic ones for these tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu

SHAPES = [(20, 20), (64, 64), (100, 90), (120, 160), (480, 360)]
SENT = 12345.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


def _weights(rs):
    W1 = rs.uniform(-1, 1, (8, 8, 3, 16)) / np.sqrt(192)
    b1 = rs.uniform(-1, 1, 16) / np.sqrt(192)
    W2 = rs.uniform(-1, 1, (4, 4, 16, 32)) / np.sqrt(256)
    b2 = rs.uniform(-1, 1, 32) / np.sqrt(256)
    return [w.astype(np.float32) for w in (W1, b1, W2, b2)]


def _padded(n, fill=SENT, pad=67):
    """fp32 device buffer of n elements followed by `pad` sentinels."""
    t = torch.full((n + pad,), fill, dtype=torch.float32, device=DEV)
    return t


def _frames(rs, N, H, W, stride):
    """A shuffled pool of N + 3 frames, `stride` bytes apart, and the indices of N of them."""
    pool = N + 3
    buf = np.zeros((pool, stride), np.uint8)
    buf[:, :H * W * 3] = rs.randint(0, 256, size=(pool, H * W * 3), dtype=np.uint8)
    idx = rs.permutation(pool)[:N].astype(np.int32)
    return buf, torch.from_numpy(buf.reshape(-1)).to(DEV), torch.from_numpy(idx).to(DEV), idx


def _close_fwd(got, want, what):
    err = np.abs(got - want)
    tol = 1e-5 + 1e-5 * np.abs(want)
    assert (err <= tol).all(), (what, float(err.max()), float(np.abs(want).max()))


def _close_bwd(got, want, what, ref_max=None):
    err = float(np.abs(got - want).max())
    m = float(np.abs(want).max()) if ref_max is None else ref_max
    assert err <= 2e-5 * m, (what, err, m)


def _check_against_fp64(buf, idx, H, W, ws, scale, d2, c1_dev, f2_dev, d1_dev, chunk=48):
    """float64 torch conv2d over chunks of frames: c1, f2 (1e-5 abs + 1e-5 rel) and the conv1 pre-activation gradient
    d1 (2e-5 of its max) chunk by chunk; -> (dW1, db1, dW2, db2) of the whole batch in float64."""
    W1, b1, W2, b2 = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    N = len(idx)
    d1_parts = []
    for a in range(0, N, chunk):
        e = min(N, a + chunk)
        x = torch.from_numpy(buf[idx[a:e], :H * W * 3].reshape(e - a, H, W, 3)).double().mul(scale).permute(0, 3, 1, 2)
        z1 = TF.conv2d(x, W1.permute(3, 2, 0, 1), b1, stride=4)
        z1.retain_grad()
        nc1 = z1[0].numel()
        _close_fwd(c1_dev[a * nc1:e * nc1], torch.relu(z1).detach().permute(0, 2, 3, 1).reshape(-1).numpy(), "c1")
        # the backward runs through the DEVICE's ReLU mask (c1 > 0): a pre-activation within fp32 rounding of 0 may land
        # on either side, and a flipped element would move d1 and dW1 by a whole gradient element
        m = torch.from_numpy(c1_dev[a * nc1:e * nc1] > 0).double().reshape(e - a, *z1.shape[2:], 16).permute(0, 3, 1, 2)
        c1 = z1 * m
        z2 = TF.conv2d(c1, W2.permute(3, 2, 0, 1), b2, stride=2)
        nf2 = z2[0].numel()
        _close_fwd(f2_dev[a * nf2:e * nf2], torch.relu(z2).detach().permute(0, 2, 3, 1).reshape(-1).numpy(), "f2")
        g = torch.from_numpy(d2[a:e]).double().permute(0, 3, 1, 2)
        (z2 * g).sum().backward()
        d1_parts.append((d1_dev[a * nc1:e * nc1], z1.grad.permute(0, 2, 3, 1).reshape(-1).numpy()))
    d1_max = max(float(np.abs(r).max()) for _, r in d1_parts)
    for got, want in d1_parts:
        _close_bwd(got, want, "d1", d1_max)
    return W1.grad.numpy().reshape(-1), b1.grad.numpy(), W2.grad.numpy().reshape(-1), b2.grad.numpy()


@pytest.mark.parametrize("H,W", SHAPES + [(84, 84)])
@pytest.mark.parametrize("N", [1, 7, 1300])
def test_encoder_hw_matches_fp64(ops, H, W, N):
    """Forward (c1, f2, max f2) within 1e-5 abs + 1e-5 rel of float64, backward (dW1, db1, dW2, db2 and the conv1
    pre-activation gradient) within 2e-5 of the largest element, sentinels untouched, two backward launches bit-identical;
    at 84 x 84 also against the product kernels encoder_fwd / encoder_bwd."""
    rs = np.random.RandomState(H * 1000 + W + N)
    h1, w1, h2, w2, F = ops.frame_dims(H, W)
    stride = ops.frame_stride(H, W)
    buf, frames, idx_d, idx = _frames(rs, N, H, W, stride)
    ws = _weights(rs)
    dws = [torch.from_numpy(w.reshape(-1)).to(DEV) for w in ws]
    scale = 1.0 / 255.0
    n1, n2 = N * h1 * w1 * 16, N * F
    c1, f2 = _padded(n1), _padded(n2)
    slot = torch.zeros(1, dtype=torch.float32, device=DEV)
    ops.encoder_hw_fwd(frames, idx_d, (H, W), stride, scale, *dws, c1, f2, f2_max=slot)
    c1_h, f2_h = c1.cpu().numpy(), f2.cpu().numpy()
    assert (c1_h[n1:] == SENT).all() and (f2_h[n2:] == SENT).all()
    assert float(slot.cpu()[0]) == float(f2_h[:n2].max())

    d2 = rs.standard_normal((N, h2, w2, 32)).astype(np.float32)
    d2_d = torch.from_numpy(d2.reshape(-1)).to(DEV)
    nwork = ops.encoder_hw_work_floats(N, (H, W))
    runs = []
    for _ in range(2):
        grads = [torch.full((n + 33,), SENT, dtype=torch.float32, device=DEV) for n in (3072, 16, 8192, 32)]
        for g in grads:
            g[:-33].fill_(0.25)              # the backward ADDS into the gradient buffers
        work = _padded(nwork)
        ops.encoder_hw_bwd(frames, idx_d, (H, W), stride, scale, dws[2], c1, d2_d, grads[0], grads[1], grads[2],
                           grads[3], work)
        h = [g.cpu().numpy() for g in grads]
        for g in h:
            assert (g[-33:] == SENT).all()
        wk = work.cpu().numpy()
        assert (wk[nwork:] == SENT).all()
        runs.append([g[:-33].astype(np.float64) - 0.25 for g in h] + [wk[:n1]])
        del work
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    want = _check_against_fp64(buf, idx, H, W, ws, scale, d2, c1_h, f2_h, runs[0][4].astype(np.float64))
    for name, got, ref in zip(("dW1", "db1", "dW2", "db2"), runs[0][:4], want):
        _close_bwd(got, ref, name)
    if (H, W) == (84, 84):
        f2_84 = torch.zeros(n2, dtype=torch.float32, device=DEV)
        c1_84 = torch.zeros(n1, dtype=torch.float32, device=DEV)
        ops.encoder_fwd(frames, idx_d, scale, *dws, f2_84, c1_84)
        _close_fwd(f2_h[:n2], f2_84.cpu().numpy().astype(np.float64), "f2 vs encoder_fwd")
        g84 = [torch.zeros(n, dtype=torch.float32, device=DEV) for n in (3072, 16, 8192, 32)]
        ops.encoder_bwd(frames, idx_d, scale, dws[2], c1[:n1], d2_d, *g84)     # the same ReLU mask on both sides
        for name, a, b in zip(("dW1", "db1", "dW2", "db2"), runs[0][:4], g84):
            _close_bwd(a, b.cpu().numpy().astype(np.float64), name + " vs encoder_bwd")


def test_encoder_hw_rejects_bad_shapes(ops):
    frames = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = [torch.zeros(n, device=DEV) for n in (3072, 16, 8192, 32)]
    big = torch.zeros(1 << 16, device=DEV)
    for shape in [(19, 64), (64, 481)]:
        with pytest.raises(ValueError):
            ops.encoder_hw_fwd(frames, idx, shape, 64 * 64 * 3, 1.0, *w, big, big)
    with pytest.raises(ValueError):                 # a stride shorter than a frame
        ops.encoder_hw_fwd(frames, idx, (64, 64), 64 * 64 * 3 - 16, 1.0, *w, big, big)
    with pytest.raises(ValueError):                 # c1 too small
        ops.encoder_hw_fwd(frames, idx, (64, 64), 64 * 64 * 3, 1.0, *w, big[:10], big)


# ---- ingest ------------------------------------------------------------------------------------------------------
def _mirror_step(st, H1, staged, actions, rewards, terminals, active, reset_on_terminal=True, clip=False):
    """numpy mirror of unreal_hostfed_step (without pixel change)."""
    for b in range(len(actions)):
        if active is not None and not active[b]:
            continue
        cnt = st["count"][b]
        slot = cnt % H1
        prev_term = st["r_terminal"][b, (cnt - 1) % H1] if cnt > 0 else 0
        term = terminals[b] != 0
        ncnt = cnt if (term and cnt > 0 and prev_term) else cnt + 1
        st["frames"][b, ncnt % H1] = staged[b]
        r = np.float32(min(max(rewards[b], -1), 1)) if clip else rewards[b]
        lr = np.float32(min(max(st["last_reward"][b], -1), 1)) if clip else st["last_reward"][b]
        st["r_reward"][b, slot] = r
        st["r_action"][b, slot] = actions[b]
        st["r_terminal"][b, slot] = int(term)
        st["r_last_action"][b, slot] = st["last_action"][b]
        st["r_last_reward"][b, slot] = lr
        st["count"][b] = ncnt
        reset = term and reset_on_terminal
        st["last_action"][b] = 0 if reset else actions[b]
        st["last_reward"][b] = 0.0 if reset else rewards[b]


@pytest.mark.parametrize("shape", [(100, 90), (120, 160), (20, 20)])
def test_hostfed_step_at_frame_size_matches_numpy_mirror(ops, shape):
    """unreal_hostfed_step / _reset at another frame size (no pixel change) write the ring (frames at ring.frame_stride),
    rewards as given (the indoor wrapper divides by termination_time on the host), the replay fields, the terminal /
    discard rules and the per-actor state exactly as a numpy mirror; the stride padding and r_pc are never written."""
    H, W = shape
    B, Hist = 5, 3
    H1 = Hist + 1
    rs = np.random.RandomState(H + W)
    ring = ops.Ring(B, Hist, DEV, objective_size=2, frame_shape=shape)
    fs = ring.frame_stride
    assert fs % 16 == 0 and fs >= H * W * 3 and ring.frames.numel() == B * H1 * fs
    ring.frames.fill_(0xA5)
    ring.r_pc.fill_(SENT)
    fb = H * W * 3
    st = dict(frames=np.full((B, H1, fs), 0xA5, np.uint8), count=np.zeros(B, np.int64),
              last_action=np.zeros(B, np.int64), last_reward=np.zeros(B, np.float32),
              r_reward=np.zeros((B, H1), np.float32), r_action=np.zeros((B, H1), np.int64),
              r_terminal=np.zeros((B, H1), np.int64), r_last_action=np.zeros((B, H1), np.int64),
              r_last_reward=np.zeros((B, H1), np.float32))

    def staged_of(fr):
        buf = np.zeros((B, fs), np.uint8)
        buf[:, :fb] = fr
        return buf

    fr0 = rs.randint(0, 256, size=(B, fb)).astype(np.uint8)
    s0 = staged_of(fr0)
    ops.hostfed_reset(ring, torch.from_numpy(s0.reshape(-1)).to(DEV))
    for b in range(B):
        st["frames"][b, 0] = s0[b]
    for step in range(9):
        fr = rs.randint(0, 256, size=(B, fb)).astype(np.uint8)
        s = staged_of(fr)
        a = rs.randint(0, 3, size=B).astype(np.int32)
        r = (rs.randint(-8, 9, size=B) / 8.0).astype(np.float32)
        t = (rs.random_sample(B) < 0.3).astype(np.int32)
        act = (rs.random_sample(B) < 0.8).astype(np.int32) if step % 3 == 2 else None
        ops.hostfed_step(ring, torch.from_numpy(s.reshape(-1)).to(DEV), torch.from_numpy(a).to(DEV),
                         torch.from_numpy(r).to(DEV), torch.from_numpy(t).to(DEV),
                         None if act is None else torch.from_numpy(act).to(DEV), clip_reward=False)
        _mirror_step(st, H1, s, a, r, t, act)
        if step == 5:                                # a masked reset of two actors
            m = np.array([1, 0, 0, 1, 0], np.int32)
            fr = rs.randint(0, 256, size=(B, fb)).astype(np.uint8)
            s = staged_of(fr)
            ops.hostfed_reset(ring, torch.from_numpy(s.reshape(-1)).to(DEV), torch.from_numpy(m).to(DEV))
            for b in np.nonzero(m)[0]:
                st["frames"][b, st["count"][b] % H1] = s[b]
                st["last_action"][b], st["last_reward"][b] = 0, 0.0
    np.testing.assert_array_equal(ring.frames.cpu().numpy().reshape(B, H1, fs), st["frames"])
    np.testing.assert_array_equal(ring.count.cpu().numpy(), st["count"])
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), st["last_action"])
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), st["last_reward"])
    for k in ("r_reward", "r_action", "r_terminal", "r_last_action", "r_last_reward"):
        np.testing.assert_array_equal(getattr(ring, k).cpu().numpy().reshape(B, H1), st[k], err_msg=k)
    assert (ring.r_pc.cpu().numpy() == SENT).all()
    assert st["r_terminal"].any() and (st["count"] > H1).any()


def test_ring_of_84_frames_is_unchanged_without_pixel_change(ops):
    """The default ring keeps FRAME_BYTES per frame, and at 84 x 84 the ingest without pixel change (r_pc NULL, the
    indoor contract at other sizes) writes exactly what the one with it writes (pixel change aside)."""
    from unreal_amd._lib import lib, ptr, stream
    B, Hist = 4, 3
    H1 = Hist + 1
    assert ops.frame_stride(84, 84) == ops.FRAME_BYTES
    rs = np.random.RandomState(84)
    rings = [ops.Ring(B, Hist, DEV), ops.Ring(B, Hist, DEV, frame_shape=(84, 84))]
    for ring in rings:
        assert ring.frame_stride == ops.FRAME_BYTES and ring.frames.numel() == B * H1 * ops.FRAME_BYTES
        ring.frames.zero_()
    s0 = torch.from_numpy(rs.randint(0, 256, size=B * ops.FRAME_BYTES).astype(np.uint8)).to(DEV)
    ops.hostfed_reset(rings[0], s0)
    ops.hostfed_reset(rings[1], s0)
    rings[1].r_pc.fill_(SENT)

    def step_without_pc(ring, s, a, r, t):         # ops.hostfed_step passes r_pc at 84 x 84: the entry, r_pc NULL
        lib().call("unreal_hostfed_step", B, H1, ring.frame_stride, ptr(s), None, ptr(a), ptr(r), ptr(t), None,
                   ptr(ring.last_action), ptr(ring.last_reward), ptr(ring.count), ptr(ring.frames), ptr(ring.r_reward),
                   ptr(ring.r_action), ptr(ring.r_terminal), ptr(ring.r_last_action), ptr(ring.r_last_reward), None, None,
                   None, ptr(ring.episode_reward), ptr(ring.score_out), ptr(ring.score_valid), 1, 0, 0, 48.0 * 255.0,
                   stream())
    for step in range(7):
        s = torch.from_numpy(rs.randint(0, 256, size=B * ops.FRAME_BYTES).astype(np.uint8)).to(DEV)
        a = torch.from_numpy(rs.randint(0, 3, size=B).astype(np.int32)).to(DEV)
        r = torch.from_numpy((rs.randint(-8, 9, size=B) / 4.0).astype(np.float32)).to(DEV)
        t = torch.from_numpy((rs.random_sample(B) < 0.3).astype(np.int32)).to(DEV)
        ops.hostfed_step(rings[0], s, a, r, t, clip_reward=False)
        step_without_pc(rings[1], s, a, r, t)
    for k in ("frames", "count", "last_action", "last_reward", "r_reward", "r_action", "r_terminal", "r_last_action",
              "r_last_reward"):
        assert torch.equal(getattr(rings[0], k), getattr(rings[1], k)), k
    assert (rings[1].r_pc.cpu().numpy() == SENT).all()


# ---- end to end --------------------------------------------------------------------------------------------------
@pytest.fixture
def generic_oracle(monkeypatch):
    """The oracle network with its two 2592-wide reshapes made shape-generic, and the (unused) pixel change of the
    oracle's indoor wrapper taken on the 84 x 84 grid only."""
    import oracle.hostfed as OH
    import oracle.model as M

    def fc1(conv_out, p):
        return torch.relu(conv_out.reshape(conv_out.shape[0], -1) @ p["W_base_fc1"] + p["b_base_fc1"])

    def rp_head(x3, p):
        _, h2 = M.encoder(x3, p)
        return torch.softmax(h2.reshape(1, -1) @ p["W_rp_fc1"] + p["b_rp_fc1"], dim=1)

    monkeypatch.setattr(M, "fc1", fc1)
    monkeypatch.setattr(M, "rp_head", rp_head)
    monkeypatch.setattr(OH, "calc_pixel_change", lambda s, l: np.zeros((20, 20)))
    return M


def _indoor_parity(cfg, B, Hist, T, tr, net, applier, draws, orc, edraws, shape, OBJ, iters=3):
    """_hostfed_parity (tests/test_trainer_gpu.py) for frames of `shape`: no pixel change in the ring."""
    from unreal_amd import ops
    from tests.test_trainer_gpu import _feed_draws, HF_LOSS_ATOL, HF_LOSS_RTOL, HF_GRAD_ATOL, HF_GRAD_REL
    while not tr._full:
        assert tr.process(None, 0) == (0, None)
    assert len(draws.log) == Hist
    for step_u in draws.log:
        for b in range(B):
            edraws[b].action_u.append(float(step_u[b]))
    orc.fill()
    np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
    H1 = Hist + 1
    fs, fb = tr.ring.frame_stride, shape[0] * shape[1] * 3
    fr = tr.ring.frames.cpu().numpy().reshape(B, H1, fs)[:, :, :fb].reshape(B, H1, shape[0], shape[1], 3)
    rr = tr.ring.r_reward.cpu().numpy().reshape(B, H1)
    rt = tr.ring.r_terminal.cpu().numpy().reshape(B, H1)
    robj = tr.ring.r_objective.cpu().numpy().reshape(B, H1, OBJ)
    for b in range(B):
        x = orc.actors[b].exp
        for i in range(x.top, x.count):
            f = x.frames[i]
            np.testing.assert_array_equal(fr[b, i % H1], np.rint(f.state['image'] * 255.0).astype(np.uint8))
            assert rr[b, i % H1] == f.reward and bool(rt[b, i % H1]) == bool(f.terminal)
            np.testing.assert_array_equal(robj[b, i % H1], f.state['objective'].astype(np.float32))
    global_t = 0
    for it in range(iters):
        draws.log.clear()
        lr = tr._anneal_learning_rate(global_t)
        tr.compute_gradients()
        g_dev = {k: v.detach().cpu().double().numpy().copy() for k, v in net.g.items()}
        tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, lr)
        norm_dev = float(tr.last_grad_norm.cpu()[0])
        tr.stats.zero_()
        ops.rollout_stats(B, tr.n_steps, tr.ring.score_valid, tr.ring.score_out, tr.stats)
        steps_dev, episodes_dev, score_dev = tr.read_stats()
        losses_dev = tr._publish_losses()
        _feed_draws(cfg, draws.log, edraws, T, B)
        steps_o, infos, losses_o, mean_g, norm_o = orc.process_batched(global_t)
        n_dev = tr.n_steps.cpu().numpy()
        acts = tr.actions.cpu().numpy().reshape(T, B)
        rews = tr.rewards.cpu().numpy().reshape(T, B)
        assert steps_dev == steps_o
        for b in range(B):
            n = infos[b]["n"]
            assert n_dev[b] == n and list(acts[:n, b]) == infos[b]["actions"]
            assert list(rews[:n, b]) == [float(r) for r in infos[b]["rewards"]]
        for key in ("policy_loss", "value_loss", "vr_loss", "rp_loss", "total_loss"):
            if key not in losses_o[0]:
                assert losses_dev[key] == 0.0
                continue
            want = np.mean([l[key] for l in losses_o])
            assert abs(losses_dev[key] - want) <= HF_LOSS_ATOL + HF_LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
        bad = []
        for (name, _), gref in zip(orc.params.items(), mean_g):
            gr = gref.numpy().reshape(-1)
            tol = HF_GRAD_ATOL + HF_GRAD_REL * np.abs(gr).max()
            err = np.abs(g_dev[name] - gr).max()
            if err > tol:
                bad.append("%s: err %.3g, bar %.3g, max |g| %.3g" % (name, err, tol, np.abs(gr).max()))
        assert not bad, (it, bad)
        assert abs(norm_dev - norm_o) <= 2e-4 * max(1.0, norm_o)
        global_t += steps_dev
    # post-RMSProp parameters: the oracle applied the same updates
    for name, pref in orc.params.items():
        pr = pref.detach().numpy().reshape(-1)
        pd = net.params.shaped(name).detach().cpu().double().numpy().reshape(-1)
        assert np.abs(pd - pr).max() <= 1e-5 + 1e-4 * np.abs(pr).max(), name


@pytest.mark.parametrize("shape", [(120, 160), (100, 90)])
@pytest.mark.parametrize("B", [3, 4])
def test_trainer_indoor_at_frame_size_matches_oracle(generic_oracle, shape, B):
    """Trainer(env_type='indoor') with image_shape = shape, LSTM + value replay + reward prediction, against the oracle
    trainer on the same draws (B = 4: the half-batch host / device schedule)."""
    from oracle.hostfed import OracleIndoorEnv
    from oracle.trainer import OracleTrainer, ExplicitDraws
    from tests.test_trainer_gpu import _cfg, RecordingDraws
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.synthetic_sim import SyntheticBatchIndoorSimulator, SyntheticIndoorSim
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer, PhiloxDraws
    Hist, T, OBJ = 40, 20, 5
    cfg = _cfg(True, (False, True, True), Hist, T)
    cfg.update(action_size=3, objective_size=OBJ, initial_learning_rate=7.0711e-4)
    kw = dict(episode_len=23, reward_p=0.15, big_reward_p=0.05, objective_size=OBJ, termination_time=50.0)
    name = "rooms_%dx%d" % shape
    Environment.register_indoor_config(name, OBJ, height=shape[0], width=shape[1])
    assert Environment.get_image_shape("indoor", name) == list(shape)
    sim = SyntheticBatchIndoorSimulator(B, seed=5, height=shape[0], width=shape[1], **kw)
    Environment.action_size = -1
    A = Environment.get_action_size("indoor", name)
    # seed: with seed 11 one conv2 pre-activation of the 120 x 160 rollout is +2.3e-8 in float64 and <= 0 in fp32, so the
    # oracle passes gradient through a ReLU the device closes -- an fp32-vs-fp64 boundary case, not an error of the
    # kernels (test_encoder_hw_matches_fp64 pins them with the device's own ReLU mask); this seed has no such element
    net = UnrealModel(A, OBJ, -1, True, False, True, True, 0.05, 0.001, DEV, image_shape=shape, seed=12,
                      frame_scale=1.0 / 255.0)
    F = 32 * ((((shape[0] - 8) // 4 + 1) - 4) // 2 + 1) * ((((shape[1] - 8) // 4 + 1) - 4) // 2 + 1)
    assert net.params.shaped("W_base_fc1").shape == (F, 256) and net.params.shaped("W_rp_fc1").shape == (3 * F, 3)
    applier = RMSPropApplier(None, decay=cfg["rmsp_alpha"], momentum=0.0, epsilon=cfg["rmsp_epsilon"],
                             clip_norm=cfg["grad_norm_clip"], device=DEV)
    draws = RecordingDraws(PhiloxDraws(0xA3C, 0))
    tr = Trainer(0, net, 7.0711e-4, None, applier, "indoor", name, True, False, True, True, 0.05, 0.001, T, T, 0.99, 0.9,
                 Hist, 10 ** 6, DEV, batch_size=B, draws=draws, simulator=sim, overlap_host=(B % 2 == 0),
                 image_shape=shape)
    tr.prepare()
    assert tr.overlap_host == (B % 2 == 0)
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    edraws = [ExplicitDraws() for _ in range(B)]
    envs = [OracleIndoorEnv(SyntheticIndoorSim(5 * 100003 + b, height=shape[0], width=shape[1], **kw), 50.0)
            for b in range(B)]
    orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=envs)
    _indoor_parity(cfg, B, Hist, T, tr, net, applier, draws, orc, edraws, shape, OBJ)


def test_batch1_runners_and_evaluate_at_120x160(generic_oracle):
    """run_base_policy_and_value / run_base_value / run_vr_value / run_rp_c at 120 x 160 against the oracle's trunk, and
    Evaluate over host-fed indoor actors of that size."""
    M = generic_oracle
    from unreal_amd.environment.synthetic_sim import SyntheticBatchIndoorSimulator
    from unreal_amd.evaluate import Evaluate
    from unreal_amd.model.model import UnrealModel
    shape, A, OBJ = (120, 160), 3, 4
    net = UnrealModel(A, OBJ, -1, True, False, True, True, 0.05, 0.001, DEV, image_shape=shape, seed=7)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    rs = np.random.RandomState(3)
    imgs = [rs.randint(0, 256, size=shape + (3,)) / 255.0 for _ in range(3)]
    lar = np.concatenate([np.eye(A)[1], [0.25], rs.uniform(-1, 1, OBJ)])
    x = torch.tensor(np.stack(imgs[:1]), dtype=torch.float64)
    feat, st = M.trunk(x, torch.tensor(lar[None], dtype=torch.float64), p, True, None)
    pi_o, v_o = M.policy_value(feat, p)
    pi, v, _ = net.run_base_policy_and_value(None, {'image': imgs[0]}, lar)
    np.testing.assert_allclose(pi, pi_o.numpy()[0], rtol=1e-4, atol=2e-6)
    assert abs(v - float(v_o[0])) <= 2e-5 + 1e-4 * abs(float(v_o[0]))
    np.testing.assert_allclose(net.base_lstm_state_out[1].cpu().numpy(), st[1].numpy().reshape(-1), rtol=1e-4, atol=2e-6)
    assert abs(net.run_vr_value(None, {'image': imgs[0]}, lar) - float(v_o[0])) <= 2e-5 + 1e-4 * abs(float(v_o[0]))
    z = net.run_rp_c(None, [{'image': im} for im in imgs])
    z_o = M.rp_head(torch.tensor(np.stack(imgs), dtype=torch.float64), p).numpy()[0]
    np.testing.assert_allclose(z, z_o, rtol=1e-4, atol=2e-6)
    with pytest.raises(ValueError):
        net.run_base_value(None, {'image': np.zeros((84, 84, 3))}, lar)
    sim = SyntheticBatchIndoorSimulator(2, seed=9, objective_size=OBJ, height=shape[0], width=shape[1], episode_len=6)
    ev = Evaluate(net, batch_size=2, device=DEV, simulator=sim)
    out = ev.process(4, max_episode_steps=50)
    assert out["episodes"] >= 4 and out["timeouts"] == 0 and out["mean_length"] == 6
    pi_e = ev.pi.cpu().numpy().reshape(2, A)
    np.testing.assert_allclose(pi_e.sum(1), 1.0, rtol=1e-5)
