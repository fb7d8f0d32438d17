"""Action counts 2..18 (gym / Atari) through every A-dependent kernel, against float64 at the suite's bars.

Row counts sit on both sides of each launch-shape threshold: linear_small_fwd's 4 rows per workgroup, linear_small_bwd's
4-row unroll and 128-row chunks, the pixel-control kernels' grid caps (768 workgroups for the wide forward, 512 for the wide
backward / training pass: frames past them run through the grid-stride loop).  A >= 8 takes the wide pixel-control
kernels; A in {8, 9, ...} also hit head instances that did not exist before."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import DEV, close, dev

pytestmark = pytest.mark.gpu

ACTIONS = [2, 5, 7, 8, 9, 12, 16, 18]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("rows", [1, 7, 130])
def test_linear_small_fwd_bwd(ops, A, rows):
    rs = np.random.RandomState(100 * A + rows)
    for nout in (A, A + 1):                       # policy logits; the LSTM input's action + reward rows
        K, ldx, ldo = 256, 264, nout + 3
        X = rs.normal(size=(rows, ldx))
        W = rs.normal(size=(K, nout)) * 0.1
        b = rs.normal(size=nout) * 0.1
        out = torch.full((rows * ldo,), 5.0, device=DEV)
        ops.linear_small_fwd(rows, K, nout, dev(X.reshape(-1), torch.float32), ldx, dev(W.reshape(-1), torch.float32),
                             dev(b, torch.float32), out, ldo)
        ref = X[:, :K] @ W + b
        o = out.cpu().numpy().reshape(rows, ldo)
        close(o[:, :nout], ref, atol=1e-5, rtol=1e-5, what="linear_small_fwd A=%d" % nout)
        assert (o[:, nout:] == 5.0).all()
        dO = rs.normal(size=(rows, ldo))
        dX0 = rs.normal(size=(rows, K))
        dX = dev(dX0.reshape(-1), torch.float32)
        dW = torch.zeros(K * nout, device=DEV)
        db = torch.zeros(nout, device=DEV)
        ops.linear_small_bwd(rows, K, nout, dev(X.reshape(-1), torch.float32), ldx, dev(dO.reshape(-1), torch.float32), ldo,
                             dev(W.reshape(-1), torch.float32), dX, K, True, dW, db)
        close(dX.reshape(rows, K), dX0 + dO[:, :nout] @ W.T, atol=1e-5, rtol=1e-5, what="linear_small_bwd dX")
        close(dW.reshape(K, nout), X[:, :K].T @ dO[:, :nout], atol=1e-4, rtol=1e-5, what="linear_small_bwd dW")
        close(db, dO[:, :nout].sum(0), atol=1e-4, rtol=1e-5, what="linear_small_bwd db")


def _draw_ref(pi32, u):
    """numpy RandomState.choice: searchsorted(cumsum / sum, u, 'right') in float64, clamped to A - 1."""
    p = pi32.astype(np.float64)
    c = np.cumsum(p, 1)
    cdf = c / c[:, -1:]
    return np.array([min(int(np.searchsorted(cdf[r], u[r], side="right")), p.shape[1] - 1) for r in range(len(u))])


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("rows", [1, 5, 300])
def test_softmax_sample_and_policy_step(ops, A, rows):
    rs = np.random.RandomState(7 * A + rows)
    X = rs.normal(size=(rows, 256)).astype(np.float32)
    Wp = (rs.normal(size=(256, A)) * 0.2).astype(np.float32)
    bp = (rs.normal(size=A) * 0.2).astype(np.float32)
    Wv = (rs.normal(size=256) * 0.1).astype(np.float32)
    bv = np.float32([0.3])
    u = rs.random_sample(rows)
    u[0] = 0.0
    # logits by the head kernel, then the draw
    logits = torch.zeros(rows * A, device=DEV)
    ops.linear_small_fwd(rows, 256, A, dev(X.reshape(-1)), 256, dev(Wp.reshape(-1)), dev(bp), logits, A)
    lg = logits.cpu().numpy().reshape(rows, A).astype(np.float64)
    e = np.exp(lg - lg.max(1, keepdims=True))
    pi_ref = e / e.sum(1, keepdims=True)
    pi = logits.clone()
    act = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ops.softmax_sample(rows, A, pi, A, u=dev(u), action=act)
    pi_np = pi.cpu().numpy().reshape(rows, A)
    close(pi_np, pi_ref, atol=1e-6, rtol=1e-5, what="softmax")
    np.testing.assert_array_equal(act.cpu().numpy(), _draw_ref(pi_np, u))
    # the fused rollout step: bit-identical to the two kernels above
    pi2 = torch.zeros(rows * A, device=DEV)
    v2 = torch.zeros(rows, device=DEV)
    act2 = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ops.policy_step(rows, A, dev(X.reshape(-1)), 256, dev(Wp.reshape(-1)), dev(bp), dev(Wv), dev(bv), dev(u), pi2, v2, act2)
    assert torch.equal(pi2, pi) and torch.equal(act2, act)
    close(v2, X.astype(np.float64) @ Wv + bv[0], atol=1e-5, rtol=1e-5, what="policy_step v")
    # greedy (u = null): first maximum
    act3 = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ops.policy_step(rows, A, dev(X.reshape(-1)), 256, dev(Wp.reshape(-1)), dev(bp), dev(Wv), dev(bv), None, pi2, v2, act3)
    np.testing.assert_array_equal(act3.cpu().numpy(), np.argmax(pi_np, 1))


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("rows", [3, 257])
def test_base_loss_grad(ops, A, rows):
    rs = np.random.RandomState(11 * A + rows)
    beta, gs = 0.001, 0.25
    logits = torch.tensor(rs.normal(size=(rows, A)) * 2, requires_grad=True)
    v = torch.tensor(rs.normal(size=rows), requires_grad=True)
    act = rs.randint(0, A, rows)
    adv = rs.normal(size=rows)
    R = rs.normal(size=rows)
    active = (rs.rand(rows) < 0.8).astype(np.int32)
    m = torch.tensor(active.astype(np.float64))
    pi = torch.softmax(logits, 1)
    log_pi = torch.log(torch.clamp(pi, 1e-20, 1.0))
    ent = -(pi * log_pi).sum(1)
    pl = -(((log_pi * torch.tensor(np.eye(A)[act])).sum(1) * torch.tensor(adv) + ent * beta) * m).sum()
    vl = 0.25 * (((torch.tensor(R) - v) ** 2) * m).sum()
    ((pl + vl) * gs).backward()
    dl = torch.zeros(rows * A, device=DEV)
    dv = torch.zeros(rows, device=DEV)
    losses = torch.zeros(3, device=DEV)
    ops.base_loss_grad(rows, A, dev(pi.detach().reshape(-1), torch.float32), A, dev(v.detach(), torch.float32),
                       dev(act, torch.int32), dev(adv, torch.float32), dev(R, torch.float32), dev(active), beta, gs,
                       dl, dv, losses)
    close(dl.reshape(rows, A), logits.grad, what="dlogits", atol=1e-6, rtol=1e-4)
    close(dv, v.grad, what="dv", atol=1e-6, rtol=1e-4)
    close(losses, [float(pl) * gs, float(vl) * gs, float((ent * m).sum()) * gs], atol=1e-4, rtol=1e-4, what="losses")


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("N", [1, 9, 600])
def test_pc_deconv_fwd_bwd_train(ops, A, N):
    """The three pixel-control entries at the bars of test_kernels_gpu.test_pc_deconv_fwd_bwd."""
    if N == 600 and A not in (8, 18):
        pytest.skip("the grid-stride row count is pinned at the narrowest and widest wide instances")
    rs = np.random.RandomState(N * 100 + A)
    lam, gs = 0.05, 0.25
    hp = torch.tensor(np.maximum(rs.normal(size=(N, 9, 9, 32)), 0), requires_grad=True)
    Wv = torch.tensor(rs.uniform(-.1, .1, (4, 4, 1, 32)), requires_grad=True)
    bv = torch.tensor(rs.uniform(-.1, .1, 1), requires_grad=True)
    Wa = torch.tensor(rs.uniform(-.1, .1, (4, 4, A, 32)), requires_grad=True)
    ba = torch.tensor(rs.uniform(-.1, .1, A), requires_grad=True)
    x = hp.permute(0, 3, 1, 2)
    pre = torch.cat([F.conv_transpose2d(x, Wv.permute(3, 2, 0, 1), bv, stride=2),
                     F.conv_transpose2d(x, Wa.permute(3, 2, 0, 1), ba, stride=2)], 1)      # [N, 1 + A, 20, 20]
    pre.retain_grad()
    v, a = F.relu(pre[:, :1]), F.relu(pre[:, 1:])
    q = (v + a - a.mean(1, keepdim=True)).permute(0, 2, 3, 1)
    qmax_ref = q.max(3)[0]
    act = rs.randint(0, A, N)
    tgt = torch.tensor(rs.uniform(0, 1, (N, 20, 20)))
    mask = (rs.rand(N) < 0.8).astype(np.int32)
    mask[0] = 1
    m = torch.tensor(mask.astype(np.float64)).reshape(N, 1, 1)
    qa = (q * torch.tensor(np.eye(A)[act]).reshape(N, 1, 1, A)).sum(3)
    loss = lam * 0.5 * (((tgt - qa) ** 2) * m).sum()
    (loss * gs).backward()
    f32 = torch.float32
    d = dict(hp=dev(hp.detach().reshape(-1), f32), Wv=dev(Wv.detach().reshape(-1), f32), bv=dev(bv.detach(), f32),
             Wa=dev(Wa.detach().reshape(-1), f32), ba=dev(ba.detach(), f32))
    qmax = torch.zeros(N * 400, device=DEV)
    ops.pc_deconv_fwd(N, A, d["hp"], d["Wv"], d["bv"], d["Wa"], d["ba"], qmax=qmax)
    close(qmax.reshape(N, 20, 20), qmax_ref, what="qmax")
    d_dec = torch.zeros(N * 400 * (1 + A), device=DEV)
    ls = torch.zeros(1, device=DEV)
    ddm = torch.zeros(1, device=DEV)
    ops.pc_deconv_fwd(N, A, d["hp"], d["Wv"], d["bv"], d["Wa"], d["ba"], action=dev(act, torch.int32),
                      target=dev(tgt.reshape(-1), f32), mask=dev(mask), lam=lam, grad_scale=gs, d_dec=d_dec, loss=ls,
                      ddec_max=ddm)
    close(ls, [float(loss) * gs], atol=1e-4, rtol=1e-4, what="pc loss")
    close(d_dec.reshape(N, 20, 20, 1 + A), pre.grad.permute(0, 2, 3, 1), atol=1e-6, rtol=1e-5, what="d_dec")
    assert float(ddm) >= float(d_dec.abs().max())
    tol = dict(atol=1e-5, rtol=1e-5)
    d_hp = torch.zeros(N * 2592, device=DEV)
    dWv = torch.zeros(512, device=DEV); dbv = torch.zeros(1, device=DEV)
    dWa = torch.zeros(512 * A, device=DEV); dba = torch.zeros(A, device=DEV)
    ops.pc_deconv_bwd(N, A, d["hp"], d_dec, d["Wv"], d["Wa"], d_hp, dWv, dbv, dWa, dba)
    close(d_hp.reshape(N, 9, 9, 32), hp.grad * (hp.detach() > 0), what="d_hp", **tol)
    close(dWv.reshape(4, 4, 1, 32), Wv.grad, what="dWv", **tol)
    close(dWa.reshape(4, 4, A, 32), Wa.grad, what="dWa", **tol)
    close(dbv, bv.grad, what="dbv", **tol)
    close(dba, ba.grad, what="dba", **tol)
    # the training pass in one launch: same reference, same bars; its d_dec output is the forward kernel's bit for bit
    d_dec2 = torch.zeros_like(d_dec); ls2 = torch.zeros(1, device=DEV); d_hp2 = torch.full_like(d_hp, 7.0)
    dWv2 = torch.zeros(512, device=DEV); dbv2 = torch.zeros(1, device=DEV)
    dWa2 = torch.zeros(512 * A, device=DEV); dba2 = torch.zeros(A, device=DEV); mx = torch.zeros(1, device=DEV)
    ops.pc_deconv_train(N, A, d["hp"], d["Wv"], d["bv"], d["Wa"], d["ba"], dev(act, torch.int32), dev(tgt.reshape(-1), f32),
                        dev(mask), lam, gs, ls2, d_hp2, dWv2, dbv2, dWa2, dba2, dhp_max=mx, d_dec=d_dec2)
    assert torch.equal(d_dec2, d_dec)
    close(ls2, [float(loss) * gs], atol=1e-4, rtol=1e-4, what="pc loss (one launch)")
    close(d_hp2.reshape(N, 9, 9, 32), hp.grad * (hp.detach() > 0), what="d_hp (one launch)", **tol)
    close(dWv2.reshape(4, 4, 1, 32), Wv.grad, what="dWv (one launch)", **tol)
    close(dWa2.reshape(4, 4, A, 32), Wa.grad, what="dWa (one launch)", **tol)
    close(dbv2, bv.grad, what="dbv (one launch)", **tol)
    close(dba2, ba.grad, what="dba (one launch)", **tol)
    assert float(mx) == float(d_hp2.abs().max())
