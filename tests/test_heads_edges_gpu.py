"""Policy and loss heads at saturation (GPU): csrc/heads.hip base_loss_grad_kernel<8> / <18>, vr_loss_grad_kernel,
rp_loss_grad_kernel, softmax_sample_kernel and policy_row<A> on the inputs a trained, saturated policy produces.

The loss kernels clip probabilities to [1e-20, 1] (model.py:497, 575) and pass the gradient only inside that range
(`un`).  Fed logits from N(0, 2) the smallest probability is about e^-15 and neither `un = 0`, `pc = 1e-20` nor the
comparison on the edge itself ever executes; here probabilities sit at 1, on the fp32 edge, one ulp to either side of
it, far below it, in the subnormals and at 0.  The reference is fp64 torch autograd with the kernel's fp32 input as the
leaf and the fp32 constant as the clip edge: 1e-20 as a double lies ABOVE np.float32(1e-20), so the on-edge row would
otherwise be clipped by the reference and not by the kernel.  Bars are those of test_base_vr_rp_loss_grads and
test_softmax_sample_matches_numpy_choice; none is widened."""
import itertools

import numpy as np
import pytest
import torch

try:
    import margins
except ImportError:            # imported as tests.<module>: tests/ itself is not on sys.path
    from tests import margins

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
LO = float(F(1e-20))            # the clip edge the kernels compare with: the fp32 constant, as a double
BETA, GS = 0.001, 1.0 / 7


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


def dev(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dt is not None:
        t = t.to(dt)
    return t.to(DEV).contiguous()


def close(got, ref, atol, rtol, what):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    margins.record_close(what, got, ref, atol, rtol)
    err = np.abs(got - ref) - (atol + rtol * np.abs(ref))
    assert np.isfinite(got).all() and err.max() <= 0, "%s: max |d|=%g at %s (got %g, ref %g)" % (
        what, np.abs(got - ref).max(), np.unravel_index(np.argmax(err), err.shape), got.flat[np.argmax(err)],
        ref.flat[np.argmax(err)])


# ---------------------------------------------------------------------------------------------------
# base loss
# ---------------------------------------------------------------------------------------------------
def saturated_rows(A):
    """fp32 probability rows and taken actions.  Patterns (padded with zeros to A):
      (1)                 a saturated policy: p = 1 and p = 0 (un = 0, pc = 1e-20 on every other action)
      (1, t)              t = the fp32 clip edge 1e-20 (un = 1: the comparison is >=), one ulp below it (un = 0) and above
                          it (un = 1), 1e-19 (inside), 1e-25, 1e-30 (outside) and 1e-45 (a subnormal, outside)
      (1 - 2^-24, 6e-8, 1e-40)   the largest fp32 below 1 next to what is left of the mass, and a subnormal
      (0.5, 0.5)          control
    each rolled through every position and paired with every action index, so that the taken action's probability is in
    turn 1, inside the range, on its lower edge, just below it, and 0; repeated (with other advantages) up to a row count
    above 256 that is no multiple of 64: more than one workgroup, a partial last wave."""
    lo = F(1e-20)
    ts = [lo, np.nextafter(lo, F(0)), np.nextafter(lo, F(1)), F(1e-19), F(1e-25), F(1e-30), F(1e-45)]
    assert ts[1] < lo < ts[2] and 0 < ts[6] < F(1.2e-38)
    pats = [(1,)] + [(1, t) for t in ts] + [(F(1) - F(2.0 ** -24), F(6e-8), F(1e-40)), (0.5, 0.5)]
    pi, act = [], []
    for p in pats:
        base = np.zeros(A, F)
        base[:len(p)] = p
        for s in range(A):
            for a in range(A):
                pi.append(np.roll(base, s))
                act.append(a)
    n = max(len(pi), 257)
    n += (n % 64 == 0)
    reps = -(-n // len(pi))
    return np.stack(pi * reps)[:n], np.array(act * reps, np.int32)[:n]


def base_reference(pi, v, act, adv, R, active):
    """fp64 autograd of model.py:490-516 with pi as the leaf, then the softmax Jacobian: dlogits = pi (g - sum pi g).
    Rows with active = 0 contribute nothing and their inputs are not looked at.  -> dlogits, dv, per-row
    (policy loss, value loss, entropy) * GS."""
    on = active != 0
    rows, A = pi.shape
    safe = lambda x, fill: np.where(on.reshape((-1,) + (1,) * (x.ndim - 1)), x, fill).astype(np.float64)
    p = torch.tensor(safe(pi, 1.0 / A), requires_grad=True)
    vv = torch.tensor(safe(v, 0.0), requires_grad=True)
    ad, RR, m = torch.tensor(safe(adv, 0.0)), torch.tensor(safe(R, 0.0)), torch.tensor(on.astype(np.float64))
    log_pi = torch.log(torch.clamp(p, LO, 1.0))
    ent = -(p * log_pi).sum(1)
    pl = -(log_pi[torch.arange(rows), torch.tensor(act.astype(np.int64))] * ad + ent * BETA) * m
    vl = 0.25 * ((RR - vv) ** 2) * m
    ((pl.sum() + vl.sum()) * GS).backward()
    g = p.grad
    pd = p.detach()
    dlogits = pd * (g - (pd * g).sum(1, keepdim=True))
    per_row = torch.stack([pl, vl, ent * m], 1).detach() * GS
    return dlogits.numpy(), vv.grad.numpy(), per_row.numpy()


def run_base(ops, pi, v, act, adv, R, active, r0=0, r1=None):
    """Launch on rows [r0, r1) of device copies of the inputs."""
    A = pi.shape[1]
    r1 = pi.shape[0] if r1 is None else r1
    n = r1 - r0
    dl = torch.full((n * A,), np.nan, device=DEV)
    dv = torch.full((n,), np.nan, device=DEV)
    losses = torch.zeros(3, device=DEV)
    ops.base_loss_grad(n, A, dev(pi[r0:r1].reshape(-1)), A, dev(v[r0:r1]), dev(act[r0:r1]), dev(adv[r0:r1]), dev(R[r0:r1]),
                       dev(active[r0:r1]), BETA, GS, dl, dv, losses)
    return dl.cpu().numpy().reshape(n, A), dv.cpu().numpy(), losses.cpu().numpy()


@pytest.mark.parametrize("A", [3, 4, 6, 9, 18])
def test_base_loss_grad_saturated(ops, A):
    """A <= 8 runs base_loss_grad_kernel<8>, 9 and 18 the <18> instantiation.  One launch over all rows, then single-row
    launches (rows = 1) of the rows whose taken action has each probability of the table."""
    pi, act = saturated_rows(A)
    rows = len(act)
    assert rows > 256 and rows % 64
    rs = np.random.RandomState(30 + A)
    adv = (rs.normal(size=rows) * 3).astype(F)
    v, R = rs.normal(size=rows).astype(F), rs.normal(size=rows).astype(F)
    active = np.ones(rows, np.int32)
    taken = pi[np.arange(rows), act]
    lo = F(1e-20)
    for cond in (taken == 1, taken == lo, taken == np.nextafter(lo, F(0)), taken == 0, (taken > 0) & (taken < F(1e-38))):
        assert cond.any()                                   # the table puts the taken action where it says
    want_dl, want_dv, want_rows = base_reference(pi, v, act, adv, R, active)
    dl, dv, losses = run_base(ops, pi, v, act, adv, R, active)
    close(dl, want_dl, 1e-6, 1e-4, "dlogits")
    close(dv, want_dv, 1e-6, 1e-4, "dv")
    close(losses, want_rows.sum(0), 1e-4, 1e-4, "losses")
    per_pattern = A * A                                     # rows of one pattern: shift-major, action-minor
    for r in sorted({p * per_pattern + a for p in range(10) for a in (0, 1)}):
        dl, dv, losses = run_base(ops, pi, v, act, adv, R, active, r, r + 1)
        close(dl, want_dl[r:r + 1], 1e-6, 1e-4, "dlogits, one row")
        close(dv, want_dv[r:r + 1], 1e-6, 1e-4, "dv, one row")
        close(losses, want_rows[r], 1e-4, 1e-4, "losses, one row")


@pytest.mark.parametrize("A", [4, 18])
def test_loss_grads_ignore_inactive_rows(ops, A):
    """Rows past an actor's n_steps and masked replay rows hold stale memory in production: here NaN and +-inf in pi, v,
    adv and R.  Their dlogits and dv are exactly +0.0 and the loss sums are those of the active rows alone."""
    rs = np.random.RandomState(40 + A)
    rows = 333
    z = rs.normal(size=(rows, A)) * 2
    pi = (np.exp(z) / np.exp(z).sum(1, keepdims=True)).astype(F)
    act = rs.randint(0, A, rows).astype(np.int32)
    adv, v, R = (rs.normal(size=rows).astype(F) for _ in range(3))
    active = (rs.rand(rows) >= 0.25).astype(np.int32)
    active[[0, 63, 64, 255, 256, rows - 1]] = [0, 0, 1, 0, 1, 0]        # wave and workgroup ends on both sides
    off = np.flatnonzero(active == 0)
    junk = np.array([np.nan, np.inf, -np.inf], F)
    for x in (pi, adv, v, R):
        x[off] = junk[rs.randint(0, 3, size=(len(off),) + x.shape[1:])]
    pi[off[::2], 0] = np.nan                                            # at least one NaN per second row
    want_dl, want_dv, want_rows = base_reference(pi, v, act, adv, R, active)
    dl, dv, losses = run_base(ops, pi, v, act, adv, R, active)
    for got in (dl[off], dv[off]):
        assert (got == 0).all() and not np.signbit(got).any()
    on = active != 0
    close(dl[on], want_dl[on], 1e-6, 1e-4, "dlogits")
    close(dv[on], want_dv[on], 1e-6, 1e-4, "dv")
    close(losses, want_rows[on].sum(0), 1e-4, 1e-4, "losses")
    # value replay: mask = 0 rows hold NaN in v and R
    dv2 = torch.full((rows,), np.nan, device=DEV)
    ls = torch.zeros(1, device=DEV)
    ops.vr_loss_grad(rows, dev(v), dev(R), dev(active), GS, dv2, ls)
    dv2 = dv2.cpu().numpy()
    assert (dv2[off] == 0).all() and not np.signbit(dv2[off]).any()
    diff = R[on].astype(np.float64) - v[on].astype(np.float64)
    close(dv2[on], -GS * diff, 1e-6, 1e-4, "vr dv")
    close(ls, [0.5 * (diff ** 2).sum() * GS], 1e-4, 1e-4, "vr loss")


# ---------------------------------------------------------------------------------------------------
# reward prediction
# ---------------------------------------------------------------------------------------------------
RP_GAPS = (0.0, 1.0, 44.0, 45.3, 47.0, 60.0, 100.0, 200.0)


def rp_rows():
    """Logit rows (0, -g, -2g) in every permutation, for every class.  e^-44 = 7.8e-20 and e^-45.3 = 2.1e-20 lie inside
    the clip range, e^-47 = 3.9e-21 and e^-60 outside it, each at least a factor 2 from 1e-20 (fp32 expf and fp64 exp
    then fall on the same side); e^-88, e^-90.6 and e^-100 are fp32 subnormals, e^-120 and beyond flush to 0; g = 0 is
    three equal logits."""
    z, c = [], []
    for g in RP_GAPS:
        for perm in itertools.permutations((0.0, -g, -2 * g)):
            for k in range(3):
                z.append(perm)
                c.append(k)
    return np.array(z, F), np.array(c, np.int32)


@pytest.mark.parametrize("rows", [1, 64, 300])
def test_rp_loss_grad_saturated(ops, rows):
    z, cls = rp_rows()
    if rows == 1:
        launches = [slice(r, r + 1) for r in range(18 + 1, len(cls), 18)]       # (0, -g, -2g), class 1: p_c ~ e^-g, g > 0
    elif rows == 64:
        launches = [slice(40, 104)]                                              # g = 44 .. 47: around the edge
    else:
        reps = -(-rows // len(cls))
        z, cls = np.tile(z, (reps, 1))[:rows], np.tile(cls, reps)[:rows]
        launches = [slice(0, rows)]
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    pr = torch.softmax(zt, 1)
    per_row = -torch.log(torch.clamp(pr, LO, 1.0))[torch.arange(len(cls)), torch.tensor(cls.astype(np.int64))]
    (per_row.sum() * GS).backward()
    per_row = per_row.detach()
    taken = pr.detach().numpy()[np.arange(len(cls)), cls]
    assert (np.abs(np.log(taken[taken > 0] / LO)) > np.log(2)).all()             # no case near the edge
    for s in launches:
        n = s.stop - s.start
        assert n == rows
        prob = torch.full((n * 3,), np.nan, device=DEV)
        dz = torch.full((n * 3,), np.nan, device=DEV)
        ls = torch.zeros(1, device=DEV)
        ops.rp_loss_grad(n, dev(z[s].reshape(-1)), dev(cls[s]), GS, prob, dz, ls)
        close(prob.reshape(n, 3), pr.detach()[s], 1e-6, 1e-5, "rp prob")
        close(dz.reshape(n, 3), zt.grad[s], 1e-6, 1e-4, "rp dlogits")
        close(ls, [float(per_row[s].sum()) * GS], 1e-4, 1e-4, "rp loss")
    if rows == 1:
        assert (taken[[s.start for s in launches]] < 0.5).all() and len(launches) == len(RP_GAPS) - 1


# ---------------------------------------------------------------------------------------------------
# action draws
# ---------------------------------------------------------------------------------------------------
def logit_rows(A):
    """Rows with ties in the CDF (zero-probability actions before, between and after the mass), exp underflow and
    equal maxima:
      all equal (at 0 and at 3.5)
      one action at 0, the rest at -30 (tiny but distinct CDF steps), -90 (an fp32 subnormal: 1 + e^-90 = 1 in fp64, a
        tie), -104 (rounds to 0 or to the smallest subnormal) and -1e4 (expf underflows to exactly 0); the mass on the
        first, a middle and the last action
      two equal maxima (first pair, first and last, middle and last), the rest at -30 and at -1e4
      a common offset of 1e4, with gaps of 0, 0.25 and 2 between neighbours
      a plain spread row (control)"""
    rows = [np.zeros(A), np.full(A, 3.5)]
    spots = (0, A // 2, A - 1)
    for gap in (30.0, 90.0, 104.0, 1e4):
        for s in spots:
            r = np.full(A, -gap)
            r[s] = 0
            rows.append(r)
    for rest in (-30.0, -1e4):
        for i, j in ((0, 1), (0, A - 1), (A // 2, A - 1)):
            r = np.full(A, rest)
            r[i] = r[j] = 0
            rows.append(r)
    for step in (0.0, 0.25, 2.0):
        rows.append(1e4 + step * np.arange(A))
    rows.append(np.linspace(-2, 2, A))
    return np.array(rows, F)


def _policy_step_inputs(logits):
    """X carries the logit of action n in column n, Wp selects it: a row sum of one value and zeros is exact."""
    rows, A = logits.shape
    X = np.zeros((rows, 256), F)
    X[:, :A] = logits
    Wp = np.zeros((256, A), F)
    Wp[np.arange(A), np.arange(A)] = 1
    Wv = np.random.RandomState(A).normal(size=256).astype(F)
    return dev(X.reshape(-1)), dev(Wp.reshape(-1)), torch.zeros(A, device=DEV), dev(Wv), torch.ones(1, device=DEV)


@pytest.mark.parametrize("A", [3, 4, 6, 18])
def test_action_draws_on_cdf_steps_and_ties(ops, A):
    """unreal_softmax_sample, and unreal_policy_step bit-identical to it, with u on every step of the device's own
    normalised fp64 CDF and one ulp to either side of it; greedy with equal maxima takes the first."""
    base = logit_rows(A)
    n0 = len(base)
    lp = dev(base.reshape(-1))
    ops.softmax_sample(n0, A, lp, A)                        # pi alone
    pi0 = lp.cpu().numpy().reshape(n0, A)
    ref = torch.softmax(torch.tensor(base.astype(np.float64)), 1).numpy()
    close(pi0, ref, 1e-6, 1e-5, "pi")
    cdf0 = np.cumsum(pi0.astype(np.float64), 1)
    cdf0 /= cdf0[:, -1:]
    assert any(len(set(c)) < A for c in cdf0) and any((c[:-1] == 0).any() for c in cdf0)   # ties, leading zeros
    src, us = [], []
    for r in range(n0):
        cand = [0.0, 1.0 - 2.0 ** -53]
        for c in cdf0[r]:
            cand += [c, np.nextafter(c, 0.0), np.nextafter(c, 2.0)]
        for x in sorted(set(cand)):
            if 0.0 <= x <= 1.0:
                src.append(r)
                us.append(x)
    src, us = np.array(src), np.array(us, np.float64)
    rows = len(src)
    logits = base[src]
    lp = dev(logits.reshape(-1))
    act = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    ops.softmax_sample(rows, A, lp, A, dev(us), act)
    pi = lp.cpu().numpy().reshape(rows, A)
    np.testing.assert_array_equal(pi, pi0[src])             # a row's softmax does not depend on its neighbours or on u
    cdf = np.cumsum(pi.astype(np.float64), 1)
    cdf /= cdf[:, -1:]
    want = np.minimum([np.searchsorted(cdf[r], us[r], side="right") for r in range(rows)], A - 1)
    got = act.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert set(got) == set(range(A))
    # the fused step on exact logits: the same pi, the same action
    X, Wp, bp, Wv, bv = _policy_step_inputs(logits)
    pi1, v1 = torch.full((rows * A,), np.nan, device=DEV), torch.full((rows,), np.nan, device=DEV)
    a1 = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    ops.policy_step(rows, A, X, 256, Wp, bp, Wv, bv, dev(us), pi1, v1, a1)
    assert torch.equal(pi1, lp) and torch.equal(a1, act)
    # greedy: np.argmax (the first maximum) of the device's own pi, on both paths
    lg = dev(base.reshape(-1))
    ag = torch.full((n0,), -1, dtype=torch.int32, device=DEV)
    ops.softmax_sample(n0, A, lg, A, None, ag)
    np.testing.assert_array_equal(ag.cpu().numpy(), np.argmax(pi0, 1))
    assert sum((p == p.max()).sum() > 1 for p in pi0) >= 8  # rows with equal maxima
    X, Wp, bp, Wv, bv = _policy_step_inputs(base)
    pi2, v2 = torch.full((n0 * A,), np.nan, device=DEV), torch.full((n0,), np.nan, device=DEV)
    a2 = torch.full((n0,), -1, dtype=torch.int32, device=DEV)
    ops.policy_step(n0, A, X, 256, Wp, bp, Wv, bv, None, pi2, v2, a2)
    assert torch.equal(pi2, lg) and torch.equal(a2, ag)
