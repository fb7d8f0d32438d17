"""Sample reuse without a GPU: option checks, flags, the entry's argument checks and hand-derivable rows of
the fp64 loss model (tests/ppo_model.py) that the GPU tests hold the kernel against."""
import numpy as np
import pytest
import torch

try:
    import ppo_model as PM
except ImportError:            # imported as tests.<module>
    from tests import ppo_model as PM
from oracle import model as OM


@pytest.fixture(scope="module")
def built():
    from unreal_amd.build import build_library
    return build_library(verbose=False)


def test_check_reuse_options():
    from unreal_amd.train.trainer import Trainer
    chk = Trainer.check_reuse_options
    assert chk("maze", 1, 0.2) == (1, 0.2) and chk("arcade", 16, 0.5) == (16, 0.5) and chk("maze", 4, 1e-3) == (4, 1e-3)
    for env_type in ("lab", "indoor", "gym"):
        assert chk(env_type, 1, 0.2) == (1, 0.2)                  # off: every environment
        with pytest.raises(ValueError, match="host-fed"):
            chk(env_type, 2, 0.2)
    for bad in (0, 17, -1, True, False, 2.0, "2", None):
        with pytest.raises(ValueError, match="reuse_epochs"):
            chk("maze", bad, 0.2)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), True, "0.2", None):
        with pytest.raises(ValueError, match="ppo_clip"):
            chk("maze", 2, bad)
    with pytest.raises(ValueError, match="ppo_clip"):
        chk("maze", 1, 0.0)                                       # checked even when the option is off


def test_trainer_refuses_before_touching_the_device():
    """The constructor checks the options first: no network, no device needed."""
    from unreal_amd.train.trainer import Trainer
    args = (0, None, 7e-4, None, None, "lab", "nav_maze_static_01", True, True, True, True, 0.05, 0.001, 20, 20, 0.99, 0.9,
            2000, 10 ** 6, "cuda:0")
    with pytest.raises(ValueError, match="host-fed"):
        Trainer(*args, reuse_epochs=2)
    with pytest.raises(ValueError, match="reuse_epochs"):
        Trainer(*args, reuse_epochs=0)


def test_flag_names_and_defaults():
    from unreal_amd.options import get_options
    f = get_options("training")
    assert f.reuse_epochs == 1 and f.ppo_clip == 0.2
    g = get_options("training", argv=["--reuse_epochs", "4", "--ppo_clip", "0.1"])
    assert g.reuse_epochs == 4 and isinstance(g.reuse_epochs, int) and g.ppo_clip == 0.1


def test_entry_refuses_bad_arguments_without_launch(built):
    """Fake device pointers: every call below is refused on the host, so none of them reaches a kernel."""
    from unreal_amd import _lib, ops
    L = _lib.lib()
    fn = L._fn["unreal_ppo_heads_loss_grad"]
    dev = 1 << 20
    #       rows A  X    ldx  Wp   bp   Wv   bv   pi_old ld action adv R   active eps  beta  scale pi_out v_out dlogits dv
    good = [8, 4, dev, 256, dev, dev, dev, dev, dev, 4, dev, dev, dev, dev, 0.2, 0.001, 0.25, dev, dev, dev, dev,
            dev, dev, dev]                                        # ... losses, stats_i, stats_f
    assert len(good) == len(L.protos["unreal_ppo_heads_loss_grad"]) - 1

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    bad = [with_(_0=0), with_(_0=-3),                             # rows
           with_(_1=1), with_(_1=19), with_(_1=0),                # A
           with_(_3=255),                                         # ldx < 256
           with_(_9=3),                                           # ld_old < A
           with_(_14=0.0), with_(_14=1.0), with_(_14=-0.2), with_(_14=float("nan")),     # eps outside (0, 1)
           with_(_20=None)]                                       # a gradient asked for without dv
    bad += [with_(**{"_%d" % k: None}) for k in (2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 17, 18, 21, 22, 23)]   # required pointers
    for a in bad:
        assert fn(*a, None) == -22, a
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_ppo_heads_loss_grad", *with_(_0=0), None)
    x = torch.zeros(8 * 256)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ppo_heads_loss_grad(8, 4, x, 256, x, x, x, x, x, 4, x, x, x, x, 0.2, 0.001, 1.0, x, x, x, x, x, x, x)
    with pytest.raises(ValueError, match="clip_eps"):
        ops.ppo_heads_loss_grad(8, 4, x, 256, x, x, x, x, x, 4, x, x, x, x, 1.0, 0.001, 1.0, x, x, x, x, x, x, x)
    with pytest.raises(ValueError, match="rows"):
        ops.ppo_heads_loss_grad(8, 19, x, 256, x, x, x, x, x, 19, x, x, x, x, 0.2, 0.001, 1.0, x, x, x, x, x, x, x)


# ---- hand-derivable rows of the model --------------------------------------------------------------------------------------------
P = np.array([[0.5, 0.3, 0.2]])
BETA, EPS = 0.01, 0.2


def _row(rho, adv, a=0, R=1.5, v=0.25, scale=1.0):
    po = P.copy()
    po[0, a] = P[0, a] / rho
    return PM.ppo_loss(P, [v], po, [a], [adv], [R], [1], EPS, BETA, scale)


def _entropy_only():
    z = torch.tensor(np.log(P), requires_grad=True)
    pi = torch.softmax(z, 1)
    (BETA * (pi * torch.log(pi)).sum()).backward()               # -beta H
    return z.grad.numpy()


def test_model_at_rho_1_is_the_a3c_gradient():
    for adv in (0.7, -1.3):
        for a in (0, 2):
            got = _row(1.0, adv, a=a, scale=0.5)
            z = torch.tensor(np.log(P), requires_grad=True)
            v = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
            pi = torch.softmax(z, 1)
            f64 = lambda x: torch.tensor(x, dtype=torch.float64)
            pl, vl, ent = OM.base_loss(pi, v, f64(np.eye(3)[[a]]), f64([adv]), f64([1.5]), BETA)
            (0.5 * (pl + vl)).backward()
            np.testing.assert_allclose(got["dlogits"], z.grad.numpy(), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(got["dv"], v.grad.numpy(), rtol=1e-12)
            # the surrogate's value at rho = 1 is A, not log pi A: value and entropy are base_loss's, the policy term is its own
            np.testing.assert_allclose(got["losses"][1:], [0.5 * vl.item(), 0.5 * ent.sum().item()], rtol=1e-12)
            np.testing.assert_allclose(got["losses"][0], 0.5 * (-adv - BETA * ent.sum().item()), rtol=1e-12)
            assert got["clipped"] == 0 and got["counted"] == 1 and got["kl_sum"] == 0.0 and got["abs_sum"] == 0.0


@pytest.mark.parametrize("rho,adv", [(1.5, 0.8), (0.5, -0.8)])
def test_model_clipped_rows_keep_only_the_entropy_gradient(rho, adv):
    got = _row(rho, adv)
    np.testing.assert_allclose(got["dlogits"], _entropy_only(), rtol=1e-12, atol=1e-15)
    assert got["clipped"] == 1 and got["counted"] == 1 and not got["unclipped"][0]
    rc = 1 + EPS if rho > 1 else 1 - EPS
    H = -(P * np.log(P)).sum()
    np.testing.assert_allclose(got["losses"][0], -(rc * adv) - BETA * H, rtol=1e-12)
    np.testing.assert_allclose(got["kl_sum"], rho - 1 - np.log(rho), rtol=1e-12)
    np.testing.assert_allclose(got["abs_sum"], abs(rho - 1), rtol=1e-12)
    np.testing.assert_allclose(got["dv"], [-0.5 * (1.5 - 0.25)], rtol=1e-12)


@pytest.mark.parametrize("rho,adv", [(0.5, 0.8), (1.5, -0.8)])
def test_model_unclipped_rows_have_gradient_minus_a_over_p_old(rho, adv):
    got = _row(rho, adv)
    p_old = P[0, 0] / rho
    g = BETA * (np.log(P) + 1.0)
    g[0, 0] += -adv / p_old
    want = P * (g - (P * g).sum())
    np.testing.assert_allclose(got["dlogits"], want, rtol=1e-12, atol=1e-15)
    assert got["clipped"] == 0 and got["counted"] == 1 and got["unclipped"][0]
    H = -(P * np.log(P)).sum()
    np.testing.assert_allclose(got["losses"][0], -(rho * adv) - BETA * H, rtol=1e-12)


@pytest.mark.parametrize("rho", [0.5, 1.0, 1.5])
def test_model_tie_is_unclipped(rho):
    got = _row(rho, 0.0)
    assert got["unclipped"][0] and got["clipped"] == 0 and got["counted"] == 1
    np.testing.assert_allclose(got["dlogits"], _entropy_only(), rtol=1e-12, atol=1e-15)


def test_model_inactive_rows_and_probability_floor():
    p = np.array([[0.6, 0.4], [1.0 - 1e-30, 1e-30], [0.25, 0.75]])
    po = np.array([[0.6, 0.4], [0.5, 1e-25], [0.5, 0.5]])
    got = PM.ppo_loss(p, [0.0, 0.0, 0.0], po, [0, 1, 1], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1, 1, 0], EPS, BETA, 2.0)
    assert (got["dlogits"][2] == 0).all() and got["dv"][2] == 0 and got["counted"] == 2
    assert got["rho"][1] == 1.0                                   # both probabilities sit on the floor
    # below the floor the clip passes no gradient: un = 0, so the action's own term vanishes and only the entropy's log stays
    g = BETA * (np.log(np.clip(p[1], PM.P_LO, 1.0)) + np.array([1.0, 0.0]))
    want = 2.0 * p[1] * (g - (p[1] * g).sum())
    np.testing.assert_allclose(got["dlogits"][1], want, rtol=1e-12, atol=1e-300)


def test_numpy_and_torch_forms_agree():
    rs = np.random.RandomState(0)
    rows, A = 64, 6
    z = rs.normal(0, 2, (rows, A))
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    a = rs.randint(0, A, rows)
    rho = rs.choice([0.3, 0.7, 0.9, 1.0, 1.1, 1.3, 3.0], rows)
    po = p[np.arange(rows), a] / rho
    adv, R, v = rs.normal(0, 1, rows), rs.normal(0, 1, rows), rs.normal(0, 1, rows)
    got = PM.ppo_loss(p, v, po, a, adv, R, np.ones(rows), EPS, BETA, 0.125)
    assert 0 < got["clipped"] < rows and PM.edge_distance(got["rho"], EPS) > 1e-4
    zt = torch.tensor(z, requires_grad=True)
    vt = torch.tensor(v, requires_grad=True)
    pl, vl, ent = PM.surrogate_torch(torch.softmax(zt, 1), vt, torch.tensor(po), torch.tensor(np.eye(A)[a]),
                                     torch.tensor(adv), torch.tensor(R), EPS, BETA)
    (0.125 * (pl + vl)).backward()
    np.testing.assert_allclose(got["losses"], 0.125 * np.array([pl.item(), vl.item(), ent.sum().item()]), rtol=1e-12)
    np.testing.assert_allclose(got["dlogits"], zt.grad.numpy(), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(got["dv"], vt.grad.numpy(), rtol=1e-12)
