"""The Adam applier and advantage normalisation without a GPU: the fp64 model of tests/adam_model.py against
torch.optim and hand answers, the applier's constructor and step counting, the two entries' argument checks, the flags,
Trainer.check_optim_options and the checkpoint round trips."""
import math
import warnings

import numpy as np
import pytest
import torch

try:
    import adam_model as AM
except ImportError:            # imported as tests.<module>
    from tests import adam_model as AM


@pytest.fixture(scope="module")
def built():
    from unreal_amd.build import build_library
    return build_library(verbose=False)


# ---- the model against torch.optim ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.01, 0.3])
def test_model_is_torch_adam_and_adamw(weight_decay):
    """A random state, 5 random gradients, no clipping: torch.optim.Adam (AdamW with decay) in fp64 on CPU tensors."""
    rs = np.random.RandomState(3)
    n, lr, b1, b2, eps = 64, 3e-3, 0.9, 0.999, 1e-8
    x0 = rs.normal(0, 1, n)
    p = torch.tensor(x0.copy(), dtype=torch.float64, requires_grad=True)
    cls = torch.optim.AdamW if weight_decay else torch.optim.Adam
    opt = cls([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=weight_decay)
    model = AM.Adam(n, b1, b2, eps, weight_decay, clip_norm=0.0)
    x = x0.copy()
    for k in range(5):
        g = rs.normal(0, 10.0 ** rs.randint(-3, 2), n)
        p.grad = torch.tensor(g.copy())
        opt.step()
        x = model.step(x, g, lr)["var"]
        assert model.t == k + 1
        np.testing.assert_allclose(x, p.detach().numpy(), rtol=1e-12, atol=0)
    st = opt.state[p]
    np.testing.assert_allclose(model.m, st["exp_avg"].numpy(), rtol=1e-12)
    np.testing.assert_allclose(model.v, st["exp_avg_sq"].numpy(), rtol=1e-12)


# ---- hand answers -----------------------------------------------------------------------------------------------------------------
def test_first_step_moves_by_lr_sign_g():
    g = np.array([3.0, -0.02, 1e-3, -700.0])
    x = np.array([1.0, 2.0, -3.0, 0.5])
    lr, eps = 1e-2, 1e-8
    out = AM.Adam(4, eps=eps, clip_norm=0.0).step(x, g, lr)
    # m / bc1 = g and sqrt(v / bc2) = |g| at t = 1: the step is lr g / (|g| + eps)
    np.testing.assert_allclose(x - out["var"], lr * g / (np.abs(g) + eps), rtol=1e-12)
    np.testing.assert_allclose(x - out["var"], lr * np.sign(g), rtol=2e-5)
    np.testing.assert_allclose(out["m"], 0.1 * g, rtol=1e-12)
    np.testing.assert_allclose(out["v"], 0.001 * g * g, rtol=1e-12)


def test_clip_below_at_above_and_zero_norm():
    g = np.array([3.0, -4.0])                                     # norm 5
    for clip, scale in ((10.0, 1.0), (5.0, 1.0), (2.5, 0.5), (0.0, 1.0), (-1.0, 1.0)):
        assert AM.clip_scale(5.0, clip) == pytest.approx(scale, rel=1e-15)
        out = AM.adam_step(np.zeros(2), np.zeros(2), np.zeros(2), g, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, clip_norm=clip)
        np.testing.assert_allclose(out["g"], g * scale, rtol=1e-15)
    assert AM.clip_scale(0.0, 40.0) == 1.0
    z = AM.adam_step(np.ones(3), np.zeros(3), np.zeros(3), np.zeros(3), 0.1, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, clip_norm=40.0)
    assert (z["var"] == 1.0).all() and (z["m"] == 0).all() and (z["v"] == 0).all()      # 0 / (0 + eps): nothing moves


def test_decay_is_decoupled():
    out = AM.adam_step(np.array([2.0]), np.zeros(1), np.zeros(1), np.zeros(1), 0.1, 0.9, 0.999, 1e-8, 0.5, 0.1, 0.001)
    assert out["var"][0] == 2.0 * (1 - 0.05) and out["m"][0] == 0.0      # the decay does not enter the moments


# ---- AdamApplier ------------------------------------------------------------------------------------------------------------------
def test_applier_constructor_refusals():
    from unreal_amd.train.adam_applier import AdamApplier
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    a = AdamApplier(None)
    assert a.kind == "adam" and RMSPropApplier.kind == "rmsprop" and RMSPropApplier(None).kind == "rmsprop"
    assert (a._beta1, a._beta2, a._epsilon, a._weight_decay, a._clip_norm, a.t) == (0.9, 0.999, 1e-8, 0.0, 40.0, 0)
    assert a.m is None and a.v is None and a.get_slot(None, "m") is None
    AdamApplier(None, beta1=0.0, beta2=0.0, epsilon=1e-3, weight_decay=0.1, clip_norm=0.0)
    nan, inf = float("nan"), float("inf")
    for name, values in (("beta1", (-0.1, 1.0, 1.5, nan, inf, True, "0.9", None)),
                         ("beta2", (-0.1, 1.0, 1.5, nan, inf, True, "0.9", None)),
                         ("epsilon", (0.0, -1e-8, nan, inf, True, None)),
                         ("weight_decay", (-0.01, nan, inf, True, None)),
                         ("clip_norm", (nan, inf, -inf, True, None))):
        for bad in values:
            with pytest.raises(ValueError, match=name):
                AdamApplier(None, **{name: bad})


class _StubOps(object):
    def __init__(self):
        self.calls = []

    def grad_norm(self, grad, scratch, norm):
        self.calls.append(("grad_norm",))

    def adam_step(self, var, m, v, grad, lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip_norm, norm):
        self.calls.append(("adam_step", lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip_norm, norm))


def test_applier_counts_steps_and_passes_fp64_bias_corrections(monkeypatch):
    from unreal_amd.train import adam_applier
    stub = _StubOps()
    monkeypatch.setattr(adam_applier, "ops", stub)
    a = adam_applier.AdamApplier(None, beta1=0.8, beta2=0.99, epsilon=1e-6, weight_decay=0.02, clip_norm=7.0)
    flat, grad = torch.ones(10), torch.ones(10)
    assert a.minimize_local(None, [], [])[0] is a
    for t in range(1, 6):
        norm = a.step(flat, grad, 0.5 / t)
        assert a.t == t and norm is a._norm and norm.numel() == 1
        assert stub.calls[-2] == ("grad_norm",)
        name, lr, b1, b2, eps, wd, bc1, bc2, clip, nm = stub.calls[-1]
        assert (name, lr, b1, b2, eps, wd, clip) == ("adam_step", 0.5 / t, 0.8, 0.99, 1e-6, 0.02, 7.0) and nm is norm
        assert isinstance(bc1, float) and bc1 == 1.0 - 0.8 ** t and bc2 == 1.0 - 0.99 ** t
        assert (bc1, bc2) == AM.bias_corrections(0.8, 0.99, t)
    assert a.get_slot(None, "m") is a.m and a.get_slot(None, "v") is a.v and a.get_slot(None, "rms") is None
    assert a.m.shape == flat.shape and float(a.m.abs().max()) == 0.0 and float(a.v.abs().max()) == 0.0
    a.t = 999
    a.step(flat, grad, 0.1)
    assert a.t == 1000 and stub.calls[-1][6:8] == (1.0 - 0.8 ** 1000, 1.0 - 0.99 ** 1000)


# ---- the C entries' refusals ------------------------------------------------------------------------------------------------------
def _with(good, **kw):
    a = list(good)
    for k, v in kw.items():
        a[int(k[1:])] = v
    return a


def test_adam_entry_refuses_bad_arguments_without_launch(built):
    """Fake device pointers: every call below is refused on the host, so none of them reaches a kernel."""
    from unreal_amd import _lib, ops
    L = _lib.lib()
    fn = L._fn["unreal_adam_step"]
    dev = 1 << 20
    nan, inf = float("nan"), float("inf")
    #       var  m    v    grad n     lr    b1   b2     eps   wd   bc1  bc2    clip  norm
    good = [dev, dev, dev, dev, 1000, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 40.0, dev]
    assert len(good) == len(L.protos["unreal_adam_step"]) - 1
    bad = [_with(good, **{"_%d" % k: None}) for k in (0, 1, 2, 3, 13)]                  # required pointers
    bad += [_with(good, _4=0), _with(good, _4=-8)]                                      # n
    bad += [_with(good, **{"_%d" % k: dev + 4}) for k in (0, 1, 2, 3)]                  # not 16-byte aligned
    bad += [_with(good, **{"_%d" % k: x}) for k in (6, 7) for x in (-0.1, 1.0, 1.5)]    # betas outside [0, 1)
    bad += [_with(good, _8=0.0), _with(good, _8=-1e-8), _with(good, _9=-0.01)]          # eps <= 0, weight_decay < 0
    bad += [_with(good, **{"_%d" % k: x}) for k in (10, 11) for x in (0.0, -0.5, 1.0001)]        # bc outside (0, 1]
    bad += [_with(good, **{"_%d" % k: x}) for k in (5, 6, 7, 8, 9, 10, 11, 12) for x in (nan, inf)]     # non-finite scalars
    for a in bad:
        assert fn(*a, None) == -22, a
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_adam_step", *_with(good, _4=0), None)
    x = torch.zeros(16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.adam_step(x, x, x, x, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 40.0, x)


def test_adv_normalize_entry_refuses_bad_arguments_without_launch(built):
    from unreal_amd import _lib, ops
    L = _lib.lib()
    fn = L._fn["unreal_adv_normalize"]
    dev = 1 << 20
    #       rows adv  active eps   adv_out     stats
    good = [100, dev, dev, 1e-8, dev + 4096, dev + 8192]
    assert len(good) == len(L.protos["unreal_adv_normalize"]) - 1
    bad = [_with(good, _0=0), _with(good, _0=-5)]
    bad += [_with(good, **{"_%d" % k: None}) for k in (1, 2, 4, 5)]
    bad += [_with(good, _3=x) for x in (0.0, -1e-8, float("nan"), float("inf"))]
    bad += [_with(good, _4=dev)]                                                        # adv_out aliases adv
    for a in bad:
        assert fn(*a, None) == -22, a
    x, i = torch.zeros(8), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.adv_normalize(8, x, i, 1e-8, x.clone(), x)
    with pytest.raises(ValueError, match="rows"):
        ops.adv_normalize(0, x, i, 1e-8, x.clone(), x)
    for eps in (0.0, float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="eps"):
            ops.adv_normalize(8, x, i, eps, x.clone(), x)


# ---- flags and trainer options ----------------------------------------------------------------------------------------------------
def test_flag_names_and_defaults():
    from unreal_amd.options import get_options
    f = get_options("training")
    assert f.optimizer == "rmsprop" and f.normalize_advantages is False
    assert (f.adam_beta1, f.adam_beta2, f.adam_epsilon, f.weight_decay) == (0.9, 0.999, 1e-8, 0.0)
    g = get_options("training", argv=["--optimizer", "adam", "--adam_beta1", "0.8", "--adam_beta2", "0.99", "--adam_epsilon",
                                      "1e-5", "--weight_decay", "0.01", "--normalize_advantages", "true"])
    assert g.optimizer == "adam" and g.normalize_advantages is True
    assert (g.adam_beta1, g.adam_beta2, g.adam_epsilon, g.weight_decay) == (0.8, 0.99, 1e-5, 0.01)
    with pytest.raises(SystemExit):
        get_options("training", argv=["--optimizer", "sgd"])
    assert not hasattr(get_options("evaluate"), "optimizer")


def test_check_optim_options():
    from unreal_amd.train.trainer import Trainer
    chk = Trainer.check_optim_options
    assert chk(False) == (False, 1e-8) and chk(True, 1e-5) == (True, 1e-5) and chk(True, 1) == (True, 1.0)
    for bad in (0, 1, None, "true", 1.0):
        with pytest.raises(ValueError, match="normalize_advantages"):
            chk(bad)
    for bad in (0.0, -1e-8, float("nan"), float("inf"), True, "1e-8", None):
        with pytest.raises(ValueError, match="adv_norm_eps"):
            chk(True, bad)
    with pytest.raises(ValueError, match="adv_norm_eps"):
        chk(False, 0.0)                                           # checked even when the option is off


def test_trainer_refuses_before_touching_the_device():
    """The constructor checks the options first: no network, no device needed; host-fed environments may normalise."""
    from unreal_amd.train.trainer import Trainer
    args = (0, None, 7e-4, None, None, "lab", "nav_maze_static_01", True, True, True, True, 0.05, 0.001, 20, 20, 0.99, 0.9,
            2000, 10 ** 6, "cuda:0")
    with pytest.raises(ValueError, match="normalize_advantages"):
        Trainer(*args, normalize_advantages=1)
    with pytest.raises(ValueError, match="adv_norm_eps"):
        Trainer(*args, normalize_advantages=True, adv_norm_eps=0.0)
    with pytest.raises(NotImplementedError, match="simulator"):    # past the option checks: what a host-fed trainer needs next
        Trainer(*args, normalize_advantages=True)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------
class _Net(object):
    def __init__(self):
        from unreal_amd.model.model import FlatParams, param_spec
        self.spec = param_spec(4)
        self.params = FlatParams(self.spec, "cpu")
        self.params.flat.copy_(torch.arange(self.params.size, dtype=torch.float32) * 1e-6)


def _adam(net, t=0):
    from unreal_amd.train.adam_applier import AdamApplier
    a = AdamApplier(None, device="cpu")
    a._create_slots(net.params.flat)
    if t:
        a.m.copy_(torch.linspace(-1, 1, a.m.numel()))
        a.v.copy_(torch.linspace(0, 3, a.v.numel()))
        a.t = t
    return a


def _rmsprop(net, touched=False):
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    a = RMSPropApplier(None, device="cpu")
    a._create_slots(net.params.flat)
    if touched:
        a.ms.mul_(0.5)
        a.mom.add_(0.25)
    return a


def test_checkpoint_adam_to_adam(tmp_path):
    from unreal_amd import checkpoint as ck
    d = str(tmp_path / "ckpt")
    net, app = _Net(), _adam(_Net(), t=37)
    path = ck.save(d, net, app, global_t=100, wall_t=1.5, best_score=-0.5)
    payload = torch.load(path, map_location="cpu", weights_only=True)
    assert payload["optimizer"] == "adam" and payload["adam_t"] == 37
    assert payload["rms"] is None and payload["momentum"] is None
    assert torch.equal(payload["adam_m"], app.m) and torch.equal(payload["adam_v"], app.v)
    net2, app2 = _Net(), _adam(_Net())
    net2.params.flat.zero_()
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)               # an Adam checkpoint into an Adam applier: nothing to warn of
        assert ck.restore(d, net2, app2) == (100, 1.5, -0.5)
    assert torch.equal(net2.params.flat, net.params.flat)
    assert torch.equal(app2.m, app.m) and torch.equal(app2.v, app.v) and app2.t == 37
    app3 = _adam(_Net(), t=5)
    with pytest.warns(UserWarning, match="restore_slots=False"):
        ck.restore(d, _Net(), app3, restore_slots=False)
    assert float(app3.m.abs().max()) == 0.0 and float(app3.v.abs().max()) == 0.0 and app3.t == 0


def test_checkpoint_rmsprop_to_adam_and_back(tmp_path):
    from unreal_amd import checkpoint as ck
    d = str(tmp_path / "rms")
    net = _Net()
    rms = _rmsprop(net, touched=True)
    path = ck.save(d, net, rms, global_t=200, wall_t=2.0)
    payload = torch.load(path, map_location="cpu", weights_only=True)
    assert payload["optimizer"] == "rmsprop" and "adam_m" not in payload and "adam_t" not in payload
    assert torch.equal(payload["rms"], rms.ms) and torch.equal(payload["momentum"], rms.mom)     # today's keys, today's values
    app = _adam(_Net(), t=9)
    with pytest.warns(UserWarning, match="no Adam slots"):
        assert ck.restore(d, _Net(), app)[0] == 200
    assert float(app.m.abs().max()) == 0.0 and float(app.v.abs().max()) == 0.0 and app.t == 0
    rms2 = _rmsprop(_Net())
    ck.restore(d, _Net(), rms2)
    assert torch.equal(rms2.ms, rms.ms) and torch.equal(rms2.mom, rms.mom)
    # Adam -> RMSProp: the slots restart at 1 / 0
    d2 = str(tmp_path / "adam")
    ck.save(d2, net, _adam(net, t=3), global_t=300, wall_t=3.0)
    rms3 = _rmsprop(_Net(), touched=True)
    assert ck.restore(d2, _Net(), rms3)[0] == 300
    assert float(rms3.ms.min()) == 1.0 and float(rms3.ms.max()) == 1.0 and float(rms3.mom.abs().max()) == 0.0


def test_checkpoint_without_optimizer_key_loads_as_rmsprop(tmp_path):
    from unreal_amd import checkpoint as ck
    d = str(tmp_path / "old")
    net = _Net()
    rms = _rmsprop(net, touched=True)
    path = ck.save(d, net, rms, global_t=100, wall_t=1.0)
    payload = torch.load(path, map_location="cpu", weights_only=True)
    del payload["optimizer"]                                      # a file written before the key existed
    torch.save(payload, path)
    rms2 = _rmsprop(_Net())
    assert ck.restore(d, _Net(), rms2)[0] == 100
    assert torch.equal(rms2.ms, rms.ms) and torch.equal(rms2.mom, rms.mom)
    app = _adam(_Net(), t=4)
    with pytest.warns(UserWarning, match="'rmsprop' checkpoint"):
        ck.restore(d, _Net(), app)
    assert app.t == 0 and float(app.m.abs().max()) == 0.0
    # no applier at all: saved and restored as before
    p2 = ck.save(str(tmp_path / "none"), net, None, global_t=100, wall_t=1.0)
    payload = torch.load(p2, map_location="cpu", weights_only=True)
    assert payload["optimizer"] == "rmsprop" and payload["rms"] is None
    assert ck.restore(str(tmp_path / "none"), _Net())[0] == 100


# ---- the normalisation model ------------------------------------------------------------------------------------------------------
def test_normalisation_model():
    rs = np.random.RandomState(5)
    x = rs.normal(0.3, 2.0, 57)
    eps = 1e-8
    out, mean, std, n = AM.adv_normalize(x, np.ones(57), eps)
    np.testing.assert_allclose(out, (x - x.mean()) / (x.std() + eps), rtol=1e-12, atol=1e-15)
    assert n == 57 and mean == pytest.approx(x.mean(), rel=1e-14) and std == pytest.approx(x.std(), rel=1e-14)
    active = (np.arange(57) % 3 != 1).astype(np.int32)
    out, mean, std, n = AM.adv_normalize(x, active, eps)
    on = active.astype(bool)
    assert n == on.sum() and (out[~on] == 0).all()
    np.testing.assert_allclose(out[on], (x[on] - x[on].mean()) / (x[on].std() + eps), rtol=1e-12, atol=1e-15)
    assert abs(out[on].mean()) < 1e-12 and out[on].std() == pytest.approx(1.0, rel=1e-6)
    one = np.zeros(57, np.int32)
    one[11] = 1
    out, mean, std, n = AM.adv_normalize(x, one, eps)
    assert n == 1 and out[11] == x[11] and np.count_nonzero(out) == 1 and mean == x[11] and std == 0.0
    out, mean, std, n = AM.adv_normalize(x, np.zeros(57), eps)
    assert n == 0 and (out == 0).all() and (mean, std) == (0.0, 0.0)
    out, mean, std, n = AM.adv_normalize(np.full(57, 2.5), active, eps)
    assert (out == 0).all() and mean == 2.5 and std == 0.0
    # where E[x^2] - E[x]^2 fails: fp32 advantages at 1e4 with noise of 1e-2 keep their spread in two passes
    big = (1e4 + rs.normal(0, 1e-2, 57)).astype(np.float32)
    out, mean, std, n = AM.adv_normalize(big, np.ones(57), eps)
    assert 5e-3 < std < 2e-2 and out.std() == pytest.approx(1.0, rel=1e-6) and math.isfinite(out.max())
