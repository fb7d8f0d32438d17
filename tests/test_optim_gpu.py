"""The Adam applier and advantage normalisation on the device: unreal_adam_step and unreal_adv_normalize against
the fp64 model of tests/adam_model.py, the trainer's Adam updates replayed through that model from its own buffers, the
normalised advantages where the policy loss reads them, and one full-UNREAL run with every option of §7o-§7s on.

Bars of one Adam step, from counting fp32 roundings at 2^-24 each: v at rel 1e-6; m within 1e-6 (|beta1 m0| + |(1 - beta1) g|)
(the two terms can cancel, so the bar is on the terms); var within 2^-23 |var| + 1e-5 |update|.  The model is fed what the
kernel is fed: the fp32 scalars and the device's norm."""
import numpy as np
import pytest
import torch

try:
    import adam_model as AM
    import margins
    import maze_model as MM
    import test_reuse_gpu as RG
    import timelimit_cases as TC
except ImportError:            # imported as tests.<module>
    from tests import adam_model as AM
    from tests import margins
    from tests import maze_model as MM
    from tests import test_reuse_gpu as RG
    from tests import timelimit_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = lambda x: float(np.float32(x))
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _check_step(what, got, want, m0, times=1.0):
    """got = (var, m, v) of the device, want = the model's dict for the same inputs, m0 the first moment before the step.
    -> the worst |error| / bar of the three."""
    var, m, v = (np.asarray(x, np.float64) for x in got)
    bars = dict(v=1e-6 * np.abs(want["v"]),
                m=1e-6 * (np.abs(want["beta1"] * m0) + np.abs((1.0 - want["beta1"]) * want["g"])),
                var=2.0 ** -23 * np.abs(want["var"]) + 1e-5 * np.abs(want["update"]))
    worst = 0.0
    for name, g in (("v", v), ("m", m), ("var", var)):
        err, bar = np.abs(g - want[name]), times * bars[name]
        ratio = float((err / np.maximum(bar, 1e-300)).max()) if (err > 0).any() else 0.0
        margins.record("%s %s" % (what, name), ratio, {"v": "rel 1e-6", "m": "1e-6 (|b1 m0| + |(1 - b1) g|)",
                                                       "var": "2^-23 |var| + 1e-5 |update|"}[name])
        k = int(np.argmax(err / np.maximum(bar, 1e-300)))
        print("%s: %s worst |error| / bar %.3f at %d: got %.9g want %.9g (m0 %.9g g %.9g v %.9g update %.9g)" % (
            what, name, ratio, k, g[k], want[name][k], m0[k], want["g"][k], want["v"][k], want["update"][k]))
        assert (err <= bar).all(), (what, name, ratio, int((err > bar).sum()))
        worst = max(worst, ratio)
    return worst


def _model_step(var, m, v, grad, lr, beta1, beta2, eps, wd, bc1, bc2, clip, norm):
    """The model on the kernel's inputs: every scalar as the fp32 the entry receives."""
    out = AM.adam_step(var, m, v, grad, F32(lr), F32(beta1), F32(beta2), F32(eps), F32(wd), F32(bc1), F32(bc2), F32(clip),
                       norm)
    out["beta1"] = F32(beta1)
    return out


# ---- 1. unreal_adam_step ----------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 1023, 2048 * 256 * 4 + 4 * 256 + 3]           # the last: once round the grid-stride loop + a 3-element tail


def _state(n, seed, zero_grad=False):
    rs = np.random.RandomState(seed)
    var = rs.normal(0, 1, n).astype(np.float32)
    m = (rs.normal(0, 0.3, n) * (1 + (np.arange(n) % 3 == 0))).astype(np.float32)      # non-zero, both signs against g
    v = rs.uniform(1e-3, 2.0, n).astype(np.float32)                                    # positive
    g = np.zeros(n, np.float32) if zero_grad else rs.normal(0, 1, n).astype(np.float32)
    return var, m, v, g


@pytest.mark.parametrize("clip", ["below", "above", "off", "zero_grad"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_against_fp64(n, clip):
    """One step from non-zero m and positive v at t in {1, 2, 1000} and weight_decay in {0, 0.01}; the norm below and above
    clip_norm, clip_norm = 0 with a null norm, and an all-zero gradient (norm 0: scale 1)."""
    from unreal_amd import ops
    var0, m0, v0, g = _state(n, n % 9973 + len(clip), zero_grad=clip == "zero_grad")
    scratch, norm = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)
    gd = _dev(g)
    ops.grad_norm(gd, scratch, norm)
    nv = float(norm.cpu()[0])
    exact = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    assert abs(nv - exact) <= 1e-5 * exact
    clip_norm = dict(below=2.0 * exact, above=0.5 * exact, off=0.0, zero_grad=40.0)[clip]
    if n >= 1023 and clip != "zero_grad":
        assert ((m0 * g) > 0).any() and ((m0 * g) < 0).any()
    for t in (1, 2, 1000):
        for wd in (0.0, 0.01):
            bc1, bc2 = AM.bias_corrections(B1, B2, t)
            var, m, v = _dev(var0), _dev(m0), _dev(v0)
            ops.adam_step(var, m, v, gd, LR, B1, B2, EPS, wd, bc1, bc2, clip_norm, None if clip == "off" else norm)
            want = _model_step(var0, m0, v0, g, LR, B1, B2, EPS, wd, bc1, bc2, clip_norm, nv)
            if clip == "above":
                assert want["g"][0] == pytest.approx(0.5 * g[0], rel=1e-5)
            else:                                                 # (clip_norm * (1 / clip_norm) is 1 but for a rounding)
                np.testing.assert_allclose(want["g"], g, rtol=1e-15, atol=0)
            _check_step("adam n=%d %s t=%d wd=%g" % (n, clip, t, wd), (_f64(var), _f64(m), _f64(v)), want, m0)
            assert torch.equal(gd, _dev(g))                       # the gradient is read only
            if clip == "zero_grad":
                assert (_f64(v) <= v0).all() and (np.abs(_f64(m)) <= np.abs(m0)).all()


def test_adam_five_steps_against_fp64():
    """Five successive steps at n = 1023 (t = 1..5, weight decay on, clipped): the device and the model each carry their own
    state from the same start and see the same gradients and norms; the one-step bars times 5, the update's term summed."""
    from unreal_amd import ops
    n, wd, clip_norm = 1023, 0.01, 20.0
    var0, m0, v0, _ = _state(n, 77)
    var, m, v = _dev(var0), _dev(m0), _dev(v0)
    scratch, norm = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)
    mv, mm, mvv = var0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    rs = np.random.RandomState(78)
    moved = np.zeros(n)
    for t in range(1, 6):
        g = rs.normal(0, 10.0 ** (t % 3 - 1), n).astype(np.float32)
        gd = _dev(g)
        ops.grad_norm(gd, scratch, norm)
        bc1, bc2 = AM.bias_corrections(B1, B2, t)
        ops.adam_step(var, m, v, gd, LR, B1, B2, EPS, wd, bc1, bc2, clip_norm, norm)
        m_prev = mm
        want = _model_step(mv, mm, mvv, g, LR, B1, B2, EPS, wd, bc1, bc2, clip_norm, float(norm.cpu()[0]))
        mv, mm, mvv = want["var"], want["m"], want["v"]
        moved += np.abs(want["update"])
    want["update"] = moved / 5.0                                  # times 5 below: the sum of the five updates
    _check_step("adam five steps", (_f64(var), _f64(m), _f64(v)), want, m_prev, times=5.0)


def test_adam_without_decay_skips_the_decay_line():
    """weight_decay = 0: bit-identical to the call on parameters pre-multiplied by 1, and a step that moves nothing (zero
    gradient, zero m) returns every parameter bit for bit -- -0, subnormals and the largest float included --, where the
    same call with a decay changes them."""
    from unreal_amd import ops
    n = 1027
    var0, m0, v0, g = _state(n, 5)
    var0[:6] = [-0.0, 0.0, 1e-40, -1e-45, 3.4028235e38, -1.1754944e-38]
    scratch, norm = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)
    gd = _dev(g)
    ops.grad_norm(gd, scratch, norm)
    outs = []
    for pre in (None, 1.0):
        var, m, v = _dev(var0), _dev(m0), _dev(v0)
        if pre is not None:
            var = (var * pre).contiguous()
        ops.adam_step(var, m, v, gd, LR, B1, B2, EPS, 0.0, 0.1, 0.001, 40.0, norm)
        outs.append([x.cpu().numpy().view(np.uint32).copy() for x in (var, m, v)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    zero = torch.zeros(n, device=DEV)
    for wd, same in ((0.0, True), (0.01, False)):
        var, m, v = _dev(var0), torch.zeros(n, device=DEV), _dev(v0)
        ops.adam_step(var, m, v, zero, LR, B1, B2, EPS, wd, 0.1, 0.001, 0.0, None)
        bits, bits0 = var.cpu().numpy().view(np.uint32), var0.view(np.uint32)
        if same:
            np.testing.assert_array_equal(bits, bits0)
        else:
            assert (bits != bits0).sum() > n // 2
            np.testing.assert_allclose(var.cpu().numpy()[6:], var0[6:] * (1 - LR * wd), rtol=2e-7)
        assert float(m.abs().max()) == 0.0


# ---- 2. unreal_adv_normalize ------------------------------------------------------------------------------------------------------
ROWS = [1, 2, 5, 257, 1025, 81920]
STATS0 = np.array([0.5, 0.25, 3.0], np.float32)


def _masks(rows, rs):
    one = np.zeros(rows, np.int32)
    one[rows // 2] = 1
    return dict(random=(rs.uniform(size=rows) < 0.6).astype(np.int32) * rs.randint(1, 5, rows).astype(np.int32),
                all=np.ones(rows, np.int32), none=np.zeros(rows, np.int32), one=one)


@pytest.mark.parametrize("mask", ["random", "all", "none", "one"])
@pytest.mark.parametrize("rows", ROWS)
def test_adv_normalize_against_fp64(rows, mask):
    """Random, constant and 1e4 + 1e-2 noise advantages under one mask kind; stats start non-zero; the kernel works in fp64
    and rounds once: one fp32 unit of max(1, |want|).  Two calls on the same input are bit-identical."""
    from unreal_amd import ops
    rs = np.random.RandomState(rows + len(mask))
    active = _masks(rows, rs)[mask]
    data = dict(random=rs.normal(0.3, 2.0, rows), constant=np.full(rows, -1.75), offset=1e4 + rs.normal(0, 1e-2, rows))
    eps = 1e-8
    for kind, x in data.items():
        adv = x.astype(np.float32)
        want, mean, std, n = AM.adv_normalize(adv, active, F32(eps))
        assert n == int((active != 0).sum())
        outs = []
        for rep in range(2):
            out = torch.full((rows,), 9.0, device=DEV)
            stats = _dev(STATS0)
            ad = _dev(adv)
            ops.adv_normalize(rows, ad, _dev(active, torch.int32), eps, out, stats)
            assert torch.equal(ad, _dev(adv))                     # the raw advantages stay
            outs.append((out.cpu().numpy(), stats.cpu().numpy()))
        np.testing.assert_array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
        np.testing.assert_array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
        got, st = outs[0][0].astype(np.float64), outs[0][1].astype(np.float64)
        bar = 2.0 ** -23 * np.maximum(1.0, np.abs(want))
        ratio = float((np.abs(got - want) / bar).max())
        margins.record("adv_normalize rows=%d %s %s" % (rows, mask, kind), ratio, "2^-23 max(1, |want|)")
        print("rows=%d %s %s: n=%d mean %.9g std %.9g, worst |error| / bar %.3f" % (rows, mask, kind, n, mean, std, ratio))
        assert (np.abs(got - want) <= bar).all(), ratio
        want_st = STATS0.astype(np.float64) + [mean, std, 1.0]
        assert (np.abs(st - want_st) <= 1e-6 * np.abs(want_st)).all(), (st, want_st)
        on = active != 0
        assert (got[~on] == 0).all()
        if n < 2:
            np.testing.assert_array_equal(outs[0][0][on], adv[on])                    # a single row keeps its advantage
        elif std == 0.0:
            assert (got == 0).all()
        else:
            assert kind != "constant"
            assert abs(got[on].mean()) < 1e-6 and got[on].std() == pytest.approx(1.0, rel=1e-4)
            if kind == "offset" and n >= 100:
                assert 2e-3 < std < 5e-2                          # E[x^2] - E[x]^2 in fp32 would have no digit of this left


@pytest.mark.parametrize("rows", [5, 1025, 4099])
def test_adv_normalize_does_not_depend_on_alignment(rows):
    """Pointers that are not 16-byte aligned take scalar loads over the same rows in the same order: the same bits."""
    from unreal_amd import ops
    rs = np.random.RandomState(rows)
    adv = rs.normal(0, 3, rows).astype(np.float32)
    active = (rs.uniform(size=rows) < 0.7).astype(np.int32)
    outs = []
    for shift in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)):
        a, m, o = (torch.zeros(rows + 4, dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.float32))
        a, m, o = a[shift[0]:shift[0] + rows], m[shift[1]:shift[1] + rows], o[shift[2]:shift[2] + rows]
        a.copy_(_dev(adv))
        m.copy_(_dev(active, torch.int32))
        stats = torch.zeros(3, device=DEV)
        ops.adv_normalize(rows, a, m, 1e-8, o, stats)
        outs.append((o.cpu().numpy().view(np.uint32), stats.cpu().numpy().view(np.uint32)))
    for o, st in outs[1:]:
        np.testing.assert_array_equal(o, outs[0][0])
        np.testing.assert_array_equal(st, outs[0][1])
    want = AM.adv_normalize(adv, active, F32(1e-8))[0]
    assert (np.abs(outs[0][0].view(np.float32) - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want))).all()


# ---- 3. the trainer with Adam ------------------------------------------------------------------------------------------------------
ENV_NAME = "optim_gpu_fp7"


@pytest.fixture
def fp7():
    """First-person N = 7 with a step limit of 3 (tests/test_reuse_gpu.py's configuration, under its own name)."""
    from unreal_amd.environment.environment import Environment
    rs = np.random.RandomState(7)
    Environment.register_maze_config(ENV_NAME, [MM.random_layout(7, rs, marks="") for _ in range(2)], view="first_person",
                                     random_start=True, random_goal=True, max_episode_steps=3)
    yield Environment.MAZE_CONFIG[ENV_NAME]
    Environment.MAZE_CONFIG.pop(ENV_NAME, None)


ADAM = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.01, clip_norm=40.0)


def _build(Bn, T, Hn, lstm, aux=False, groups=1, env=("maze", ENV_NAME), lr0=7.0711e-4, seed=21, net_seed=4, adam=None,
           fill=True, **options):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.adam_applier import AdamApplier
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    A = Environment.get_action_size(*env)
    net = UnrealModel(A, 0, -1, lstm, aux, aux, aux, 0.05, 0.001, DEV, seed=net_seed)
    applier = AdamApplier(None, device=DEV, **adam) if adam is not None else \
        RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    tr = Trainer(0, net, lr0, None, applier, env[0], env[1], lstm, aux, aux, aux, 0.05, 0.001, T, T, 0.99, 0.9, Hn,
                 10 ** 6, DEV, batch_size=Bn, groups=groups, seed=seed, **options)
    if fill:
        tr.prepare()
        while not tr._full:
            tr.process(None, 0)
    return net, applier, tr


def _record_steps(applier, log):
    """Wrap applier.step: (parameters, m, v before, gradient, lr, t) and (norm, parameters, m, v after) of every call."""
    inner = applier.step

    def step(flat_params, flat_grad, lr):
        z = lambda x: torch.zeros_like(flat_params) if x is None else x.clone()
        rec = dict(var0=flat_params.clone(), m0=z(applier.m), v0=z(applier.v), grad=flat_grad.clone(), lr=lr, t=applier.t + 1)
        norm = inner(flat_params, flat_grad, lr)
        rec.update(norm=norm.clone(), var=flat_params.clone(), m=applier.m.clone(), v=applier.v.clone())
        log.append(rec)
        return norm
    applier.step = step


def _replay(what, rec, hp, got=None):
    """One recorded update through the model -> worst |error| / bar; `got`: another device result for the same inputs."""
    bc1, bc2 = AM.bias_corrections(hp["beta1"], hp["beta2"], rec["t"])
    m0 = _f64(rec["m0"])
    want = _model_step(_f64(rec["var0"]), m0, _f64(rec["v0"]), _f64(rec["grad"]), rec["lr"], hp["beta1"], hp["beta2"],
                       hp["epsilon"], hp["weight_decay"], bc1, bc2, hp["clip_norm"], float(rec["norm"].cpu()[0]))
    got = got if got is not None else (rec["var"], rec["m"], rec["v"])
    return _check_step(what, tuple(_f64(x) for x in got), want, m0)


@pytest.mark.parametrize("reuse", [1, 2])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("lstm", [True, False])
def test_trainer_adam_updates_replay_through_the_model(fp7, tmp_path, lstm, groups, reuse):
    """4 actors, T = 5, history 50: every update of three process() calls, from the device's state before it; the step count;
    and a checkpoint of call 2 restored into a fresh trainer and applier, which then makes call 3's first update."""
    from unreal_amd import checkpoint as ck
    net, applier, tr = _build(4, 5, 50, lstm, groups=groups, adam=ADAM, reuse_epochs=reuse)
    assert applier.t == 0 and applier.kind == "adam"
    log = []
    _record_steps(applier, log)
    per_call = groups * reuse
    for call in range(3):
        steps, _ = tr.process(None, call * 20)
        assert steps > 0 and applier.t == (call + 1) * per_call and len(log) == applier.t
        for k, rec in enumerate(log[call * per_call:]):
            assert rec["t"] == call * per_call + k + 1 and float(rec["norm"].cpu()[0]) > 0
            _replay("trainer adam lstm=%s G=%d E=%d call %d update %d" % (lstm, groups, reuse, call, k), rec, ADAM)
        assert all(np.isfinite(v) for v in tr.last_losses.values())
        if call == 1:
            ck.save(str(tmp_path), net, applier, global_t=40, wall_t=1.0)
    assert bool((applier.get_slot(None, "v") > 0).any()) and applier.get_slot(None, "m") is applier.m
    # restored: parameters, m, v and t of the end of call 2; fed call 3's first gradient it makes call 3's first update
    net2, applier2, tr2 = _build(4, 5, 50, lstm, groups=groups, adam=ADAM, reuse_epochs=reuse, net_seed=9, fill=False)
    assert ck.restore(str(tmp_path), tr2.local_network, tr2.grad_applier)[0] == 40
    rec = log[2 * per_call]
    assert applier2.t == 2 * per_call and torch.equal(net2.params.flat, rec["var0"])
    assert torch.equal(applier2.m, rec["m0"]) and torch.equal(applier2.v, rec["v0"])
    norm = applier2.step(net2.params.flat, rec["grad"], rec["lr"])
    assert applier2.t == rec["t"] and torch.equal(norm, rec["norm"])
    _replay("restored lstm=%s G=%d E=%d" % (lstm, groups, reuse), rec, ADAM, got=(net2.params.flat, applier2.m, applier2.v))
    assert torch.equal(net2.params.flat, rec["var"])              # the same kernel on the same bits


# ---- 4. the trainer with normalised advantages ------------------------------------------------------------------------------------
def _adv_bar(want):
    return 2.0 ** -23 * np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize("lstm,groups", [(True, 1), (False, 2)])
def test_trainer_normalises_what_the_policy_loss_reads(fp7, lstm, groups):
    """normalize_advantages on, 4 actors: after every group's gradients adv_norm is the model of the read-back adv and
    active_log, the loss kernel re-run on the trainer's buffers with adv_norm gives its dlogits / dv bit for bit (and with
    the raw advantages does not), and adv_mean / adv_std are the means over the call's groups."""
    from unreal_amd import ops
    net, applier, tr = _build(4, 5, 50, lstm, groups=groups, normalize_advantages=True, adv_norm_eps=1e-6)
    Bg, T, A = tr.Bg, 5, tr.action_size
    rows = T * Bg
    assert tr.adv_norm.numel() == rows and tr.adv_stats.numel() == 3
    seen = []
    apply_update = tr._apply_update

    def snapshot(lr):                                             # called by process() right after a group's gradients
        adv, on = tr.adv.cpu().numpy(), tr.active_log.cpu().numpy()
        want, mean, std, n = AM.adv_normalize(adv, on, F32(1e-6))
        got = tr.adv_norm.cpu().numpy().astype(np.float64)
        assert n >= 2 and (np.abs(got - want) <= _adv_bar(want)).all()
        assert (got[on == 0] == 0).all() and np.abs(got - adv).max() > 1e-3
        f = lambda k: torch.full((k,), 7.0, device=DEV)
        dl, dv, losses = f(rows * A), f(rows), torch.zeros(3, device=DEV)
        ops.base_loss_grad(rows, A, tr.pi, A, tr.v, tr.actions, tr.adv_norm, tr.R, tr.active_log, tr.entropy_beta,
                           tr.grad_scale, dl, dv, losses)
        assert torch.equal(dl, tr.dlogits[:rows * A]) and torch.equal(dv, tr.dv[:rows])
        assert torch.equal(losses, tr.losses[:3])
        ops.base_loss_grad(rows, A, tr.pi, A, tr.v, tr.actions, tr.adv, tr.R, tr.active_log, tr.entropy_beta,
                           tr.grad_scale, dl, dv, losses)
        assert not torch.equal(dl, tr.dlogits[:rows * A]) and torch.equal(dv, tr.dv[:rows])     # the value loss reads R
        seen.append((mean, std))
        apply_update(lr)

    tr._apply_update = snapshot
    for call in range(2):
        del seen[:]
        tr.process(None, call * 20)
        assert len(seen) == groups
        l = tr.last_losses
        mean, std = np.mean([s[0] for s in seen]), np.mean([s[1] for s in seen])
        assert abs(l["adv_mean"] - mean) <= 1e-6 * max(abs(mean), std) and abs(l["adv_std"] - std) <= 1e-6 * std
        assert std > 0 and all(np.isfinite(v) for v in l.values())


def test_trainer_normalisation_leaves_adv_and_R_raw(fp7):
    """One actor, auxiliary heads off (the case in which two runs repeat bit for bit, tests/test_reuse_gpu.py): the first
    rollout of a trainer with the option on and of its twin with it off leave the same adv and R, bit for bit."""
    kept = []
    for on in (True, False):
        net, applier, tr = _build(1, 5, 16, True, normalize_advantages=on)
        tr._select_group(0)
        tr.compute_gradients()
        kept.append((tr.adv.clone(), tr.R.clone(), tr.active_log.clone()))
        if on:
            want, _, _, n = AM.adv_normalize(tr.adv.cpu().numpy(), tr.active_log.cpu().numpy(), F32(1e-8))
            assert n >= 2 and (np.abs(tr.adv_norm.cpu().numpy() - want) <= _adv_bar(want)).all()
    for a, b in zip(*kept):
        assert torch.equal(a, b)
    assert int(kept[0][2].sum()) >= 2


OPTIM_BUFFERS = ("adv_norm", "adv_stats")
OPTIM_KEYS = ("adv_mean", "adv_std")


def test_option_off_is_todays_trainer(fp7):
    """normalize_advantages=False against no argument at all, one actor: today's keys, nothing allocated, the same parameters
    bit for bit after three calls."""
    flats, keys = [], []
    for options in (dict(normalize_advantages=False, adv_norm_eps=1e-3), {}):
        net, applier, tr = _build(1, 5, 16, True, **options)
        for it in range(3):
            steps, _ = tr.process(None, 0)
            assert steps > 0
        assert tr.normalize_advantages is False and not any(hasattr(tr, name) for name in OPTIM_BUFFERS)
        assert not any(k in tr.last_losses for k in OPTIM_KEYS)
        flats.append(net.params.flat.cpu().numpy().copy())
        keys.append(sorted(tr.last_losses))
    assert keys[0] == keys[1] == sorted(["total_loss", "base_loss", "policy_loss", "value_loss", "entropy", "pc_loss",
                                         "vr_loss", "rp_loss", "grad_norm"])
    np.testing.assert_array_equal(flats[0].view(np.uint32), flats[1].view(np.uint32))


# ppo_clip, learning rate and trainer seed per case, as tests/test_reuse_gpu.py picks them: the fp64 rebuild of a reuse update
# must have no row within EDGE of a clip edge (asserted below)
REUSE_CASES = [(True, 1, (0.01, 0.1, 21)), (False, 2, (0.05, 0.02, 21))]


@pytest.mark.parametrize("lstm,groups,picked", REUSE_CASES)
def test_reuse_updates_with_normalised_advantages_against_fp64(fp7, lstm, groups, picked):
    """reuse_epochs = 2 with the option on: both updates of every group rebuilt in fp64 by tests/test_reuse_gpu.py's _rebuild
    with adv_norm in the place of adv, at that file's bars."""
    ppo_clip, lr0, seed = picked
    Bn, T, E = (3 if groups == 1 else 4), 5, 2
    net, applier, tr = _build(Bn, T, 12, lstm, groups=groups, lr0=lr0, seed=seed, reuse_epochs=E, ppo_clip=ppo_clip,
                              normalize_advantages=True)
    ended = 0
    for g in range(groups):
        tr._select_group(g)
        for e in range(E):
            tr.reuse_stats_i.zero_()
            if e == 0:
                tr.compute_gradients()
            else:
                tr.reuse_gradients()
            raw = tr.adv
            want_n = AM.adv_normalize(raw.cpu().numpy(), tr.active_log.cpu().numpy(), F32(1e-8))[0]
            assert (np.abs(tr.adv_norm.cpu().numpy() - want_n) <= _adv_bar(want_n)).all()
            tr.adv = tr.adv_norm                                  # what the policy loss read: _rebuild reads tr.adv
            try:
                want_l, want_g, info = RG._rebuild(net, tr, T, lstm, e > 0, 0.0)
            finally:
                tr.adv = raw
            got_l = tr.losses.cpu().numpy()[:3].astype(np.float64)
            loss_ratio = float((np.abs(got_l - want_l) / (RG.LOSS_RTOL * np.abs(want_l))).max())
            ratios = {}
            for name, gw in want_g.items():
                gd = net.grads.shaped(name).cpu().numpy().astype(np.float64)
                ratios[name] = float(np.abs(gd - gw).max() / (RG.GRAD_REL * np.abs(gw).max()))
            worst = max(ratios, key=ratios.get)
            print("lstm=%s groups=%d g=%d e=%d: loss %.3f of its bar, gradient %.3f (%s); counted %d" % (
                lstm, groups, g, e, loss_ratio, ratios[worst], worst, info["counted"]))
            margins.record("normalised reuse lstm=%s G=%d g=%d e=%d" % (lstm, groups, g, e), max(loss_ratio, ratios[worst]),
                           "losses rel 1e-4, gradients 2e-5 of the variable's largest")
            assert loss_ratio <= 1.0, (got_l, want_l)
            assert ratios[worst] <= 1.0, (worst, ratios[worst])
            if e > 0:
                edge = RG.PM.edge_distance(info["rho"], ppo_clip)
                assert edge > RG.EDGE, edge                       # asserted, not skipped
                assert tr.reuse_stats_i.cpu().numpy().tolist() == [info["clipped"], info["counted"]]
            ended += int((~info["on"]).sum())
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, tr._anneal_learning_rate(0))
            net.mark_params_changed()
    assert ended > 0


# ---- 5. full UNREAL ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_type", ["maze", "arcade"])
def test_full_unreal_with_every_option(env_type):
    """Adam, normalised advantages, reuse_epochs = 2, groups = 2, the exploration bonus and GAE(0.95), LSTM + pixel control +
    value replay + reward prediction, on a first-person maze and on Breakout: finite losses and parameters, and a call's
    env steps are those of its two rollouts."""
    from unreal_amd.environment.environment import Environment
    name = "optim_full_" + env_type
    if env_type == "arcade":
        Environment.register_arcade_config(name, **dict(TC.BREAKOUT, max_episode_steps=9))
    else:
        rs = np.random.RandomState(7)
        Environment.register_maze_config(name, [MM.random_layout(7, rs, marks="")], view="first_person", random_start=True,
                                         random_goal=True, max_episode_steps=3)
    try:
        net, applier, tr = _build(4, 5, 50, True, aux=True, groups=2, env=(env_type, name), adam=ADAM, reuse_epochs=2,
                                  normalize_advantages=True, explore_beta=0.0625, gae_lambda=0.95)
        rolled = []
        inner = tr.compute_gradients

        def counting():
            inner()
            rolled.append(int(tr.active_log.sum()))
        tr.compute_gradients = counting
        for call in range(3):
            del rolled[:]
            steps, _ = tr.process(None, call * 20)
            assert len(rolled) == 2 and steps == sum(rolled) and 0 < steps <= 4 * 5, (steps, rolled)
            l = tr.last_losses
            assert all(np.isfinite(v) for v in l.values()), l
            assert all(k in l for k in ("adv_mean", "adv_std", "clip_fraction", "approx_kl", "explore_bonus", "vr_loss"))
            assert l["adv_std"] > 0 and 0.0 <= l["clip_fraction"] <= 1.0
            assert applier.t == (call + 1) * 4
        assert bool(torch.isfinite(net.params.flat).all()) and bool(torch.isfinite(applier.m).all())
        assert bool(torch.isfinite(applier.v).all()) and float(applier.v.min()) >= 0.0
    finally:
        (Environment.ARCADE_CONFIG if env_type == "arcade" else Environment.MAZE_CONFIG).pop(name, None)
