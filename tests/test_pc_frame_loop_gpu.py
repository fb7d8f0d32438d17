"""The frame loops of unreal_pc_deconv_train / _fwd / _bwd on per-lane address tables (GPU): every per-frame output bit for
bit what the kernels before that change computed (tests/golden/pc_train_parent_bits.json, written by
tools/record_pc_train_bits.py on that commit), at the launch sizes and channel counts where the loop can go wrong; the sums
that float atomics reduce across workgroups against a float64 restatement at the bars of
test_kernels_gpu.test_pc_deconv_fwd_bwd (grads atol = rtol = 1e-5, loss atol = rtol = 1e-4), and bit for bit where one
workgroup does all the adding (N = 1); and nothing written outside the outputs (dump rows stay on chip).
Shapes and inputs: tests/pc_cases.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

try:
    import pc_cases as C
except ImportError:            # imported as tests.<module>: tests/ itself is not on sys.path
    from tests import pc_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pc_train_parent_bits.json")
GRAD_TOL = dict(atol=1e-5, rtol=1e-5)            # test_pc_deconv_fwd_bwd's `tol`
LOSS_TOL = dict(atol=1e-4, rtol=1e-4)            # test_pc_deconv_fwd_bwd's loss bars


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _fp64(case, inp):
    """loss * GS, d_hp (relu mask applied) and the four parameter gradients in float64."""
    N, A, _ = case
    t = lambda a, shape: torch.tensor(a.astype(np.float64).reshape(shape), requires_grad=True)
    hp, Wv, bv = t(inp["hp"], (N, 9, 9, 32)), t(inp["Wv"], (4, 4, 1, 32)), t(inp["bv"], (1,))
    Wa, ba = t(inp["Wa"], (4, 4, A, 32)), t(inp["ba"], (A,))
    x = hp.permute(0, 3, 1, 2)
    v = F.relu(F.conv_transpose2d(x, Wv.permute(3, 2, 0, 1), bv, stride=2))
    a = F.relu(F.conv_transpose2d(x, Wa.permute(3, 2, 0, 1), ba, stride=2))
    q = (v + a - a.mean(1, keepdim=True)).permute(0, 2, 3, 1)
    qa = (q * torch.tensor(np.eye(A)[inp["act"]]).reshape(N, 1, 1, A)).sum(3)
    m = torch.tensor(inp["mask"].astype(np.float64)).reshape(N, 1, 1)
    tgt = torch.tensor(inp["tgt"].astype(np.float64).reshape(N, 20, 20))
    loss = C.LAM * 0.5 * (((tgt - qa) ** 2) * m).sum()
    (loss * C.GS).backward()
    return dict(loss=float(loss.detach()) * C.GS, dhp=(hp.grad * (hp.detach() > 0)).numpy().reshape(-1), dWv=Wv.grad.numpy().reshape(-1),
                dbv=bv.grad.numpy().reshape(-1), dWa=Wa.grad.numpy().reshape(-1), dba=ba.grad.numpy().reshape(-1))


def _ratio(got, ref, atol, rtol):
    """max of |got - ref| / (atol + rtol |ref|): <= 1 passes."""
    g = got.detach().cpu().double().numpy().reshape(-1)
    r = np.asarray(ref, dtype=np.float64).reshape(-1)
    return float((np.abs(g - r) / (atol + rtol * np.abs(r))).max())


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_bits_match_parent_sums_match_fp64_and_nothing_else_is_written(ops, case):
    N, A, _ = case
    inp = C.inputs(case)
    d = {k: torch.as_tensor(v).to(DEV) for k, v in inp.items() if k != "zq"}
    before = {k: v.clone() for k, v in d.items()}
    out = C.run(ops, torch, case, d)
    got, want = C.digests(out, N), _golden()["cases"][C.case_id(case)]
    ref = _fp64(case, inp)
    err = {}
    for pre in ("t_", "b_"):
        for k in ("dWv", "dbv", "dWa", "dba"):
            err[pre + k] = _ratio(out[pre + k], ref[k], **GRAD_TOL)
    err["t_dhp"] = _ratio(out["t_dhp_v"], ref["dhp"], **GRAD_TOL)
    err["b_dhp"] = _ratio(out["b_dhp_v"], ref["dhp"], **GRAD_TOL)
    err["t_loss"] = _ratio(out["t_loss"], [ref["loss"]], **LOSS_TOL)
    err["f_loss"] = _ratio(out["f_loss"], [ref["loss"]], **LOSS_TOL)
    print("%s: error / bar against float64: %s" % (C.case_id(case), " ".join("%s %.3f" % kv for kv in sorted(err.items()))))
    assert got == want, "bits differ from the parent's in %s; error / bar against float64: %r" % (
        [k for k in got if got[k] != want[k]], err)
    assert max(err.values()) <= 1.0, err
    # the training pass computes the same d_hp with and without its inspection output, and the forward's d_dec
    assert torch.equal(out["u_dhp_v"], out["t_dhp_v"]) and torch.equal(out["t_ddec_v"], out["f_ddec_v"])
    assert float(out["t_max"]) == float(out["t_dhp_v"].abs().max())
    if inp["zq"] >= 0:         # targets equal to Q: that frame's d_dec is zero, and its zero scale poisons nothing
        assert not out["t_ddec_v"].reshape(N, -1)[inp["zq"]].any()
        assert all(bool(torch.isfinite(out[k]).all()) for k in ("t_dhp_v", "t_dWv", "t_dWa", "t_dbv", "t_dba", "t_loss"))
    # guard frames in front of and behind every per-frame output; the inputs
    for k in C.GUARDED:
        n = out[k + "_v"].numel()
        g = n // N * C.PAD
        assert bool((out[k][:g] == C.SENTINEL).all()) and bool((out[k][g + n:] == C.SENTINEL).all()), k
    for k in d:
        assert torch.equal(d[k], before[k]), k
