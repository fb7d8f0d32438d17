"""unreal_encoder_fwd with the frame staged through registers into an fp16 image (GPU): every output bit for bit what the
kernel before that change computed (tests/golden/encoder_fwd_parent_bits.json, written by tools/record_encoder_fwd_bits.py
on that commit), at the launch sizes where the staging can go wrong; no write outside the outputs; and a prepared block made
for another frame scale is not used.  Shapes and inputs: tests/encoder_fwd_cases.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

try:
    import encoder_fwd_cases as C
except ImportError:            # imported as tests.<module>: tests/ itself is not on sys.path
    from tests import encoder_fwd_cases as C

from oracle import model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_fwd_parent_bits.json")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from unreal_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _params():
    return {k: torch.as_tensor(v.reshape(-1)).to(DEV) for k, v in C.params().items()}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _oracle_err(case, out):
    """max of |got - ref| / (1e-5 + 1e-5 |ref|) for c1 and f2 against float64 (the bars of test_kernels_gpu.test_encoder_fwd)."""
    N = case[0]
    pool, idx, scale = C.inputs(case)
    p = {k: torch.tensor(v.astype(np.float64)) for k, v in C.params().items()}
    po = dict(W_base_conv1=p["W1"], b_base_conv1=p["b1"], W_base_conv2=p["W2"], b_base_conv2=p["b2"])
    h1, h2 = M.encoder(torch.tensor(pool[idx].astype(np.float64)) * scale, po)
    res = {}
    for name, got, ref in (("c1", out["c1"][:N * 6400], h1), ("f2", out["f2"][:N * 2592], h2)):
        g, r = got.cpu().double().numpy().reshape(-1), ref.numpy().reshape(-1)
        res[name] = float((np.abs(g - r) / (1e-5 + 1e-5 * np.abs(r))).max())
    return res


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_bits_match_parent_and_nothing_else_is_written(ops, case):
    N = case[0]
    pool, idx, scale = C.inputs(case)
    pool_d = torch.as_tensor(pool.reshape(-1)).to(DEV)
    before = pool_d.clone()
    out = C.run(ops, torch, pool_d, torch.as_tensor(idx).to(DEV), scale, _params())
    got, want = C.digests(out, N), _golden()["cases"][C.case_id(case)]
    err = _oracle_err(case, out)
    print("%s: error / bar against float64: c1 %.3f, f2 %.3f" % (C.case_id(case), err["c1"], err["f2"]))
    assert got == want, "bits differ from the parent's in %s; error / bar against float64: %r" % (
        [k for k in got if got[k] != want[k]], err)
    assert err["c1"] <= 1.0 and err["f2"] <= 1.0, err
    # one frame's worth of sentinel behind every output, and the frame pool
    assert bool((out["f2"][N * 2592:] == -7.0).all()) and bool((out["c1"][N * 6400:] == -7.0).all())
    assert bool((out["bits"][N * 162:] == 0x5a5a).all())
    assert torch.equal(pool_d, before)
    assert float(out["s2"]) == float(out["f2"][:N * 2592].max()) and float(out["s1"]) == float(out["c1"][:N * 6400].max())


@pytest.mark.parametrize("N", [3, 513])
def test_output_combinations(ops, N):
    """c1 saved or not, bit words on or off, prepared block or not: f2 bit-equal across all eight, c1 / bit words equal wherever
    they are produced, sentinels intact; and a frame's bits do not depend on N or on its place in the list."""
    case = (N, "u8", "pool")
    pool, idx, scale = C.inputs(case)
    P = _params()
    pool_d, idx_d = torch.as_tensor(pool.reshape(-1)).to(DEV), torch.as_tensor(idx).to(DEV)
    prep = ops.encoder_prepare(P["W1"], P["b1"], P["W2"], scale)
    ref = C.run(ops, torch, pool_d, idx_d, scale, P)
    for save_c1 in (True, False):
        for bits in (True, False):
            for blk in (None, prep):
                o = C.run(ops, torch, pool_d, idx_d, scale, P, save_c1=save_c1, bits=bits, prepared=blk)
                what = (save_c1, bits, blk is not None)
                assert torch.equal(o["f2"], ref["f2"]) and torch.equal(o["s2"], ref["s2"]), what
                assert not save_c1 or (torch.equal(o["c1"], ref["c1"]) and torch.equal(o["s1"], ref["s1"])), what
                assert not bits or torch.equal(o["bits"], ref["bits"]), what
    for k in sorted({0, N // 2, N - 1}):
        one = C.run(ops, torch, pool_d, idx_d[k:k + 1].clone(), scale, P)
        assert torch.equal(one["f2"][:2592], ref["f2"][k * 2592:(k + 1) * 2592]), k
        assert torch.equal(one["c1"][:6400], ref["c1"][k * 6400:(k + 1) * 6400]), k
        assert torch.equal(one["bits"][:162], ref["bits"][k * 162:(k + 1) * 162]), k


def test_block_prepared_for_another_scale_is_not_used(ops):
    """The block stores the frame scale it was made for (its c1 plane scale depends on it): a launch at another scale
    derives scales and fragments itself -- bit-equal to the launch without a block."""
    case = (3, "u8", "pool")
    pool, idx, scale = C.inputs(case)
    P = _params()
    pool_d, idx_d = torch.as_tensor(pool.reshape(-1)).to(DEV), torch.as_tensor(idx).to(DEV)
    other = ops.encoder_prepare(P["W1"], P["b1"], P["W2"], 1.0)
    a = C.run(ops, torch, pool_d, idx_d, scale, P)
    b = C.run(ops, torch, pool_d, idx_d, scale, P, prepared=other)
    for k in ("f2", "c1", "bits", "s2", "s1"):
        assert torch.equal(a[k], b[k]), k


def test_batch1_runner_with_and_without_prepared_block():
    """run_base_policy_and_value reads its staged frame at 1/255 whatever the environment's scale: with prepare_encoder on it
    must launch with a block made for 1/255, not the maze-scale one -- the same pi and V as with prepare_encoder off."""
    from unreal_amd.model.model import UnrealModel
    net = UnrealModel(4, 0, -1, True, True, True, True, 0.05, 0.001, DEV, seed=7)
    net.bind_frame_scale(1.0)                   # a maze-scale network
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, size=(84, 84, 3)) / 255.0
    lar = np.array([0, 1, 0, 0, 0.5])
    res = []
    for on in (True, False):
        net.prepare_encoder = on
        net.reset_state()
        res.append(net.run_base_policy_and_value(None, {'image': img}, lar))
        assert net.frame_scale == 1.0
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1], (res[0][:2], res[1][:2])
    assert np.isfinite(res[0][0]).all() and abs(res[0][0].sum() - 1.0) < 1e-5
