"""tests/absmax_audit.py without a GPU: its table against include/unreal_hip.h (a new slot-taking entry cannot be added
without the audit knowing) and the wrapper's bookkeeping against a fake lib().call on host memory."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

from tests import absmax_audit as AA
from unreal_amd import _lib


# ---- 1. the table against the header ---------------------------------------------------------------------------------------
def test_every_entry_with_an_absmax_parameter_is_in_the_table():
    params = AA.header_params()
    protos = _lib.parse_header()
    assert set(params) == set(protos)
    takers = {e: [n for n in names if "absmax" in n] for e, names in params.items()}
    takers = {e: n for e, n in takers.items() if n and e != "unreal_absmax_f32"}
    assert len(takers) >= 14, sorted(takers)                      # the header as it stands (unreal_absmax_f32's is `slot`)
    assert sorted(takers) == sorted(AA.TABLE), "include/unreal_hip.h and absmax_audit.TABLE name different entries"
    for entry, names in takers.items():
        slots = [p.slot for p in AA.TABLE[entry]]
        assert sorted(slots) == sorted(names), (entry, slots, names)
        assert len(params[entry]) + 1 == len(protos[entry])       # + stream: the positions are ops._call's
    pos = AA.positions()
    for entry, by_name in pos.items():
        assert by_name and all(0 <= i < len(protos[entry]) - 1 for i in by_name.values()), entry
        for name, i in by_name.items():
            assert params[entry][i] == name
        for p in AA.TABLE[entry]:
            assert protos[entry][pos[entry][p.slot]] is ctypes.c_void_p
            if p.kind != AA.SHADOW:
                assert protos[entry][pos[entry][p.operand]] is ctypes.c_void_p
                for d in (p.rows, p.cols, p.ld):
                    assert not isinstance(d, str) or protos[entry][pos[entry][d]] is ctypes.c_int, (entry, d)


def test_a_weight_shadows_slot_is_listed_but_not_audited_and_kinds_follow_constness():
    """A slot the kernel commits to is `float*`, one it reads `const float*`: the table's kinds agree with the header."""
    src = re.sub(r"/\*.*?\*/", " ", open(AA.HEADER).read(), flags=re.S)
    for entry, pairs in AA.TABLE.items():
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % entry, src).group(1).split(",")
        decl = {re.findall(r"\w+", a)[-1]: a for a in args}
        for p in pairs:
            const = "const" in decl[p.slot]
            assert const == (p.kind != AA.COMMITTED), (entry, p.slot, decl[p.slot])
            assert (p.kind == AA.SHADOW) == (p.slot == "w_absmax" and entry != "unreal_split_f16x2"), (entry, p.slot)
    floors = {(e, p.operand): p.floor for e, ps in AA.TABLE.items() for p in ps if p.floor}
    assert floors == {("unreal_lstm_step_fwd", "x"): 1.0}             # a_floor = 1 (gemm_split.hip)


def test_positions_refuses_a_name_the_header_lacks():
    with pytest.raises(KeyError, match="no parameter"):
        AA.positions({"unreal_gemm_f32_split_tn": [AA.Pair(AA.READ, "c_absmax", "A", "K", "M", "lda")]})


# ---- 2. the wrapper against a fake lib().call ------------------------------------------------------------------------------
def _floats(addr, n):
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(addr))


class FakeLib(object):
    """unreal_absmax_f32 on host memory (slot = max(slot, max |x[r][c]|)); every call is recorded."""

    def __init__(self):
        self.calls = []

    def call(self, name, *a):
        self.calls.append((name,) + a)
        assert name == "unreal_absmax_f32"
        rows, cols, x, ld, slot, stream = a
        assert stream == 77
        v = _floats(x, (rows - 1) * ld + cols)
        m = max(float(np.abs(v[r * ld:r * ld + cols]).max()) for r in range(rows))
        s = _floats(slot, 1)
        s[0] = max(s[0], m)


def _harness(n_pairs=8):
    """A stand-in ops module whose _call records launches and runs `effect` (the kernel's stores), the audit around it."""
    launches = []

    def _call(name, *a):
        launches.append((name,) + a)
        if ops.effect is not None:
            ops.effect()

    ops = types.SimpleNamespace(_call=_call, effect=None, stream=lambda: 77)
    fake = FakeLib()
    cells = torch.zeros(2 * n_pairs, dtype=torch.float32)
    audit = AA.AbsmaxAudit("cpu", n_pairs=n_pairs, ops_module=ops, lib_call=fake.call, cells=cells)
    return ops, _call, launches, fake, cells, audit


def _nt_args(A, M, K, lda, a_slot, C, N, ldc, c_slot):
    p = lambda t: 0 if t is None else t.data_ptr()
    return (M, N, K, p(A), lda, p(a_slot), 1234, 64, 4096, 5678, p(C), ldc, p(c_slot), 0, 0, 0, 0, 1)


def test_read_and_committed_pairs_cells_and_restore():
    ops, orig, launches, fake, cells, audit = _harness()
    A = torch.arange(12, dtype=torch.float32).reshape(3, 4) - 20.0        # [3, 4], ld 4: the launch reads columns 0..2
    A[:, 3] = 99.0                                                        # (outside the view: not the launch's to cover)
    a_slot = torch.tensor([12.0])                                         # one binade under max |A[:, :3]| = 20
    C = torch.zeros(6)
    c_slot = torch.zeros(1)

    def kernel():                                                         # the launch stores C and commits max |C|
        C.copy_(torch.tensor([1.0, -7.0, 2.0, 0.5, 3.0, -1.0]))
        c_slot[0] = 7.0
    ops.effect = kernel
    with audit:
        assert ops._call is not orig
        ops._call("unreal_gemm_f32_split_nt", *_nt_args(A, 3, 3, 4, a_slot, C, 2, 2, c_slot))
        ops._call("unreal_copy_words", 4, 1, 2)                           # not in the table: forwarded untouched
    assert ops._call is orig                                              # restored on exit
    assert [l[0] for l in launches] == ["unreal_gemm_f32_split_nt", "unreal_copy_words"] and audit.launches == 1
    # two audit launches per pair, the read pair's BEFORE the forwarded launch could store anything
    assert [c[0] for c in fake.calls] == ["unreal_absmax_f32"] * 4
    base = cells.data_ptr()
    assert [c[5] for c in fake.calls] == [base, base + 4, base + 8, base + 12]
    assert fake.calls[0][1:5] == (3, 3, A.data_ptr(), 4) and fake.calls[1][1:5] == (1, 1, a_slot.data_ptr(), 1)
    assert fake.calls[2][1:5] == (3, 2, C.data_ptr(), 2) and fake.calls[3][1:5] == (1, 1, c_slot.data_ptr(), 1)
    read, committed = audit.pairs
    assert (read["kind"], read["operand"], read["true"], read["claimed"]) == ("read", "A", 20.0, 12.0)
    assert (committed["kind"], committed["operand"], committed["true"], committed["claimed"]) == ("committed", "C", 7.0, 7.0)
    assert audit.violations() == [read]
    with pytest.raises(AssertionError, match=r"unreal_gemm_f32_split_nt A \(slot a_absmax, read\).*slot 12 < 20 = max \|A\| "
                                             r"\(1 binade\(s\) short\)"):
        audit.assert_clean()
    assert audit.overcover() == {("unreal_gemm_f32_split_nt", "A"): dict(binades=-1, true=20.0, claimed=12.0,
                                                                           site=read["site"], pairs=1)}


def test_a_committed_slot_below_what_the_launch_stored_is_a_violation():
    ops, orig, launches, fake, cells, audit = _harness()
    C, c_slot = torch.zeros(4), torch.zeros(1)

    def kernel():
        C.copy_(torch.tensor([0.0, 9.0, -3.0, 1.0]))
        c_slot[0] = 3.0                                                   # misses the 9
    ops.effect = kernel
    A, a_slot = torch.ones(4), torch.ones(1)
    with audit:
        ops._call("unreal_gemm_f32_split_nt", *_nt_args(A, 2, 2, 2, a_slot, C, 2, 2, c_slot))
    assert [(p["kind"], p["true"], p["claimed"]) for p in audit.violations()] == [("committed", 9.0, 3.0)]


def test_null_pointers_skip_the_pair_and_the_floor_is_claimed():
    ops, orig, launches, fake, cells, audit = _harness()
    x = torch.tensor([0.25, -0.75, 0.5, 0.0])
    x_slot = torch.tensor([0.125])                                        # under the operand, within the kernel's floor of 1
    big = torch.tensor([0.25, -1.5, 0.5, 0.0])
    p = lambda t: t.data_ptr()
    step = lambda xp, sp: ("unreal_lstm_step_fwd", 2, xp, 2, 2, sp, 11, 256, 12, 288, 0, 13, 14, 15, 16, 17, 18, 256)
    A, one, C = torch.ones(4), torch.ones(1), torch.zeros(4)
    with audit:
        ops._call(*step(0, 0))                                            # x == NULL: the hoisted form, no pair
        ops._call(*step(p(x), p(x_slot)))
        ops._call(*step(p(big), p(x_slot)))
        ops._call("unreal_gemm_f32_split_nt", *_nt_args(A, 2, 2, 2, one, C, 2, 2, None))    # no c_absmax
    assert len(launches) == 4 and audit.launches == 4
    assert [(q["entry"], q["true"], q["claimed"]) for q in audit.pairs] == [
        ("unreal_lstm_step_fwd", 0.75, 1.0), ("unreal_lstm_step_fwd", 1.5, 1.0), ("unreal_gemm_f32_split_nt", 1.0, 1.0)]
    assert [q["true"] for q in audit.violations()] == [1.5]
    assert audit.overcover()[("unreal_lstm_step_fwd", "x")]["binades"] == 1          # floor(log2 1) - floor(log2 0.75)


def test_zero_operands_are_left_out_of_the_over_cover_and_exhaustion_raises():
    ops, orig, launches, fake, cells, audit = _harness(n_pairs=2)
    Z, slot, C = torch.zeros(4), torch.ones(1), torch.zeros(4)
    with pytest.raises(RuntimeError, match="holds 2 pairs"):
        with audit:
            for _ in range(3):
                ops._call("unreal_gemm_f32_split_nt", *_nt_args(Z, 2, 2, 2, slot, C, 2, 2, None))
    assert ops._call is orig                                              # restored although the body raised
    assert len(audit.pairs) == 2 and audit.violations() == [] and audit.overcover() == {}
    assert len(launches) == 2                                             # the third launch was not forwarded


def test_the_site_is_the_frame_inside_the_package_and_the_report_merges(tmp_path, monkeypatch):
    ops, orig, launches, fake, cells, audit = _harness()
    A, slot, C = torch.full((4,), 3.0), torch.tensor([64.0]), torch.zeros(4)
    monkeypatch.setattr(AA, "PKG_DIR", __file__)                          # "the package" is this file: the frame below
    monkeypatch.setattr(AA, "OPS_FILE", "")

    def call_site():
        ops._call("unreal_gemm_f32_split_nt", *_nt_args(A, 2, 2, 2, slot, C, 2, 2, None))
    with audit:
        call_site()
    site = audit.pairs[0]["site"]
    assert site[0].endswith("test_absmax_audit_cpu.py") and site[2] == "call_site"
    table = audit.overcover()
    assert table[("unreal_gemm_f32_split_nt", "A")]["binades"] == 5       # floor(log2 64) - floor(log2 3)
    worse = {("unreal_gemm_f32_split_nt", "A"): dict(binades=7, true=0.5, claimed=64.0, site=site, pairs=2)}
    merged = AA.merge_overcover(table, worse)
    assert merged[("unreal_gemm_f32_split_nt", "A")]["binades"] == 7 and merged[("unreal_gemm_f32_split_nt", "A")]["pairs"] == 3
    path = str(tmp_path / "out" / "absmax_audit.json")
    AA.write_report("one", table, path=path, extra=dict(seconds=1.5))
    doc = AA.write_report("two", merged, path=path)
    assert sorted(doc) == ["one", "two"] and doc["one"]["seconds"] == 1.5
    assert doc["two"]["rows"][0]["binades"] == 7 and doc["one"]["rows"][0]["site"].endswith("call_site")


def test_a_watched_shadows_slot_is_audited_against_the_live_weights():
    """AbsmaxAudit.watch: the w_absmax of a GEMM is looked up among the network's shadows (made on first use: the dict is read
    when a launch names an unknown slot) and compared with the fp32 weights the shadow was split from."""
    ops, orig, launches, fake, cells, audit = _harness()
    W = torch.tensor([0.0, 0.5, -2.0, 1.0, 7.0, 7.0, 7.0, 7.0])          # the shadow is of W[2:6] as [2, 1], ld 2: -2, 7
    wmax = torch.tensor([2.0])                                            # split when the weights were smaller
    kernel = torch.arange(2 * 1024 + 256 * 1024, dtype=torch.float32) / 1e6
    kmax = torch.tensor([1.0])
    net = types.SimpleNamespace(_shadow=None)
    A, one, C = torch.ones(4), torch.ones(1), torch.zeros(4)
    args = list(_nt_args(A, 2, 2, 2, one, C, 2, 2, None))
    with audit.watch(net):
        args[9] = wmax.data_ptr()
        ops._call("unreal_gemm_f32_split_nt", *args)                      # no shadow known yet: the slot is skipped
        net._shadow = dict(fc=types.SimpleNamespace(src=W, offset=2, rows=2, cols=1, ld_src=2, wmax=wmax),
                           lstm=types.SimpleNamespace(src=kernel, K_x=2, wmax=kmax))
        ops._call("unreal_gemm_f32_split_nt", *args)
        args[9] = kmax.data_ptr()
        ops._call("unreal_gemm_f32_split_nt", *args)
    got = [(q["operand"], q["slot"], q["true"], q["claimed"]) for q in audit.pairs]
    top = float(kernel[-1])
    assert got == [("A", "a_absmax", 1.0, 1.0), ("A", "a_absmax", 1.0, 1.0), ("W", "w_absmax", 7.0, 2.0),
                   ("A", "a_absmax", 1.0, 1.0), ("W", "w_absmax", top, 1.0)]
    assert [q["true"] for q in audit.violations()] == [7.0]
    view = [c for c in fake.calls if c[3] == W.data_ptr() + 8][0]
    assert view[1:5] == (2, 1, W.data_ptr() + 8, 2)
