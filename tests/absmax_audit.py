"""Launch interceptor that audits the absmax slot of every fp16-split operand (test infrastructure, no product code).

include/unreal_hip.h, at unreal_absmax_f32: "the slot handed to a GEMM must cover every element the GEMM reads (a larger
value only costs precision)".  The kernel tests reduce the slot from the operand itself; which slot the HOST hands over
(model/model.py, train/trainer.py) is what this module checks.  Inside `with AbsmaxAudit(...)` every launch of the library
(ops._call) is looked up in TABLE:

  read pair       before the launch, on the launch's stream: the true max |operand| of the view the launch reads is reduced
                  into a fresh cell (the library's own unreal_absmax_f32) and the slot's value is copied into a second one
  committed pair  the same two launches after the launch: max |what the launch stored| against the slot it committed to
  shadow slot     the w_absmax of a pre-split weight shadow.  The planes are fp16, so the operand cannot be reduced; for the
                  shadows of a network handed to `watch()` the slot is audited as a read pair against the LIVE fp32 weights
                  the shadow was split from (operand "W"): a shadow whose weights have grown since the split under-covers

No host synchronisation per launch; the cells are one pre-zeroed buffer that is read back with one copy when the context
closes.  Both checks are the header's contract, plain inequalities:

  read       max(slot, floor) >= true max of what the launch reads
  committed  slot after the launch >= max |what the launch stored|

and every read pair's over-cover floor(log2 claimed) - floor(log2 true) is recorded (pairs with a true maximum of 0 are
skipped): `overcover()` keeps the worst per (entry, operand), `write_report` merges it into the JSON report (REPORT below).
"""
import json
import math
import os
import re
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unreal_hip.h")
PKG_DIR = os.path.join(ROOT, "unreal_amd") + os.sep
OPS_FILE = os.path.join(ROOT, "unreal_amd", "ops.py")
# the JSON report: absmax_audit.json in $ABSMAX_AUDIT_DIR (a run that collects its output elsewhere), by default in runs/
REPORT = os.path.join(os.environ.get("ABSMAX_AUDIT_DIR") or os.path.join(ROOT, "runs"), "absmax_audit.json")

READ, COMMITTED, SHADOW = "read", "committed", "shadow"
F2_DIM, C1_DIM, PC_CELLS = 2592, 6400, 400


class Pair(object):
    """One (operand, rows, cols, ld, slot) tuple of an entry, by the header's parameter names.  rows / cols / ld: a
    parameter name, an int, or a function of the {name: value} dict of the launch."""

    def __init__(self, kind, slot, operand=None, rows=None, cols=None, ld=None, floor=0.0):
        self.kind, self.slot, self.operand, self.rows, self.cols, self.ld, self.floor = kind, slot, operand, rows, cols, ld, floor

    def params(self):
        """Header parameter names this pair reads by position."""
        names = [self.slot] + ([self.operand] if self.operand else [])
        return names + [v for v in (self.rows, self.cols, self.ld) if isinstance(v, str)]


def _read(operand, rows, cols, ld, slot, floor=0.0):
    return Pair(READ, slot, operand, rows, cols, ld if ld is not None else cols, floor)


def _committed(operand, rows, cols, ld, slot):
    return Pair(COMMITTED, slot, operand, rows, cols, ld if ld is not None else cols)


def _shadow(slot):
    return Pair(SHADOW, slot)


def _hw_f2(a):
    """F = 32 h2 w2 of an H x W frame (ops.frame_dims)."""
    h1, w1 = (a["H"] - 8) // 4 + 1, (a["W"] - 8) // 4 + 1
    return 32 * ((h1 - 4) // 2 + 1) * ((w1 - 4) // 2 + 1)


def _ddec(a):
    return PC_CELLS * (1 + a["A"])


# Geometry as the ops wrappers' own _chk lines state it; frame-batched tensors are rows = N, cols = ld = per-frame size.
TABLE = {
    "unreal_gemm_f32_split_nt": [_read("A", "M", "K", "lda", "a_absmax"), _shadow("w_absmax"),
                                 _committed("C", "M", "N", "ldc", "c_absmax")],
    "unreal_gemm_f32_split_nt_slabs": [_read("A", "M", "K", "lda", "a_absmax"), _shadow("w_absmax"),
                                       _committed("C", "M", "N", "ldc", "c_absmax")],
    "unreal_gemm_f32_split_tn": [_read("A", "K", "M", "lda", "a_absmax"), _read("B", "K", "N", "ldb", "b_absmax")],
    "unreal_split_f16x2": [_read("src", "rows", "cols", "ld_src", "w_absmax")],
    # a_floor = 1 (gemm_split.hip): the kernel scales [x | h_prev] by max(slot, 1), |h_prev| < 1
    "unreal_lstm_step_fwd": [_read("x", "rows", "Kx", "ldx", "x_absmax", floor=1.0), _shadow("w_absmax")],
    "unreal_lstm_bptt_step": [_read("d_gates", "rows", 1024, None, "a_absmax"), _shadow("w_absmax"),
                              _committed("dpre", "rows", 1024, None, "dpre_absmax0"),
                              _committed("dpre", "rows", 1024, None, "dpre_absmax1")],
    "unreal_lstm_gates_bwd": [_committed("dpre", "rows", 1024, None, "dpre_absmax0"),
                              _committed("dpre", "rows", 1024, None, "dpre_absmax1")],
    "unreal_encoder_fwd": [_committed("f2_out", "N", F2_DIM, None, "f2_absmax"),
                           _committed("c1_out", "N", C1_DIM, None, "c1_absmax")],
    "unreal_encoder_hw_fwd": [_committed("f2_out", "N", _hw_f2, _hw_f2, "f2_absmax")],
    "unreal_maze_policy_rollout_step_encode": [_committed("f2_out", "B", F2_DIM, None, "f2_absmax"),
                                               _committed("c1_out", "B", C1_DIM, None, "c1_absmax")],
    "unreal_encoder_bwd": [_read("c1_saved", "N", C1_DIM, None, "c1_absmax"), _read("d2", "N", F2_DIM, None, "d2_absmax")],
    "unreal_pc_deconv_fwd": [_read("hp", "N", F2_DIM, None, "hp_absmax"), _committed("d_dec", "N", _ddec, _ddec, "ddec_absmax")],
    "unreal_pc_deconv_bwd": [_read("hp", "N", F2_DIM, None, "hp_absmax"), _read("d_dec", "N", _ddec, _ddec, "ddec_absmax"),
                             _committed("d_hp", "N", F2_DIM, None, "dhp_absmax")],
    "unreal_pc_deconv_train": [_read("hp", "N", F2_DIM, None, "hp_absmax"), _committed("d_hp", "N", F2_DIM, None, "dhp_absmax")],
}


_WATCHED = Pair(READ, "w_absmax", "W")       # a watched shadow's slot against the live weights (AbsmaxAudit.watch)


def header_params(path=HEADER):
    """-> {entry: [parameter names]} of every `int unreal_*(...)` prototype, the trailing `stream` dropped (the position of
    a name is its position among the arguments of ops._call)."""
    src = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(unreal_\w+)\s*\(([^)]*)\)\s*;", src):
        names = [re.findall(r"\w+", a)[-1] for a in m.group(2).split(",")]
        out[m.group(1)] = names[:-1] if names and names[-1] == "stream" else names
    return out


def positions(table=None, params=None):
    """-> {entry: {parameter name: argument position}} of the table's entries; KeyError for a name the header lacks."""
    table = TABLE if table is None else table
    params = header_params() if params is None else params
    out = {}
    for entry, pairs in table.items():
        names = params[entry]
        for p in pairs:
            for n in p.params():
                if n not in names:
                    raise KeyError("%s has no parameter %r" % (entry, n))
        out[entry] = dict((n, i) for i, n in enumerate(names))     # all of them: a computed size may read any (H, W, A)
    return out


def binade(x):
    """floor(log2 x) of a positive finite float."""
    return math.frexp(x)[1] - 1


def _site():
    """(file relative to the repository, line, function) of the innermost frame inside unreal_amd/ that is not an ops
    wrapper; the ops wrapper's own frame when the launch comes from outside the package."""
    f = sys._getframe(2)
    wrapper = None
    while f is not None:
        fn = f.f_code.co_filename
        if fn.startswith(PKG_DIR):
            here = (os.path.relpath(fn, ROOT), f.f_lineno, f.f_code.co_name)
            if fn != OPS_FILE:
                return here
            wrapper = here                     # ends as the outermost ops frame: the wrapper the caller used
        f = f.f_back
    return wrapper or ("<outside unreal_amd>", 0, "?")


class AbsmaxAudit(object):
    """Context manager: replaces ops._call (restored on exit) and audits every launch that TABLE knows.

    config    label of the configuration (failure messages, the report)
    n_pairs   audited pairs the cell buffer holds (two floats each); one more raises RuntimeError
    ops_module / lib_call / stream / cells: test seams -- the module whose _call is replaced, the function that launches
    the audit's own reductions (default: lib().call), the stream getter (default: ops.stream) and the zeroed float32
    cell buffer (default: torch.zeros on `device`)."""

    def __init__(self, config="", device="cuda:0", n_pairs=1 << 16, ops_module=None, lib_call=None, stream=None, cells=None,
                 table=None):
        if ops_module is None:
            from unreal_amd import ops as ops_module
        self.ops, self.config, self.device, self.n_pairs = ops_module, config, device, int(n_pairs)
        self._lib_call, self._stream, self.cells = lib_call, stream, cells
        self.table = TABLE if table is None else table
        self._pos = positions(self.table)
        self.records = []          # (entry, pair, site, cell index of the true maximum; the claimed value is the next cell)
        self.pairs = None          # after exit: [dict(entry, operand, kind, slot, site, true, claimed, floor)]
        self.launches = 0
        self._lock = threading.Lock()
        self._orig = None
        self._nets, self._shadows = [], {}

    def watch(self, *nets):
        """Audit the weight shadows of these networks too (UnrealModel: its `_shadow` dict, read again whenever a launch names
        a slot not seen before, since shadows are made on first use)."""
        self._nets.extend(nets)
        return self

    def _shadow_view(self, slot):
        """(pointer, rows, cols, ld) of the live fp32 weights behind the shadow whose wmax slot is `slot`, or None."""
        v = self._shadows.get(slot)
        if v is None:
            for net in self._nets:
                for sh in (getattr(net, "_shadow", None) or {}).values():
                    if hasattr(sh, "K_x"):               # ops.LstmKernelShadow: the whole kernel [K_x + 256, 1024]
                        view = (sh.src.data_ptr(), sh.K_x + 256, 1024, 1024)
                    else:                                # ops.SplitWeights: src[offset:] as [rows, cols], row stride ld_src
                        view = (sh.src.data_ptr() + 4 * sh.offset, sh.rows, sh.cols, sh.ld_src)
                    self._shadows[sh.wmax.data_ptr()] = view
            v = self._shadows.get(slot)
        return v

    # -- context ----------------------------------------------------------------------------------------
    def __enter__(self):
        import torch
        if self._orig is not None:
            raise RuntimeError("AbsmaxAudit is not re-entrant")
        if self.cells is None:
            self.cells = torch.zeros(2 * self.n_pairs, dtype=torch.float32, device=self.device)
            torch.cuda.synchronize(self.device)      # the fill is done before a launch on any stream maxes into a cell
        if self.cells.numel() < 2 * self.n_pairs:
            raise ValueError("cell buffer: %d floats, need %d" % (self.cells.numel(), 2 * self.n_pairs))
        if self._lib_call is None:
            from unreal_amd._lib import lib
            self._lib_call = lib().call
        if self._stream is None:
            self._stream = self.ops.stream
        self._base = self.cells.data_ptr()
        self._orig = self.ops._call
        self.ops._call = self._wrapped
        return self

    def __exit__(self, *exc):
        self.ops._call, self._orig = self._orig, None
        if self.cells.is_cuda:
            import torch
            torch.cuda.synchronize(self.cells.device)     # launches of every stream the pass used
        host = self.cells[:2 * len(self.records)].cpu().tolist()  # the one copy
        self.pairs = []
        for entry, pair, site, cell in self.records:
            claimed = host[cell + 1]
            if pair.kind == READ:
                claimed = max(claimed, pair.floor)
            self.pairs.append(dict(entry=entry, operand=pair.operand, kind=pair.kind, slot=pair.slot, site=site,
                                   true=host[cell], claimed=claimed, floor=pair.floor))
        return False

    # -- the wrapper ------------------------------------------------------------------------------------
    def _wrapped(self, name, *a):
        pairs = self.table.get(name)
        if pairs is None:
            return self._orig(name, *a)
        self.launches += 1
        pos = self._pos[name]
        site = _site()
        args = dict((n, a[i]) for n, i in pos.items())
        dim = lambda v: int(args[v]) if isinstance(v, str) else int(v(args)) if callable(v) else int(v)
        live = []
        for p in pairs:
            slot = args[p.slot]
            if p.kind == SHADOW:
                view = self._shadow_view(slot) if self._nets and slot else None
                if view is not None:
                    live.append((_WATCHED, view[0], slot) + view[1:])
                continue
            x = args[p.operand]
            if not slot or not x:                   # a nullable slot, x == NULL of unreal_lstm_step_fwd, no c1_out
                continue
            live.append((p, x, slot, dim(p.rows), dim(p.cols), dim(p.ld)))
        for m in live:
            if m[0].kind == READ:
                self._measure(name, site, *m)
        out = self._orig(name, *a)
        for m in live:
            if m[0].kind == COMMITTED:
                self._measure(name, site, *m)
        return out

    def _measure(self, name, site, p, x, slot, rows, cols, ld):
        with self._lock:
            k = len(self.records)
            if k >= self.n_pairs:
                raise RuntimeError("AbsmaxAudit: the cell buffer holds %d pairs; raise n_pairs" % self.n_pairs)
            self.records.append((name, p, site, 2 * k))
        s = self._stream()
        self._lib_call("unreal_absmax_f32", rows, cols, x, ld, self._base + 8 * k, s)
        self._lib_call("unreal_absmax_f32", 1, 1, slot, 1, self._base + 8 * k + 4, s)

    # -- results ----------------------------------------------------------------------------------------
    def violations(self):
        """The pairs that break the contract.  `not (claimed >= true)`: a NaN on either side is a violation too."""
        if self.pairs is None:
            raise RuntimeError("the audit is still open")
        return [p for p in self.pairs if not (p["claimed"] >= p["true"])]

    def describe(self, p):
        t, c = p["true"], p["claimed"]
        ok = t > 0 and c > 0 and math.isfinite(t) and math.isfinite(c)
        gap = "%d binade(s) short" % (binade(t) - binade(c)) if ok else "no binade gap: zero or non-finite"
        return "[%s] %s %s (slot %s, %s) at %s:%d in %s: slot %.9g %s %.9g = max |%s| (%s)" % (
            self.config, p["entry"], p["operand"], p["slot"], p["kind"], p["site"][0], p["site"][1], p["site"][2], c,
            "<" if c < t else "vs", t, p["operand"], gap)

    def assert_clean(self):
        bad = self.violations()
        # one line per (entry, operand, slot, site): a loop over time steps would repeat it T times
        seen, lines = set(), []
        for p in bad:
            key = (p["entry"], p["operand"], p["slot"], p["site"])
            if key not in seen:
                seen.add(key)
                lines.append(self.describe(p))
        assert not bad, "%d of %d audited slots do not cover their operand:\n  %s" % (len(bad), len(self.pairs), "\n  ".join(lines))

    def overcover(self):
        """-> {(entry, operand): dict(binades, true, claimed, site, pairs)}: the worst over-cover of the read pairs,
        floor(log2 claimed) - floor(log2 true); pairs whose true maximum is 0 (or not finite) are skipped."""
        if self.pairs is None:
            raise RuntimeError("the audit is still open")
        out = {}
        for p in self.pairs:
            t, c = p["true"], p["claimed"]
            if p["kind"] != READ or not (t > 0 and c > 0 and math.isfinite(t) and math.isfinite(c)):
                continue
            gap = binade(c) - binade(t)
            row = out.setdefault((p["entry"], p["operand"]), dict(binades=gap, true=t, claimed=c, site=p["site"], pairs=0))
            row["pairs"] += 1
            if gap > row["binades"]:
                row.update(binades=gap, true=t, claimed=c, site=p["site"])
        return out


def merge_overcover(*tables):
    """The worst row per key of several overcover() tables (the passes of one configuration)."""
    out = {}
    for t in tables:
        for k, r in t.items():
            if k not in out:
                out[k] = dict(r)
            else:
                n = out[k]["pairs"] + r["pairs"]
                if r["binades"] > out[k]["binades"]:
                    out[k] = dict(r)
                out[k]["pairs"] = n
    return out


def write_report(config, table, path=REPORT, extra=None):
    """Merge one configuration's overcover table into the JSON report (rows of other configurations are kept)."""
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    rows = [dict(entry=e, operand=o, binades=r["binades"], true=r["true"], claimed=r["claimed"], pairs=r["pairs"],
                 site="%s:%d %s" % tuple(r["site"])) for (e, o), r in sorted(table.items())]
    doc[config] = dict(rows=rows, **(extra or {}))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    return doc


def digest(doc):
    """The report as markdown: one table of every (configuration, entry, operand), worst over-cover first."""
    rows = [(r["binades"], c, r) for c, d in doc.items() for r in d["rows"]]
    rows.sort(key=lambda t: (-t[0], t[1], t[2]["entry"], t[2]["operand"]))
    out = ["| binades | configuration | entry | operand | slot | max of operand | pairs | call site |", "|--:|---|---|---|--:|--:|--:|---|"]
    for b, c, r in rows:
        out.append("| %d | %s | %s | %s | %.6g | %.6g | %d | %s |" % (b, c, r["entry"].replace("unreal_", ""), r["operand"],
                                                                     r["claimed"], r["true"], r["pairs"], r["site"]))
    runs = ["| configuration | audited launches | pairs | violations | seconds |", "|---|--:|--:|--:|--:|"]
    for c in sorted(doc):
        d = doc[c]
        runs.append("| %s | %s | %s | %s | %s |" % (c, d.get("launches"), d.get("pairs"), d.get("violations"), d.get("seconds")))
    return "\n".join(out), "\n".join(runs)


if __name__ == "__main__":      # python -m tests.absmax_audit [report.json]: the two tables of profiles/absmax_audit.md
    with open(sys.argv[1] if len(sys.argv) > 1 else REPORT) as _f:
        print("\n\n".join(digest(json.load(_f))))
