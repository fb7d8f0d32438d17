"""CPU tests of the host logic and the C-ABI boundary (no GPU, no compute calls):
  * libunreal_hip.so loads and exports every symbol include/unreal_hip.h declares
  * the product path fails loudly without a GPU (no CPU fallback anywhere)
  * flags keep the reference's names/defaults; parameter layout matches the reference's census
  * learning-rate schedule, Philox stream bookkeeping."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from unreal_amd.build import build_library
    return build_library(verbose=False)


def test_library_exports_every_declared_symbol(built):
    from unreal_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 35
    dll = ctypes.CDLL(built)
    for name, args in protos.items():
        assert hasattr(dll, name), name
        assert args[-1] is ctypes.c_void_p, "every entry point takes the stream last: %s" % name
    L = _lib.lib()
    assert set(L.protos) == set(protos)
    # every exported unreal_* symbol is declared (no undocumented entry points)
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", built], stdout=subprocess.PIPE).stdout.decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T unreal_" in l}
    assert exported == set(protos), exported ^ set(protos)


def test_invalid_arguments_and_maze_tails_are_rejected_without_launch(built):
    from unreal_amd import _lib
    L = _lib.lib()
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_gemm_f32", 0, 0, 0, 4, 4, None, 4, None, 4, None, 4, None, None, 0, 0, 1, None)
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_maze_step", 0, 3, *([None] * 18), 1, 0, 0, 7, None, 0, *([None] * 5), None)
    # a well-formed step except for its maze tail (view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading):
    # refused on the host, so these fake device pointers never reach a kernel
    dev = 1 << 20
    step = [4, 3, dev, None] + [dev] * 11 + [None, None] + [dev] * 3 + [1, 1]
    for tail in ([1, 7, None, 0] + [dev] * 5,           # first person needs a configuration block
                 [2, 7, dev, 0] + [dev] * 5,            # no such view
                 [0, 12, None, 0] + [None] * 5):        # the reference's map is 7 x 7
        assert L._fn["unreal_maze_step"](*step, *tail, None) == -22, tail
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_rmsprop_step", None, None, None, None, 10, 0.1, 0.9, 0.0, 0.1, 40.0, None, None)


def test_no_cpu_fallback():
    from unreal_amd import ops
    x = torch.zeros(16)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.colsum(4, 4, x, 4, torch.zeros(4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.gemm(0, 0, 4, 4, 4, x, 4, x, 4, x, 4)
    if not torch.cuda.is_available():
        from unreal_amd.model.model import UnrealModel
        with pytest.raises(Exception):
            UnrealModel(4, 0, -1, True, True, True, True, 0.05, 0.001, "cuda:0")


def test_product_never_imports_the_oracle():
    import re
    for dirpath, _, files in os.walk(os.path.join(ROOT, "unreal_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), os.path.join(dirpath, f)


def test_options_keep_reference_names_and_defaults():
    from unreal_amd.options import get_options
    f = get_options("training")                       # options_lab.py preset
    want = dict(use_lstm=True, use_pixel_change=True, use_value_replay=True, use_reward_prediction=True,
                segnet=0, parallel_size=8, local_t_max=20, n_step_TD=20, entropy_beta=0.001, rmsp_alpha=0.99,
                rmsp_epsilon=0.1, initial_alpha_low=1e-4, initial_alpha_high=5e-3, initial_alpha_log_rate=0.5,
                gamma=0.99, gamma_pc=0.9, pixel_change_lambda=0.05, experience_history_size=2000,
                max_time_step=13200000, save_interval_step=100000, grad_norm_clip=40.0, env_type="lab",
                env_name="nav_maze_static_01", termination_time_sec=50.0, greedy_epsilon=0.99)
    for k, v in want.items():
        assert getattr(f, k) == v, k
    d = get_options("training", preset="default")     # options.py
    assert (d.use_pixel_change, d.segnet, d.n_step_TD, d.entropy_beta, d.n_classes, d.dropout) == \
        (False, 2, 50, 0.0001, 19, 0.0)
    g = get_options("training", argv=["--env_type", "maze", "--use_lstm", "False", "--unknown_flag", "1"])
    assert g.env_type == "maze" and g.use_lstm is False
    assert hasattr(get_options("display"), "frame_save_dir") and hasattr(get_options("evaluate"), "split")


def test_param_layout_matches_reference_census():
    from unreal_amd.model.model import param_spec, ALIGN
    spec = param_spec(4)
    assert len(spec) == 20 and sum(int(np.prod(s)) for _, s, _ in spec) == 1898877
    assert len(param_spec(1, 0, True, True, False, False)) == 18      # model/model_test.py:14-58
    assert len(param_spec(1, 0, True, False, True, False)) == 12
    assert len(param_spec(1, 0, True, False, False, True)) == 14
    assert sum(int(np.prod(s)) for _, s, _ in param_spec(4, 0, False, False, False, False)) == 676405
    names = [n for n, _, _ in spec]
    assert names[:8] == ["W_base_conv1", "b_base_conv1", "W_base_conv2", "b_base_conv2", "W_base_fc1",
                         "b_base_fc1", "lstm_kernel", "lstm_bias"]
    assert dict((n, s) for n, s, _ in spec)["lstm_kernel"] == (517, 1024)
    off = 0
    for _, shape, _ in spec:
        assert off % ALIGN == 0
        off += (int(np.prod(shape)) + ALIGN - 1) // ALIGN * ALIGN


def test_learning_rate_schedule_and_draw_streams():
    from unreal_amd.train.trainer import Trainer, PhiloxDraws, log_uniform
    lr0 = log_uniform(1e-4, 5e-3, 0.5)
    assert abs(lr0 - 7.0711e-4) < 1e-8
    t = object.__new__(Trainer)
    t.initial_learning_rate, t.max_global_time_step = lr0, 13200000
    assert t._anneal_learning_rate(0) == lr0
    assert abs(t._anneal_learning_rate(6600000) - lr0 / 2) < 1e-12
    assert t._anneal_learning_rate(14000000) == 0.0
    # ranks share the stream ids and read disjoint columns [rank*B, (rank+1)*B) of each global draw
    a, b = PhiloxDraws(1, rank=0, batch=8, world_size=2), PhiloxDraws(1, rank=1, batch=8, world_size=2)
    sa = [a._next() for _ in range(1000)]
    sb = [b._next() for _ in range(1000)]
    assert sa == sb and len(set(sa)) == 1000
    assert (a.batch, a.stride, a.col0) == (8, 16, 0) and (b.batch, b.stride, b.col0) == (8, 16, 8)
    p = PhiloxDraws(1)
    assert (p.batch, p.stride, p.col0) == (None, None, 0)


def test_oracle_indoor_contract_and_objective_concat():
    """indoor_environment.py:63-139 contract of the oracle wrapper + experience.py:35-46 with an objective vector."""
    from oracle.experience import concat_action_and_reward, Frame
    from oracle.hostfed import OracleIndoorEnv
    from unreal_amd.environment.synthetic_sim import SyntheticIndoorSim, SyntheticBatchIndoorSimulator
    v = concat_action_and_reward(2, 3, -0.25, np.array([0.5, -1.0]))
    np.testing.assert_array_equal(v, [0, 0, 1, -0.25, 0.5, -1.0])
    kw = dict(episode_len=4, reward_p=0.3, big_reward_p=0.1, objective_size=2, termination_time=50.0)
    env = OracleIndoorEnv(SyntheticIndoorSim(7, **kw), 50.0)
    s0 = env.last_state
    assert s0['image'].dtype == np.float32 and s0['image'].max() <= 1.0 and s0['objective'].shape == (2,)
    f = Frame(s0, 0.5, 1, False, None, 0, 0)
    np.testing.assert_array_equal(f.get_last_action_reward(3)[4:], s0['objective'])
    np.testing.assert_array_equal(f.get_action_reward(3), np.concatenate(([0, 1, 0, 0.5], s0['objective'])))
    seen = []
    for t in range(4):
        prev = env.last_state
        state, r, term, pc = env.process(t % 3)
        seen.append(r)
        assert abs(r) <= 0.5 and (r * 8.0) == round(r * 8.0)          # raw / termination_time, exact in fp32
        if term:
            assert t == 3 and state is prev and float(pc.max()) == 0.0   # :123-124: previous state, objective included
        else:
            assert state is not prev and pc.shape == (20, 20)
    # the batched simulator is B independent actors (same streams), objectives included
    batch = SyntheticBatchIndoorSimulator(2, seed=5, **kw)
    singles = [SyntheticIndoorSim(5 * 100003 + b, **kw) for b in range(2)]
    fr, ob = batch.reset()
    for b, s_ in enumerate(singles):
        o, m = s_.reset()
        np.testing.assert_array_equal(fr[b], o); np.testing.assert_array_equal(ob[b], m)
    for t in range(6):
        fr, rw, tm, ob = batch.step(np.array([t % 3, (t + 1) % 3]))
        for b, s_ in enumerate(singles):
            o, r, term, m = s_.step([t % 3, (t + 1) % 3][b])
            if term:
                o, m = s_.reset()
            np.testing.assert_array_equal(fr[b], o); np.testing.assert_array_equal(ob[b], m)
            assert rw[b] == np.float32(r) and tm[b] == int(term)


def test_environment_objective_size_registry():
    from unreal_amd.environment.environment import Environment
    assert Environment.get_objective_size('maze', '') == 0 and Environment.get_objective_size('indoor', 'nope') == 0
    Environment.register_indoor_config('rooms_test', 7)
    assert Environment.get_objective_size('indoor', 'rooms_test') == 7
    from unreal_amd.model.model import param_spec, xcat_ld
    spec = dict((n, s) for n, s, _ in param_spec(3, 7))
    assert spec["lstm_kernel"] == (256 + 3 + 1 + 7 + 256, 1024) and xcat_ld(3, 7) == 272 and xcat_ld(4, 0) == 264


def test_wgrad_splitk_is_a_multiple_of_8_at_trainer_shapes():
    """The wgrad kernel deals whole K slabs to the 8 XCDs: slab counts that are not a multiple of 8 leave XCDs idle."""
    from unreal_amd.model.model import _splitk
    for M, N, K in ((2592, 256, 81920), (256, 1024, 81920), (256, 1024, 77824), (256, 2592, 81920), (256, 1024, 4096)):
        sk = _splitk(M, N, K)
        assert sk % 8 == 0 and 8 <= sk <= (K + 31) // 32 // 4
    assert _splitk(256, 1024, 60) == 1 and _splitk(2592, 256, 40) == 1        # tiny test batches: no split


def test_few_rows_slab_rule_and_new_entries_reject_bad_arguments(built):
    """ops.slab_count (which launches of the fc product run as K slabs + ordered sum) is host logic; the round-4 entry
    points refuse null / undersized buffers before any launch."""
    from unreal_amd import _lib, ops
    assert [ops.slab_count(m, 256, 2592) for m in (1, 8, 512, 513, 1024, 2048, 2049, 4096)] == [8, 8, 8, 4, 4, 2, 0, 0]
    assert ops.slab_count(512, 2592, 256) == 0 and ops.slab_count(512, 256, 1023) == 0       # short K: nothing to cut
    L = _lib.lib()
    with pytest.raises(_lib.UnrealLibError):      # no partials buffer
        L.call("unreal_gemm_f32_split_nt_slabs", 8, 256, 2592, None, 2592, None, None, 2592, 0, None, None, 256, None, None, 0, 8,
               None, 0, None)
    with pytest.raises(_lib.UnrealLibError):      # null block
        L.call("unreal_encoder_prepare", None, None, None, 1.0, None, 0, None)
    with pytest.raises(_lib.UnrealLibError):      # N = 0
        L.call("unreal_pc_deconv_train", 0, 4, *([None] * 9), 0.05, 1.0, *([None] * 8), None)
    assert ops.ENC_PREPARED_BYTES == 45072


def test_integration_doc_names_every_entry_point():
    """INTEGRATION.md is the map from the reference's calls to the C ABI: an entry point it does not mention is one a
    maintainer cannot find."""
    from unreal_amd import _lib
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [n for n in _lib.parse_header() if n not in text and n.replace("unreal_philox_", "_") not in text]
    assert not missing, missing


def test_smoke_entry_can_import_its_test_helpers(tmp_path):
    """__graft_entry__.smoke() borrows helpers from tests/test_trainer_gpu.py, importing it as `tests.test_trainer_gpu` from a
    process whose sys.path holds the repo root only (the driver's call): every module-level import of that file must
    resolve there (round 4: `import margins` did not)."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import importlib; "
            "m = importlib.import_module('tests.test_trainer_gpu'); assert hasattr(m, '_build') and hasattr(m.margins, 'record')" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]


def test_every_launch_label_has_a_dispatch_case():
    """Each kernel variant a launcher can choose names itself (UNREAL_LAUNCHED in csrc/*.hip); tests/test_dispatch_gpu.py
    pins each one against float64 on the GPU.  A variant added without a case there fails here, on a machine with no GPU;
    a case whose label no launcher records any more fails too."""
    import glob
    import re
    from tests.test_dispatch_gpu import CASES, case_labels
    in_source = set()
    for path in glob.glob(os.path.join(ROOT, "unreal_amd", "csrc", "*.hip")):
        src = open(path).read()
        for m in re.finditer(r"\bUNREAL_LAUNCHED\(((?:[^()]|\([^()]*\))*)\)", src):
            in_source |= set(re.findall(r'"([^"]*)"', m.group(1)))
    assert len(in_source) >= 30, sorted(in_source)
    in_cases = {lab for c in CASES for lab in case_labels(c)}
    assert not in_source - in_cases, sorted(in_source - in_cases)
    assert not in_cases - in_source, sorted(in_cases - in_source)
    assert max(len(l) for l in in_source) < 64                     # ops.last_launch reads through a 64-byte buffer


def test_last_launch_is_host_bookkeeping(built):
    """unreal_last_launch needs no device: before this thread launched anything its label is empty (the label is per
    thread); a missing or empty buffer is refused."""
    from unreal_amd import _lib
    import threading
    L = _lib.lib()
    out = {}

    def fresh_thread():
        buf = ctypes.create_string_buffer(b"x" * 15, 16)
        L.call("unreal_last_launch", buf, 16, None)
        out["label"] = buf.value
    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert out["label"] == b""
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_last_launch", None, 16, None)
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_last_launch", ctypes.create_string_buffer(4), 0, None)
