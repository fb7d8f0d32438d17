"""Exploration bonus on the device: unreal_frame_codes bit for bit against the integer host model
(tests/explore_model.py) over frame sizes, cells, row counts and parameters; unreal_count_add / unreal_count_bonus against
the model; unreal_vr_returns_bonus against a numpy fp64 scan; and the Trainer with the option off (nothing changes) and on
(codes, table, rewards, returns and r_bonus rebuilt on the host from what the rollout left on the device)."""
import numpy as np
import pytest
import torch

try:
    import explore_model as EM
    import timelimit_cases as TC
    from test_trainer_gpu import _cfg
except ImportError:            # imported as tests.<module>
    from tests import explore_model as EM
    from tests import timelimit_cases as TC
    from tests.test_trainer_gpu import _cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0xA3C


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _mult(F, seed=SEED):
    from unreal_amd import ops
    m = torch.zeros(F, dtype=torch.int32, device=DEV)
    ops.explore_multipliers(F, seed, m)
    return m


def _as_u64(m):
    return m.cpu().numpy().view(np.uint32).astype(np.uint64)


def test_multipliers_are_the_models():
    for F, seed in ((1323, SEED), (432, 7), (3, (1 << 63) + 5)):
        np.testing.assert_array_equal(_as_u64(_mult(F, seed)), EM.multipliers(F, seed))


# ---- 1. the codes ----------------------------------------------------------------------------------------------------------
def _edge_frames(H, W, cell, levels, vmax, rs):
    """Two frames that differ in one byte: one cell and channel filled to one below the first level edge, and to it."""
    denom = vmax * cell * cell + 1
    edge = -(-denom // levels)                                     # the smallest S with S levels >= denom
    cy, cx, c = rs.randint(H // cell), rs.randint(W // cell), rs.randint(3)
    out = []
    for S in (edge - 1, edge):
        fr = np.zeros((H, W, 3), np.uint8)
        px = fr[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell, c].reshape(-1).copy()
        k, rest = divmod(S, vmax)
        px[:k] = vmax
        if rest:
            px[k] = rest
        fr[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell, c] = px.reshape(cell, cell)
        out.append(fr)
    return out


def _pool(H, W, cells, rs, n_random=24):
    """-> (frames uint8 [n, H, W, 3], the device pool: frame_stride bytes per frame, the stride padding filled with 255)."""
    from unreal_amd import ops
    frames = [np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), np.ones((H, W, 3), np.uint8)]
    frames += [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n_random)]
    frames += [rs.randint(0, 3, (H, W, 3)).astype(np.uint8) for _ in range(8)]           # bytes around vmax = 1
    for cell in cells:
        for levels, vmax in ((8, 255), (8, 1), (2, 255), (64, 255)):
            frames += _edge_frames(H, W, cell, levels, vmax, rs)
    frames = np.stack(frames)
    stride = ops.frame_stride(H, W)
    buf = np.full((len(frames), stride), 255, np.uint8)
    buf[:, :H * W * 3] = frames.reshape(len(frames), -1)
    return frames, _dev(buf.reshape(-1), torch.uint8), stride


def _gate(rows, rs):
    """A rollout gate over `rows` = T B (- 1: one padded row) rows with every (n_steps, terminal_end) pair it can hold."""
    T = 3 if rows >= 3 else 1
    B = -(-rows // T)
    n = rs.randint(1, T + 1, B).astype(np.int32)
    te = rs.randint(0, 3, B).astype(np.int32)
    k = min(B, 3 * T)
    n[:k], te[:k] = (np.arange(k) // 3) % T + 1, np.arange(k) % 3
    act = (np.arange(T)[:, None] < n[None, :]).astype(np.int32)
    act[rs.rand(T, B) < 0.1] = 0                                   # (and rows switched off for no reason)
    earn = EM.earning(act, n, te).reshape(-1)[:rows]
    return B, act.reshape(-1)[:rows].copy(), n, te, earn


SHAPES = [(21, 21, (7, 3)), (24, 36, (4, 12)), (84, 84, (4, 7, 12)), (96, 192, (8, 16))]


@pytest.mark.parametrize("H,W,cells", SHAPES, ids=["21x21", "24x36", "84x84", "96x192-strips"])
def test_frame_codes_are_the_models_bit_for_bit(H, W, cells):
    """21 x 21: a stride of 1328 with 5 bytes of padding (filled with 255); 24 x 36: H != W; 84 x 84: the rings' frames;
    96 x 192: 55296 bytes, more than one LDS strip.  Gated rows carry a negative index: a kernel that read them anyway
    would show up as a code, not as a fault."""
    from unreal_amd import ops
    rs = np.random.RandomState(H * 1000 + W)
    frames, pool, stride = _pool(H, W, cells, rs)
    n_pool = len(frames)
    assert stride % 16 == 0 and (stride > H * W * 3) == (H == 21)
    checked = 0
    for cell in cells:
        F = EM.n_features(H, W, cell)
        mult = _mult(F)
        mult_h = EM.multipliers(F, SEED)
        for levels in (2, 8, 64):
            for vmax in (1, 255):
                lv = EM.levels_of(frames, cell, levels, vmax)
                assert lv.min() == 0 and lv.max() == min(levels - 1, vmax * cell * cell * levels // (vmax * cell * cell + 1))
                for bits in (10, 22):
                    want_pool = EM.codes_of(frames, cell, levels, vmax, bits, mult_h)
                    for rows in (1, 5, 257):
                        B, act, n, te, earn = _gate(rows, rs)
                        idx = rs.randint(0, n_pool, rows).astype(np.int32)          # (257 rows of ~50 frames: repeats)
                        if rows > 1:
                            idx[:min(rows, n_pool)] = rs.permutation(n_pool)[:min(rows, n_pool)]
                        want = np.where(earn, want_pool[idx], -1)
                        idx_d = np.where(earn, idx, -1 - rs.randint(0, 1 << 20, rows)).astype(np.int32)
                        codes = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
                        ops.frame_codes(rows, pool, stride, n_pool, H, W, _dev(idx_d, torch.int32), cell, levels, vmax, bits,
                                        mult, codes, gate=(B, _dev(act, torch.int32), _dev(n, torch.int32),
                                                           _dev(te, torch.int32)))
                        np.testing.assert_array_equal(codes.cpu().numpy(), want, err_msg=str((cell, levels, vmax, bits, rows)))
                        checked += int(earn.sum())
                    # no gate: every row; an index past the pool is refused per row
                    idx = rs.randint(0, n_pool, 5).astype(np.int32)
                    idx[3] = n_pool
                    codes = torch.full((5,), -7, dtype=torch.int32, device=DEV)
                    ops.frame_codes(5, pool, stride, n_pool, H, W, _dev(idx, torch.int32), cell, levels, vmax, bits, mult, codes)
                    want = want_pool[np.minimum(idx, n_pool - 1)]
                    want[3] = -1
                    np.testing.assert_array_equal(codes.cpu().numpy(), want)
    assert checked > 1000


def test_frame_codes_tell_the_level_edge_and_ignore_the_padding():
    """The two edge frames differ in one byte and get different codes; the codes of a 21 x 21 frame do not depend on its
    stride padding."""
    from unreal_amd import ops
    rs = np.random.RandomState(9)
    H = W = 21
    lo, hi = _edge_frames(H, W, 7, 8, 255, rs)
    assert (lo != hi).sum() == 1
    stride = ops.frame_stride(H, W)
    assert stride == 1328
    buf = np.zeros((4, stride), np.uint8)
    buf[0, :1323], buf[1, :1323], buf[2, :1323], buf[3, :1323] = lo.reshape(-1), hi.reshape(-1), hi.reshape(-1), lo.reshape(-1)
    buf[2:, 1323:] = 255
    mult = _mult(27)
    codes = torch.zeros(4, dtype=torch.int32, device=DEV)
    ops.frame_codes(4, _dev(buf.reshape(-1), torch.uint8), stride, 4, H, W, _dev(np.arange(4), torch.int32), 7, 8, 255, 22,
                    mult, codes)
    c = codes.cpu().numpy()
    assert c[0] == 0 and c[1] != 0 and c[2] == c[1] and c[3] == c[0]
    np.testing.assert_array_equal(c[:2], EM.codes_of(np.stack([lo, hi]), 7, 8, 255, 22, EM.multipliers(27, SEED)))


# ---- 2. counts and bonus -----------------------------------------------------------------------------------------------------
def test_count_add_and_count_bonus_against_the_model():
    """257 rows (T = 3, B = 86, one padded row) over 7 distinct frames, a 2^10 table that starts non-zero, actors that end at
    steps 0, 1 and T - 1 with terminal_end 0, 1 and 2.  Table and counts exact; bonus and rewards_total within rel 1e-6 of
    the fp64 model (fp32 sqrt and divide: 0.5 ulp each, 1.2e-7 together; the bar leaves 8x for a sqrt that is not correctly
    rounded); the sum at rel 1e-5 (float atomics in no fixed order)."""
    from unreal_amd import ops
    rs = np.random.RandomState(21)
    H = W = 84
    bits, beta, rows, n_slots = 10, 0.05, 257, 400
    frames = rs.randint(0, 256, (7, H, W, 3)).astype(np.uint8)
    pool = _dev(frames.reshape(-1), torch.uint8)
    mult_h = EM.multipliers(432, SEED)
    code_of_frame = EM.codes_of(frames, 7, 8, 255, bits, mult_h)
    assert len(np.unique(code_of_frame)) == 7
    B, act, n, te, earn = _gate(rows, rs)
    assert B == 86 and {(int(a), int(b)) for a, b in zip(n, te)} == {(a, b) for a in (1, 2, 3) for b in (0, 1, 2)}
    idx = rs.randint(0, 6, rows).astype(np.int32)
    idx[np.flatnonzero(earn)[17]] = 6                              # frame 6: one earning row, and a count that starts at 0
    want_codes = np.where(earn, code_of_frame[idx], -1)
    codes = torch.full((rows + 1,), -7, dtype=torch.int32, device=DEV)
    ops.frame_codes(rows, pool, 21168, 7, H, W, _dev(np.where(earn, idx, -5), torch.int32), 7, 8, 255, bits, _mult(432),
                    codes, gate=(B, _dev(act, torch.int32), _dev(n, torch.int32), _dev(te, torch.int32)))
    np.testing.assert_array_equal(codes.cpu().numpy()[:rows], want_codes)
    assert codes[rows] == -7
    # a table that starts non-zero: on two of the seven codes and on unrelated entries
    table0 = rs.randint(0, 4, 1 << bits).astype(np.int64)
    table0[code_of_frame[0]], table0[code_of_frame[6]] = 40, 0
    table = _dev(table0, torch.int32)
    codes_bad = codes.clone()
    codes_bad[rows] = 1 << bits                                    # a code past the table is skipped, never written
    ops.count_add(rows + 1, codes_bad, table, bits)
    want_table = EM.count_add(table0.copy(), want_codes)
    np.testing.assert_array_equal(table.cpu().numpy(), want_table)
    assert want_table.sum() - table0.sum() == earn.sum() > 100
    # the bonus, a later launch: every row sees the counts after all increments
    rewards = rs.randint(-1, 2, rows).astype(np.float32)
    slots = rs.permutation(n_slots)[:rows].astype(np.int32)
    r_bonus = torch.full((n_slots,), 7.5, device=DEV)
    bonus, total = torch.full((rows,), -3.0, device=DEV), torch.full((rows,), -3.0, device=DEV)
    stats_i, stats_f = _dev(np.array([1000, 10]), torch.int32), _dev(np.array([2.0]), torch.float32)
    ops.count_bonus(rows, codes, table, bits, beta, _dev(rewards, torch.float32), _dev(act, torch.int32),
                    _dev(slots, torch.int32), bonus, total, r_bonus, stats_i, stats_f)
    wb, n_earn, n_first = EM.bonus_of(want_table, want_codes, beta)
    got_b, got_t = bonus.cpu().numpy(), total.cpu().numpy()
    err = np.abs(got_b - wb) / np.where(wb > 0, wb, 1.0)
    print("bonus: max rel error %.3g over %d rows, %d first" % (err.max(), n_earn, n_first))
    assert (got_b[~earn] == 0).all() and err.max() <= 1e-6
    wt = rewards.astype(np.float64) + wb
    err_t = np.abs(got_t - wt)
    print("rewards_total: max error %.3g" % err_t.max())
    assert (err_t <= 1e-6 * np.maximum(np.abs(rewards) + wb, np.abs(wt))).all()
    np.testing.assert_array_equal(stats_i.cpu().numpy(), [1000 + n_earn, 10 + n_first])
    assert n_earn == earn.sum() and n_first >= 1                    # (frame 6's row is a first)
    s = float(stats_f.cpu()[0]) - 2.0
    print("sum of bonus %.7g, model %.7g" % (s, wb.sum()))
    assert abs(s - wb.sum()) <= 1e-5 * wb.sum()
    # r_bonus: written at exactly the active rows' slots (0 on their terminal steps), the sentinel elsewhere
    want_rb = np.full(n_slots, 7.5, np.float32)
    want_rb[slots[act != 0]] = got_b[act != 0]
    np.testing.assert_array_equal(r_bonus.cpu().numpy(), want_rb)
    assert ((act != 0) & ~earn).sum() > 10 and (got_b[(act != 0) & ~earn] == 0).all()
    # without a ring array: no scatter
    ops.count_bonus(rows, codes, table, bits, beta, _dev(rewards, torch.float32), None, None, bonus, total, None, stats_i,
                    stats_f)
    np.testing.assert_array_equal(bonus.cpu().numpy(), got_b)


# ---- 3. value replay ---------------------------------------------------------------------------------------------------------
def test_vr_returns_bonus_is_the_fp64_scan():
    from unreal_amd import ops
    rs = np.random.RandomState(4)
    Bn, L, Hn = 5, 4, 9
    ring = ops.Ring(Bn, Hn, torch.device(DEV), bonus=True)
    plain = ops.Ring(Bn, Hn, torch.device(DEV))
    assert ring.r_bonus is not None and ring.r_bonus.numel() == Bn * (Hn + 1) and plain.r_bonus is None
    view = ops.ring_view(ring, 1, 3)
    assert view.r_bonus.data_ptr() == ring.r_bonus.data_ptr() + 4 * (Hn + 1) and view.r_bonus.numel() == 2 * (Hn + 1)
    assert ops.ring_view(plain, 1, 3).r_bonus is None
    n = Bn * (Hn + 1)
    rew, bon = rs.normal(0, 1, n).astype(np.float32), rs.uniform(0, 0.1, n).astype(np.float32)
    term = np.zeros(n, np.int32)
    seq_len = np.array([L, 1, 2, L, L], np.int32)
    seq_idx = np.stack([rs.permutation(Hn + 1)[:L] + b * (Hn + 1) for b in range(Bn)], axis=1).astype(np.int32)   # [L, B]
    term[seq_idx[L - 2, 3]] = 1                                    # sequence 3: its second-to-last frame is terminal
    boot = rs.normal(0, 1, Bn).astype(np.float32)
    gamma = 0.99
    for r in (ring, plain):
        r.r_reward.copy_(_dev(rew, torch.float32)); r.r_terminal.copy_(_dev(term, torch.int32))
    args = (L, _dev(seq_idx.reshape(-1), torch.int32), _dev(seq_len, torch.int32), _dev(boot, torch.float32), gamma)
    out0, out1, out2, out3 = (torch.full(((L - 1) * Bn,), 9.0, device=DEV) for _ in range(4))
    ops.vr_returns(plain, *args, out0)
    ops.vr_returns(ring, *args, out1)                              # the default stays the extrinsic call
    ops.vr_returns(ring, *args, out2, bonus=True)                  # r_bonus = 0: bit-identical
    ops.vr_returns(plain, *args, out3, bonus=True)                 # no r_bonus: the extrinsic call
    for o in (out1, out2, out3):
        assert torch.equal(o, out0)
    ring.r_bonus.copy_(_dev(bon, torch.float32))
    ops.vr_returns(ring, *args, out2, bonus=True)
    want = np.zeros((L - 1, Bn))
    for b in range(Bn):
        m = seq_len[b]
        R = 0.0 if (m >= 2 and term[seq_idx[m - 2, b]]) else float(boot[b])
        for t in range(m - 2, -1, -1):
            R = (float(rew[seq_idx[t, b]]) + float(bon[seq_idx[t, b]])) + gamma * R
            want[t, b] = R
    got = out2.cpu().numpy().reshape(L - 1, Bn).astype(np.float64)
    assert (np.abs(got - want) <= TC.ulp32(want)).all(), np.abs(got - want).max()
    assert (got[:, 1] == 0).all() and (got[1:, 2] == 0).all() and np.abs(got - out0.cpu().numpy().reshape(L - 1, Bn)).max() > 1e-3
    assert want[L - 2, 3] == float(rew[seq_idx[L - 2, 3]]) + float(bon[seq_idx[L - 2, 3]])      # no bootstrap there


# ---- 4. the trainer ----------------------------------------------------------------------------------------------------------
LAYOUT = ["S-----G", "-+-+-+-", "-------", "-+-+-+-", "-------", "-+-+-+-", "-------"]


def _register(env_type, name):
    from unreal_amd.environment.environment import Environment
    if env_type == "arcade":
        Environment.register_arcade_config(name, **dict(TC.BREAKOUT, max_episode_steps=9))
    else:
        Environment.register_maze_config(name, layouts=["".join(LAYOUT)], view="first_person", random_start=True,
                                         max_episode_steps=3)


def _unregister(env_type, name):
    from unreal_amd.environment.environment import Environment
    (Environment.ARCADE_CONFIG if env_type == "arcade" else Environment.MAZE_CONFIG).pop(name, None)


def _trainer(env_type, env_name, Bn, T, Hn, lstm=True, aux=False, groups=1, seed=4, fill=True, **options):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    cfg = _cfg(lstm, aux, Hn, T)
    Environment.action_size = -1
    net = UnrealModel(Environment.get_action_size(env_type, env_name), 0, -1, lstm, aux, aux, aux, 0.05, 0.001, DEV, seed=seed)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    tr = Trainer(0, net, 7.0711e-4, None, applier, env_type, env_name, lstm, aux, aux, aux, 0.05, 0.001, T, T,
                 cfg["gamma"], cfg["gamma_pc"], Hn, 10 ** 6, DEV, batch_size=Bn, groups=groups, seed=SEED, **options)
    tr.prepare()
    while fill and not tr._full:
        tr.process(None, 0)
    return net, applier, tr


def test_trainer_with_the_option_off_is_todays_trainer():
    """explore_beta = 0 against no argument: the same keys, nothing allocated, and the same parameters bit for bit after two
    calls (one actor, auxiliary heads off, the first-person maze with a step limit of 3: the case in which two runs of the
    trainer repeat bit for bit, tests/test_reuse_gpu.py and DESIGN §7q)."""
    name = "explore_off"
    _register("maze", name)
    try:
        runs = []
        for options in ({}, dict(explore_beta=0.0, explore_cell=4, explore_levels=16, explore_bits=12)):
            net, applier, tr = _trainer("maze", name, 1, 5, 16, **options)
            for k in range(2):
                steps, _ = tr.process(None, 0)
                assert steps > 0
            assert tr.full_ring.r_bonus is None and not hasattr(tr, "explore_table") and not hasattr(tr, "rewards_total")
            runs.append((sorted(tr.last_losses), net.params.flat.cpu().numpy().copy(), dict(tr.last_losses)))
            with pytest.raises(ValueError, match="explore_beta"):
                tr.explore_counts()
        assert runs[0][0] == runs[1][0] and "explore_bonus" not in runs[0][0] and "explore_first" not in runs[0][0]
        np.testing.assert_array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))
        assert runs[0][2] == runs[1][2]
    finally:
        _unregister("maze", name)


def _nstep_scan(rewards, values, n_steps, boot_v, terminal_end, gamma):
    """unreal_base_returns in numpy fp64; [T, B] inputs -> (R, adv)."""
    T, n = rewards.shape
    R, adv = np.zeros((T, n)), np.zeros((T, n))
    for b in range(n):
        acc = 0.0 if terminal_end[b] else float(boot_v[b])
        for t in range(int(n_steps[b]) - 1, -1, -1):
            acc = float(rewards[t, b]) + gamma * acc
            R[t, b], adv[t, b] = acc, acc - float(values[t, b])
    return R, adv


CASES = [("maze", True, 1, {}), ("maze", True, 2, {}), ("maze", False, 1, {}), ("maze", False, 2, {}),
         ("arcade", True, 2, dict(bootstrap_timeouts=True))]


@pytest.mark.parametrize("env_type,lstm,groups,options", CASES,
                         ids=["maze-lstm-g1", "maze-lstm-g2", "maze-ff-g1", "maze-ff-g2", "arcade-tl-g2"])
def test_trainer_bonus_is_rebuilt_on_the_host(env_type, lstm, groups, options):
    """Three process() calls on a first-person maze with a step limit of 3 (the arcade: 9, with time-limit bootstrapping).
    After every group's rollout the test reads back what it left on the device and rebuilds codes, the running table,
    rewards_total, R / adv and r_bonus from the frames."""
    name = "explore_%s_%d%d" % (env_type, lstm, groups)
    _register(env_type, name)
    try:
        Bn, T, Hn, beta, bits, cell, levels = 4, 5, 50, 0.0625, 12, 7, 8
        net, applier, tr = _trainer(env_type, name, Bn, T, Hn, lstm=lstm, groups=groups, explore_beta=beta,
                                    explore_bits=bits, explore_cell=cell, explore_levels=levels, **options)
        Bg, H1 = tr.Bg, Hn + 1
        assert tr.explore_vmax == 255 and tr.full_ring.r_bonus is not None and tr.explore_counts() is tr.explore_table
        assert tr.explore_table.numel() == 1 << bits and int(tr.explore_table.sum()) == 0          # the fill counts nothing
        assert (tr.full_ring.r_bonus == 0).all()
        mult_h = EM.multipliers(432, SEED)
        np.testing.assert_array_equal(_as_u64(tr.explore_mult), mult_h)
        table = np.zeros(1 << bits, np.int64)
        want_rb = np.zeros(Bn * H1, np.float32)
        snaps = []
        apply_update = tr._apply_update

        def snapshot(lr):                                           # called by process() right after a group's gradients
            ring = tr.ring
            snaps.append(dict(
                g=tr.group, frames=ring.frames[:Bg * H1 * 21168].view(Bg * H1, 21168).cpu().numpy(),
                idx=tr.base_ws.frame_idx[:T * Bg].cpu().numpy().reshape(T, Bg), count=ring.count.cpu().numpy(),
                act=tr.active_log.cpu().numpy().reshape(T, Bg), n=tr.n_steps.cpu().numpy(), te=tr.terminal_end.cpu().numpy(),
                r=tr.rewards.cpu().numpy().reshape(T, Bg), v=tr.v.cpu().numpy().reshape(T, Bg), boot=tr.boot_v.cpu().numpy(),
                R=tr.R.cpu().numpy().reshape(T, Bg), adv=tr.adv.cpu().numpy().reshape(T, Bg),
                total=tr.rewards_total.cpu().numpy().reshape(T, Bg), codes=tr.explore_codes.cpu().numpy().reshape(T, Bg),
                bonus=tr.explore_bonus.cpu().numpy().reshape(T, Bg), table=tr.explore_table.cpu().numpy(),
                r_bonus=tr.full_ring.r_bonus.cpu().numpy(), r_reward=tr.full_ring.r_reward.cpu().numpy(),
                score=tr.full_ring.score_out.cpu().numpy()))
            apply_update(lr)

        tr._apply_update = snapshot
        earned = ended = 0
        for call in range(3):
            snaps.clear()
            steps, _ = tr.process(None, call * Bn * T)
            assert [s["g"] for s in snaps] == list(range(groups))
            call_earn = call_first = 0
            call_bonus = 0.0
            for s in snaps:
                b0 = s["g"] * Bg
                earn = EM.earning(s["act"], s["n"], s["te"])
                assert (s["act"] == (np.arange(T)[:, None] < s["n"][None, :])).all()
                # the next observation: the frame the next row read; of the last row, the actor's current slot
                nxt = np.concatenate([s["idx"][1:], (np.arange(Bg) * H1 + s["count"] % H1)[None, :]])
                frames = s["frames"][np.where(earn, nxt, 0)].reshape(T, Bg, 84, 84, 3)
                codes = EM.codes_of(frames.reshape(T * Bg, 84, 84, 3), cell, levels, 255, bits, mult_h).reshape(T, Bg)
                codes = np.where(earn, codes, -1)
                np.testing.assert_array_equal(s["codes"], codes)
                EM.count_add(table, codes)
                np.testing.assert_array_equal(s["table"], table)                 # over every call and group so far
                wb, n_earn, n_first = EM.bonus_of(table, codes, beta)
                assert (s["bonus"][~earn] == 0).all()
                assert (np.abs(s["bonus"] - wb) <= 1e-6 * wb).all()
                # rewards_total = extrinsic + bonus; self.rewards, the ring's r_reward and the scores stay extrinsic
                assert (s["r"] == np.round(s["r"])).all() and (s["score"] == np.round(s["score"])).all()
                np.testing.assert_array_equal(s["total"], (s["r"] + s["bonus"]).astype(np.float32))
                live = s["act"] != 0
                np.testing.assert_array_equal(s["r_reward"][b0 * H1 + s["idx"][live]], s["r"][live])
                # R / adv: the fp64 scan of rewards_total, at the bars of tests/test_timelimit_gpu.py
                if options.get("bootstrap_timeouts"):
                    wR, wadv = TC.gae_scan(s["total"], s["v"], s["n"], s["boot"], s["te"], tr.gamma, 1.0)
                else:
                    wR, wadv = _nstep_scan(s["total"], s["v"], s["n"], s["boot"], s["te"], tr.gamma)
                for got, want in ((s["R"], wR), (s["adv"], wadv)):
                    assert (np.abs(got.astype(np.float64) - want) <= TC.ulp32(want)).all(), np.abs(got - want).max()
                # r_bonus: the rollout's slots, 0 on a step that ends an episode, nothing else touched
                want_rb[b0 * H1 + s["idx"][live]] = s["bonus"][live]
                np.testing.assert_array_equal(s["r_bonus"], want_rb)
                call_earn, call_first, call_bonus = call_earn + n_earn, call_first + n_first, call_bonus + s["bonus"].sum()
                ended += int((live & ~earn).sum())
            assert steps == sum(int(s["n"].sum()) for s in snaps)
            l = tr.last_losses
            assert call_earn > 0 and l["explore_first"] == call_first / call_earn
            assert abs(l["explore_bonus"] - call_bonus / call_earn) <= 1e-5 * beta
            earned += call_earn
        assert int(table.sum()) == earned and ended > 0 and (table > 1).any()
        if options.get("bootstrap_timeouts"):
            assert tr.full_ring.final_obs is not None
    finally:
        _unregister(env_type, name)


def test_full_unreal_run_with_reuse_and_groups():
    name = "explore_full"
    _register("maze", name)
    try:
        beta = 0.0625
        net, applier, tr = _trainer("maze", name, 4, 5, 50, lstm=True, aux=True, groups=2, explore_beta=beta,
                                    reuse_epochs=2)
        for call in range(3):
            tr.process(None, call * 20)
            l = tr.last_losses
            assert all(np.isfinite(v) for v in l.values()), l
            assert 0 < l["explore_first"] <= 1 and 0 < l["explore_bonus"] <= beta, l
            assert "clip_fraction" in l and "vr_loss" in l
        assert torch.isfinite(net.params.flat).all()
        # counted once per rollout, not per epoch: the table holds as many counts as rows earned
        assert 0 < int(tr.explore_table.sum()) <= 3 * 4 * 5
        assert float(tr.full_ring.r_bonus.max()) > 0 and float(tr.full_ring.r_bonus.max()) <= beta
    finally:
        _unregister("maze", name)
