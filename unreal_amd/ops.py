"""Host-side launch wrappers: torch tensors in, libunreal_hip.so kernels out.

PyTorch is used for device memory and streams only; every computation below is a hand-written
gfx950 kernel.  Each wrapper validates dtypes / sizes on the host before launching (a kernel that
indexes out of bounds can take the whole GPU host down).
"""
import torch

from ._lib import lib, ptr, stream

FRAME_BYTES = 21168
PC_CELLS = 400
F2_DIM = 2592
C1_DIM = 6400
GEMM_RELU, GEMM_ACCUM, GEMM_ATOMIC, GEMM_RELU_MASK, GEMM_RELU_BITS = 1, 2, 4, 8, 16
RELU_WORDS = 162                      # uint16 words of ReLU bits per frame (2592 / 16)

FRAME_SHAPE = (84, 84)                # maze, Lab, gym and the default indoor frame
FRAME_HW_MIN, FRAME_HW_MAX = 20, 480  # frame sizes of the indoor contract (encoder_hw_fwd / hostfed_step)


def frame_dims(H, W):
    """Conv trunk widths of an H x W x 3 frame (model.py:786-787, VALID): (h1, w1, h2, w2, F = 32 * h2 * w2).
    Raises ValueError outside 20 <= H, W <= 480."""
    H, W = int(H), int(W)
    if not (FRAME_HW_MIN <= H <= FRAME_HW_MAX and FRAME_HW_MIN <= W <= FRAME_HW_MAX):
        raise ValueError("frame size %dx%d: supported are %d <= H, W <= %d" % (H, W, FRAME_HW_MIN, FRAME_HW_MAX))
    h1, w1 = (H - 8) // 4 + 1, (W - 8) // 4 + 1
    h2, w2 = (h1 - 4) // 2 + 1, (w1 - 4) // 2 + 1
    return h1, w1, h2, w2, 32 * h2 * w2


def frame_stride(H, W):
    """Bytes between two H x W x 3 frames of a ring or staging buffer: H * W * 3 rounded up to 16 (the ingest kernels
    copy 16 B per lane).  84 x 84 gives FRAME_BYTES."""
    return (int(H) * int(W) * 3 + 15) // 16 * 16


_DT = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8, "f64": torch.float64, "i16": torch.int16}


def _chk(t, dt, n=None, name="tensor", optional=False):
    if t is None:
        if optional:
            return
        raise ValueError("%s is required" % name)
    if not t.is_cuda:
        raise ValueError("%s must be a CUDA/HIP tensor (no CPU fallback)" % name)
    if t.dtype != _DT[dt]:
        raise ValueError("%s: dtype %s, expected %s" % (name, t.dtype, dt))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if n is not None and t.numel() < n:
        raise ValueError("%s: %d elements, need >= %d" % (name, t.numel(), n))


_TIMER = None     # {"name", "events": [(start, end, units)]} while bench.py times one kernel with HIP events


def _call(name, *a):
    if _TIMER is not None and name == _TIMER["name"]:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        lib().call(name, *a, stream())
        e1.record()
        _TIMER["events"].append((e0, e1, a[0]))
        return
    lib().call(name, *a, stream())


def last_launch():
    """Label of the kernel variant the calling thread's most recent launch of this library used ("" before the first),
    e.g. "split_nt 128x128 vec" or "bptt kw2": host bookkeeping only, no device work and no sync."""
    import ctypes
    buf = ctypes.create_string_buffer(64)
    lib().call("unreal_last_launch", buf, len(buf), None)
    return buf.value.decode()


def kernel_timer_start(name):
    """Bracket every launch of kernel entry point `name` with HIP events on the launch stream."""
    global _TIMER
    _TIMER = {"name": name, "events": []}


def kernel_timer_stop():
    """-> {"launches", "ms" (sum of launch durations), "units" (sum of each launch's first size argument)}."""
    global _TIMER
    t, _TIMER = _TIMER, None
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1, _ in t["events"])
    return {"name": t["name"], "launches": len(t["events"]), "ms": ms, "units": sum(u for _, _, u in t["events"])}


# ---- environment ---------------------------------------------------------------------------------
class Ring(object):
    """Device replay ring + per-actor environment state (layout: include/unreal_hip.h)."""

    def __init__(self, B, H, device, objective_size=0, frame_shape=FRAME_SHAPE, maze_state=False, nav=False, gen=0,
                 gen_styled=False, sense=0, arcade=False, final_obs=False, depth=False, bonus=False, arcade_stats=False):
        self.B, self.H, self.H1 = B, H, H + 1
        self.objective_size = objective_size
        self.frame_shape = (int(frame_shape[0]), int(frame_shape[1]))
        if self.frame_shape != FRAME_SHAPE:
            frame_dims(*self.frame_shape)                    # raises outside the supported sizes
        self.frame_stride = frame_stride(*self.frame_shape)
        n = B * self.H1
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)
        # `final_obs` (time-limit bootstrapping): B more frames behind the ring's, slot final_base + b keeps the
        # final observation of actor b's last episode that the step limit cut off; the encoder reads it by that index
        self.final_base = n
        self.frames = torch.empty((n + (B if final_obs else 0)) * self.frame_stride, dtype=torch.uint8, device=device)
        self.final_obs = self.frames[n * self.frame_stride:] if final_obs else None
        self.r_reward = z(n)
        self.r_action = z(n, dt=torch.int32)
        self.r_terminal = z(n, dt=torch.int32)
        self.r_last_action = z(n, dt=torch.int32)
        self.r_last_reward = z(n)
        self.r_pc = torch.empty(n * PC_CELLS, dtype=torch.float32, device=device)
        self.r_objective = z(n * objective_size) if objective_size else None
        # depth prediction, first-person mazes only: the 12 depth classes of every slot's view
        # (unreal_maze_depth_labels), allocated only when asked
        if depth and not maze_state:
            raise ValueError("depth labels are kept for first-person device mazes only (Ring(maze_state=True, depth=True))")
        self.r_depth = z(n * DEPTH_POSITIONS, dt=torch.uint8) if depth else None
        # exploration bonus: the bonus of the step stored in every slot, beside r_reward (unreal_count_bonus),
        # allocated only when asked
        self.r_bonus = z(n) if bonus else None
        self.pos = z(B * 2, dt=torch.int32)
        self.last_action = z(B, dt=torch.int32)
        self.last_reward = z(B)
        self.count = z(B, dt=torch.int32)
        self.episode_reward = z(B)
        self.score_out = z(B)
        self.score_valid = z(B, dt=torch.int32)
        # configured mazes only (environment/maze_environment.MazeConfig): goal cell (x, y), layout id, steps of the
        # running episode, episode index (-1 before the first reset)
        self.goal = z(B * 2, dt=torch.int32) if maze_state else None
        self.layout = z(B, dt=torch.int32) if maze_state else None
        self.ep_steps = z(B, dt=torch.int32) if maze_state else None
        self.episode = torch.full((B,), -1, dtype=torch.int32, device=device) if maze_state else None
        # first-person views (MazeConfig(view="first_person")): heading 0: +x, 1: +y, 2: -x, 3: -y
        self.heading = z(B, dt=torch.int32) if maze_state else None
        # navigation mazes (MazeConfig.nav): [B, 8] records (heading, apple bits lo, hi, goals_total, apples_total, 0, 0, 0)
        # handed to the kernels in place of `heading`, which is then a [B] view of their word 0
        # (`sense` = N: a goal-sense maze, DESIGN §7i: words 5..7 are gf, gs, d and every record, a generated maze's too,
        # ends in the actor's distance field of dist_words(N) words)
        self.sense_n = int(sense) if maze_state else 0
        self.nav_words = NAV_RECORD + dist_words(self.sense_n)
        self.nav = z(B * self.nav_words, dt=torch.int32) if maze_state and (nav or self.sense_n) else None
        if self.nav is not None:
            self.heading = self.nav.view(B, self.nav_words)[:, 0]
        # generated mazes (MazeConfig.generate = N = `gen`): [B, gen_record_words(N)] records (the 8 words above, then the
        # actor's own layout record and apple record, rewritten by every reset), handed to the kernels in place of `heading`
        # (`gen_styled`: a styled config, DESIGN §7h: the record also ends in the actor's style_words(N) nibble words)
        self.gen_n = int(gen) if maze_state else 0
        self.gen_words = gen_record_words(self.gen_n, bool(gen_styled)) + (dist_words(self.sense_n) if self.gen_n else 0)
        self.gen = z(B * self.gen_words, dt=torch.int32) if self.gen_n else None
        if self.gen is not None:
            self.nav = None
            self.heading = self.gen.view(B, -1)[:, 0]

        # device arcade (environment/arcade_environment.ArcadeConfig): steps of the running episode, episode
        # index (-1 before the first reset) and the [B, ARCADE_RECORD] game records
        self.arcade = z(B * ARCADE_RECORD, dt=torch.int32) if arcade else None
        if arcade:
            self.ep_steps = z(B, dt=torch.int32)
            self.episode = torch.full((B,), -1, dtype=torch.int32, device=device)
        # game mixtures: per actor, the sum of its finished episodes' scores and their number, allocated only
        # when asked (the _mix entries add to them where an episode ends)
        if arcade_stats and not arcade:
            raise ValueError("per-task statistics are the device arcade's (Ring(arcade=True, arcade_stats=True))")
        self.done_return = z(B) if arcade_stats else None
        self.done_episodes = z(B, dt=torch.int32) if arcade_stats else None

        self._cur = z(B, dt=torch.int32)

    @property
    def actor_records(self):
        """[B, words] view of the per-actor records of a navigation or generated maze (words 3, 4: goals_total,
        apples_total), or None."""
        gen, nav = getattr(self, "gen", None), getattr(self, "nav", None)
        if getattr(self, "arcade", None) is not None:        # a device arcade's game records (words 10..12: the totals)
            return self.arcade.view(self.B, ARCADE_RECORD)
        if gen is not None:
            return gen.view(self.B, -1)
        return nav.view(self.B, -1) if nav is not None else None

    @property
    def record_words(self):
        """int32 words of one actor's record (0: the maze keeps none)."""
        if getattr(self, "arcade", None) is not None:
            return ARCADE_RECORD
        if getattr(self, "gen", None) is not None:
            return self.gen_words
        return getattr(self, "nav_words", NAV_RECORD) if getattr(self, "nav", None) is not None else 0

    def cur_idx(self, out=None, base_actor=0):
        """Frame index of every actor's current observation (slot count % H1).  `base_actor` = index of this (view's)
        first actor in the ring the indices are meant for: a view then yields indices into its parent ring."""
        out = self._cur if out is None else out
        _chk(out, "i32", self.B, "cur_idx out")
        _call("unreal_ring_cur_idx", self.B, self.H1, int(base_actor), ptr(self.count), ptr(out))
        return out


def ring_view(ring, b0, b1):
    """The actors [b0, b1) of a ring as a Ring of their own (no copy: frame indices are relative to the view)."""
    v = object.__new__(Ring)
    v.B, v.H, v.H1, v.objective_size = b1 - b0, ring.H, ring.H1, ring.objective_size
    v.frame_shape, v.frame_stride = ring.frame_shape, ring.frame_stride
    H1, fs = ring.H1, ring.frame_stride
    v.frames = ring.frames[b0 * H1 * fs:b1 * H1 * fs]
    for name in ("r_reward", "r_action", "r_terminal", "r_last_action", "r_last_reward"):
        setattr(v, name, getattr(ring, name)[b0 * H1:b1 * H1])
    v.r_pc = ring.r_pc[b0 * H1 * PC_CELLS:b1 * H1 * PC_CELLS]
    obj = ring.objective_size
    v.r_objective = ring.r_objective[b0 * H1 * obj:b1 * H1 * obj] if obj else None
    dep = getattr(ring, "r_depth", None)
    v.r_depth = dep[b0 * H1 * DEPTH_POSITIONS:b1 * H1 * DEPTH_POSITIONS] if dep is not None else None
    bon = getattr(ring, "r_bonus", None)
    v.r_bonus = bon[b0 * H1:b1 * H1] if bon is not None else None
    v.pos = ring.pos[2 * b0:2 * b1]
    for name in ("last_action", "last_reward", "count", "episode_reward", "score_out", "score_valid", "_cur"):
        setattr(v, name, getattr(ring, name)[b0:b1])
    v.goal = ring.goal[2 * b0:2 * b1] if ring.goal is not None else None
    for name in ("layout", "ep_steps", "episode", "heading"):
        t = getattr(ring, name)
        setattr(v, name, t[b0:b1] if t is not None else None)
    nav = getattr(ring, "nav", None)
    v.sense_n, v.nav_words = getattr(ring, "sense_n", 0), getattr(ring, "nav_words", NAV_RECORD)
    v.nav = nav[b0 * v.nav_words:b1 * v.nav_words] if nav is not None else None
    v.gen_n, gen = getattr(ring, "gen_n", 0), getattr(ring, "gen", None)
    v.gen_words = getattr(ring, "gen_words", gen_record_words(v.gen_n))
    v.gen = gen[b0 * v.gen_words:b1 * v.gen_words] if gen is not None else None
    arcade = getattr(ring, "arcade", None)
    v.arcade = arcade[b0 * ARCADE_RECORD:b1 * ARCADE_RECORD] if arcade is not None else None
    for name in ("done_return", "done_episodes"):
        t = getattr(ring, name, None)
        setattr(v, name, t[b0:b1] if t is not None else None)
    # the view's actors' final-observation slots; their indices are the parent's: final_base + (b0 + b)
    fin = getattr(ring, "final_obs", None)
    v.final_base = getattr(ring, "final_base", ring.B * H1)
    v.final_obs = fin[b0 * fs:b1 * fs] if fin is not None else None
    return v


ARCADE_BREAKOUT, ARCADE_CFG_WORDS, ARCADE_RECORD = 1, 24, 16   # UNREAL_ARCADE_BREAKOUT / _CFG_WORDS / _RECORD
ARCADE_DUEL = 3                              # UNREAL_ARCADE_DUEL (2 is no game: the kernels write nothing for it)
ARCADE_INVADERS = 5                          # UNREAL_ARCADE_INVADERS
ARCADE_CROSSING = 7                          # UNREAL_ARCADE_CROSSING
ARCADE_LANE_STREAM = 0x43524F53              # counter word 2 of a crossing reset's lane-phase draw (UNREAL_ARCADE_LANE_STREAM)
ARCADE_BOMB_STREAM = 0x494E5642              # counter word 2 of an invaders bomb draw (UNREAL_ARCADE_BOMB_STREAM)
ARCADE_SERVE_STREAM = 0x41524B53             # counter word 2 of a serve draw (UNREAL_ARCADE_SERVE_STREAM)
ARCADE_MIX_MAX = 16                          # config blocks of a game mixture at the most (UNREAL_ARCADE_MIX_MAX)
ARCADE_SELFPLAY = "selfplay"                 # third element of the arcade tuple that selects the _selfplay entries (§7v)
ARCADE_VERSUS = "versus"                     # ... the _versus entries (§7w); a fourth element holds the opponent's buffers
MAZE_TOP_DOWN, MAZE_FIRST_PERSON = 0, 1       # the `view` of a maze (UNREAL_MAZE_TOP_DOWN / UNREAL_MAZE_FIRST_PERSON)
MAZE_FIRST_PERSON_GENERATED = 2               # first person, a generated block (UNREAL_MAZE_FIRST_PERSON_GENERATED)
# goal-sense blocks: UNREAL_MAZE_FIRST_PERSON_SENSE / UNREAL_MAZE_FIRST_PERSON_GENERATED_SENSE
MAZE_FIRST_PERSON_SENSE, MAZE_FIRST_PERSON_GENERATED_SENSE = 3, 4
# forage blocks: UNREAL_MAZE_FIRST_PERSON_FORAGE / UNREAL_MAZE_FIRST_PERSON_GENERATED_FORAGE; their records
# are the navigation / generated records (words 4..7: the running totals of pickup kinds 0..3)
MAZE_FIRST_PERSON_FORAGE, MAZE_FIRST_PERSON_GENERATED_FORAGE = 5, 6
NAV_RECORD = 8                                # int32 words of a navigation maze's per-actor record (UNREAL_MAZE_NAV_RECORD)
MAZE_RECORD_HEADER, NAV_APPLE_RECORD = 18, 65  # words of a layout record before its free list; of an apple record
DEPTH_POSITIONS, DEPTH_CLASSES = 12, 8        # UNREAL_DEPTH_POSITIONS / UNREAL_DEPTH_CLASSES
DEPTH_EDGES = (1, 2, 3, 4, 6, 8, 12)          # class = number of edges e with t >= e


def style_words(N):
    """int32 words of one maze's 4-bit style ids (UNREAL_MAZE_STYLE_WORDS(N))."""
    return (N * N + 7) // 8


def dist_words(N):
    """int32 words of one actor's distance field, 16 bits per cell (UNREAL_MAZE_DIST_WORDS(N)); 0 for N = 0."""
    return (N * N + 1) // 2 if N else 0


def sense_record_words(N):
    """int32 words of a static goal-sense maze's per-actor record (UNREAL_MAZE_SENSE_RECORD(N))."""
    return NAV_RECORD + dist_words(N)


def gen_record_words(N, styled=False):
    """int32 words of a generated maze's per-actor record (UNREAL_MAZE_GEN_RECORD(N)): the navigation record, the layout
    record (18 + N * N) and the apple record (65); `styled`: of a styled block's (UNREAL_MAZE_GEN_STYLED_RECORD(N)), which
    ends in the style ids."""
    return NAV_RECORD + MAZE_RECORD_HEADER + N * N + NAV_APPLE_RECORD + (style_words(N) if styled else 0) if N else 0


def _maze_args(ring, maze):
    """The maze tail of every maze entry.  `maze` (every maze wrapper) = (view, N, int32 config block on the device, global
    index of the ring's actor 0[, True for a styled block]) of a configured maze, or None for the reference's map,
    top-down."""
    if maze is None:
        return (MAZE_TOP_DOWN, 7, None, 0, None, None, None, None, None)
    view, N, block, actor_base = maze[:4]
    styled = len(maze) > 4 and bool(maze[4])
    _chk(block, "i32", 8, "maze config")
    nav = getattr(ring, "nav", None)
    # a goal-sense block (views 3, 4) is a first-person / generated block whose records end in the distance field: the
    # record widths are the ring's (Ring(sense=N)), checked against the block's here
    sense = view in (MAZE_FIRST_PERSON_SENSE, MAZE_FIRST_PERSON_GENERATED_SENSE)
    generated = view in (MAZE_FIRST_PERSON_GENERATED, MAZE_FIRST_PERSON_GENERATED_SENSE, MAZE_FIRST_PERSON_GENERATED_FORAGE)
    static_fp = view in (MAZE_FIRST_PERSON, MAZE_FIRST_PERSON_SENSE, MAZE_FIRST_PERSON_FORAGE)
    if getattr(ring, "sense_n", 0) != (N if sense else 0):
        raise ValueError("a goal-sense maze needs a ring with distance fields of its size (Ring(sense=%d)), any other "
                         "maze a ring without" % N)
    arrays = (("goal", 2 * ring.B), ("layout", ring.B), ("ep_steps", ring.B), ("episode", ring.B))
    if generated:
        arrays = tuple(a for a in arrays if a[0] != "layout")
    if static_fp:
        if sense and nav is None:
            raise ValueError("a goal-sense maze keeps per-actor records (Ring(nav=True, sense=%d))" % N)
        if view == MAZE_FIRST_PERSON_FORAGE and nav is None:
            raise ValueError("a forage maze keeps per-actor records (Ring(nav=True))")
        arrays += (("nav", getattr(ring, "nav_words", NAV_RECORD) * ring.B),) if nav is not None else (("heading", ring.B),)
    if generated:
        want = gen_record_words(N, styled) + (dist_words(N) if sense else 0)
        if getattr(ring, "gen_n", 0) != N or getattr(ring, "gen_words", gen_record_words(N)) != want:
            raise ValueError("a generated maze needs a ring with per-actor records of its size (Ring(gen=%d, gen_styled=%s))"
                             % (N, styled))
        arrays += (("gen", ring.gen_words * ring.B),)
    for name, n in arrays:
        _chk(getattr(ring, name), "i32", n, "ring." + name)
    heading = nav if nav is not None and static_fp else ring.heading
    if generated:
        heading = ring.gen
    layout = None if generated else ring.layout      # (a generated block has no layout records)
    return (int(view), int(N), ptr(block), int(actor_base), ptr(ring.goal), ptr(layout), ptr(ring.ep_steps),
            ptr(ring.episode), ptr(heading))


def _ring_args(ring, out_reward, out_terminal):
    """pos .. score_valid of the step entries: the ring and the per-actor state they commit to."""
    return (ptr(ring.pos), ptr(ring.last_action), ptr(ring.last_reward), ptr(ring.count), ptr(ring.frames),
            ptr(ring.r_reward), ptr(ring.r_action), ptr(ring.r_terminal), ptr(ring.r_last_action), ptr(ring.r_last_reward),
            ptr(ring.r_pc), ptr(out_reward), ptr(out_terminal), ptr(ring.episode_reward), ptr(ring.score_out),
            ptr(ring.score_valid))


def maze_reset(ring, mask=None, maze=None):
    """Reset every actor (where mask != 0)."""
    _chk(mask, "i32", ring.B, "mask", optional=True)
    _call("unreal_maze_reset", ring.B, ring.H1, ptr(mask), ptr(ring.pos), ptr(ring.last_action), ptr(ring.last_reward),
          ptr(ring.count), ptr(ring.frames), *_maze_args(ring, maze))


def maze_step(ring, actions, active=None, out_reward=None, out_terminal=None, reset_on_terminal=True,
              track_score=False, maze=None):
    B = ring.B
    _chk(actions, "i32", B, "actions")
    _chk(active, "i32", B, "active", optional=True)
    _chk(out_reward, "f32", B, "out_reward", optional=True)
    _chk(out_terminal, "i32", B, "out_terminal", optional=True)
    _call("unreal_maze_step", B, ring.H1, ptr(actions), ptr(active), *_ring_args(ring, out_reward, out_terminal),
          int(reset_on_terminal), int(track_score), *_maze_args(ring, maze))


def _rollout_args(ring, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end, next_idx, next_lar, lar_ld,
                  lar_col0, A, base_actor):
    B = ring.B
    _chk(out_reward, "f32", B, "out_reward"); _chk(out_terminal, "i32", B, "out_terminal")
    for t in (active, active_log_t, n_steps, terminal_end):
        _chk(t, "i32", B)
    _chk(next_idx, "i32", B, "next_idx", optional=True)
    _chk(next_lar, "f32", (B - 1) * lar_ld + lar_col0 + A + 1 if next_lar is not None else None, "next_lar", optional=True)
    return _ring_args(ring, out_reward, out_terminal) + (
        ptr(active), ptr(active_log_t), ptr(n_steps), ptr(terminal_end), ptr(next_idx), ptr(next_lar), int(lar_ld),
        int(lar_col0), int(A), int(base_actor))


def _final_obs_args(ring, final_obs):
    """The trailing argument of the _tl entries: `final_obs` None -> () and the plain entry; else the [B] frames of the
    final-observation store (time-limit bootstrapping)."""
    if final_obs is None:
        return "", ()
    if ring.frame_stride != FRAME_BYTES:
        raise ValueError("the final-observation store holds 84 x 84 frames")
    _chk(final_obs, "u8", ring.B * FRAME_BYTES, "final_obs")
    if final_obs.data_ptr() % 16:
        raise ValueError("final_obs must be 16-byte aligned")
    return "_tl", (ptr(final_obs),)


def _maze_final_obs(maze, final_obs):
    if final_obs is not None and (maze is None or maze[0] not in (MAZE_FIRST_PERSON, MAZE_FIRST_PERSON_GENERATED,
                                                                  MAZE_FIRST_PERSON_FORAGE,
                                                                  MAZE_FIRST_PERSON_GENERATED_FORAGE)):
        raise ValueError("a final-observation store needs a first-person maze without goal_sense (top-down and goal-sense "
                         "mazes are out of scope of time-limit bootstrapping)")


def maze_rollout_step(ring, actions, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end,
                      next_idx=None, next_lar=None, lar_ld=0, lar_col0=0, A=0, base_actor=0, maze=None, final_obs=None):
    """maze_step + rollout_advance (+ cur_idx and lar_fill for the NEXT step's rows) in one launch.  `base_actor`: index
    of this (view's) first actor in the ring the next_idx values are meant for (see Ring.cur_idx).  `final_obs`: the
    unreal_maze_rollout_step_tl form, which keeps the final observation of a timed-out episode there and flags it 2."""
    _chk(actions, "i32", ring.B, "actions")
    _maze_final_obs(maze, final_obs)
    tl, fin = _final_obs_args(ring, final_obs)
    _call("unreal_maze_rollout_step" + tl, ring.B, ring.H1, ptr(actions),
          *_rollout_args(ring, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end, next_idx, next_lar,
                         lar_ld, lar_col0, A, base_actor), *_maze_args(ring, maze), *fin)


def maze_policy_rollout_step(ring, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions, out_reward, out_terminal, active,
                             active_log_t, n_steps, terminal_end, next_idx=None, next_lar=None, lar_ld=0, lar_col0=0, A=4,
                             base_actor=0, maze=None, final_obs=None):
    """policy_step + maze_rollout_step in one launch: the workgroup that steps an actor computes its pi / V / action first
    (bit-identical to the two launches).  A = 6: a first-person navigation maze with Lab's action set.  `final_obs`: the
    _tl form, as maze_rollout_step."""
    B = ring.B
    _maze_final_obs(maze, final_obs)
    tl, fin = _final_obs_args(ring, final_obs)
    nav = maze is not None and ((maze[0] in (MAZE_FIRST_PERSON, MAZE_FIRST_PERSON_SENSE, MAZE_FIRST_PERSON_FORAGE) and
                                 getattr(ring, "nav", None) is not None) or
                                maze[0] in (MAZE_FIRST_PERSON_GENERATED, MAZE_FIRST_PERSON_GENERATED_SENSE,
                                            MAZE_FIRST_PERSON_GENERATED_FORAGE))
    if A != 4 and not (A == 6 and nav):
        raise ValueError("the maze has 4 actions (6: a first-person navigation maze with action_set='lab'); A = %r" % (A,))
    _chk(X, "f32", (B - 1) * ldx + 256, "X"); _chk(Wp, "f32", 256 * A); _chk(bp, "f32", A); _chk(Wv, "f32", 256)
    _chk(bv, "f32", 1); _chk(u, "f64", B, "u"); _chk(pi_out, "f32", B * A); _chk(v_out, "f32", B)
    _chk(actions, "i32", B, "actions")
    _call("unreal_maze_policy_rollout_step" + tl, B, ring.H1, ptr(X), int(ldx), ptr(Wp), ptr(bp), ptr(Wv), ptr(bv), ptr(u),
          ptr(pi_out), ptr(v_out), ptr(actions),
          *_rollout_args(ring, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end, next_idx, next_lar,
                         lar_ld, lar_col0, A, base_actor), *_maze_args(ring, maze), *fin)


def maze_wall_templates(maze, n_layouts, device, out=None):
    """The wall image of every layout of a top-down maze (`maze` as in the maze wrappers; None: the reference's map, one
    layout) -> uint8 [n_layouts * FRAME_BYTES], what maze_policy_rollout_step_encode patches the agent and goal blocks
    into.  Layouts do not change once a block is bound: call once per block."""
    n_layouts = int(n_layouts)
    if maze is not None and maze[0] != MAZE_TOP_DOWN:
        raise ValueError("wall templates are the top-down view's")
    if maze is None and n_layouts != 1:
        raise ValueError("the reference's map is one layout")
    if out is None:
        out = torch.empty(n_layouts * FRAME_BYTES, dtype=torch.uint8, device=device)
    _chk(out, "u8", n_layouts * FRAME_BYTES, "templates")
    N, block = (7, None) if maze is None else (maze[1], maze[2])
    _chk(block, "i32", 8, "maze config", optional=True)
    _call("unreal_maze_wall_templates", int(N), ptr(block), n_layouts, ptr(out))
    return out


def maze_policy_rollout_step_encode(ring, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions, out_reward, out_terminal,
                                    active, active_log_t, n_steps, terminal_end, templates, scale, W1, b1, W2, b2, f2_out,
                                    c1_out, relu_bits, prepared, f2_max=None, c1_max=None, next_idx=None, next_lar=None,
                                    lar_ld=0, lar_col0=0, A=4, base_actor=0, maze=None):
    """maze_policy_rollout_step + encoder_fwd(ring.frames, next_idx, ...) in one launch, bit for bit: row b of f2_out /
    c1_out / relu_bits is the encoding of actor b's next observation.  Top-down mazes with 4 actions only; `templates` from
    maze_wall_templates, `prepared` from encoder_prepare(W1, b1, W2, scale)."""
    B = ring.B
    if (maze is not None and maze[0] != MAZE_TOP_DOWN) or A != 4:
        raise ValueError("the fused step + encoder serves top-down mazes with 4 actions")
    if ring.frame_stride != FRAME_BYTES:
        raise ValueError("the fused step + encoder serves 84 x 84 frames")
    _chk(X, "f32", (B - 1) * ldx + 256, "X"); _chk(Wp, "f32", 256 * A); _chk(bp, "f32", A); _chk(Wv, "f32", 256)
    _chk(bv, "f32", 1); _chk(u, "f64", B, "u"); _chk(pi_out, "f32", B * A); _chk(v_out, "f32", B)
    _chk(actions, "i32", B, "actions")
    _chk(templates, "u8", FRAME_BYTES, "templates")
    if templates.numel() % FRAME_BYTES:
        raise ValueError("templates: whole frames")
    _chk(W1, "f32", 3072); _chk(b1, "f32", 16); _chk(W2, "f32", 8192); _chk(b2, "f32", 32)
    _chk(f2_out, "f32", B * F2_DIM); _chk(c1_out, "f32", B * C1_DIM); _chk(relu_bits, "i16", B * RELU_WORDS, "relu_bits")
    _chk(f2_max, "f32", 1, "f2_max", optional=True); _chk(c1_max, "f32", 1, "c1_max", optional=True)
    _chk(prepared, "u8", ENC_PREPARED_BYTES, "prepared")
    _call("unreal_maze_policy_rollout_step_encode", B, ring.H1, ptr(X), int(ldx), ptr(Wp), ptr(bp), ptr(Wv), ptr(bv),
          ptr(u), ptr(pi_out), ptr(v_out), ptr(actions),
          *_rollout_args(ring, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end, next_idx, next_lar,
                         lar_ld, lar_col0, A, base_actor), *_maze_args(ring, maze),
          ptr(templates), templates.numel() // FRAME_BYTES, float(scale), ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(c1_out),
          ptr(f2_out), ptr(relu_bits), ptr(f2_max), ptr(c1_max), ptr(prepared))


# ---- device arcade (csrc/arcade.hip) -----------------------------------------------------------------------
def _arcade_args(ring, arcade, stats=True):
    """-> ("", "_mix", "_selfplay" or "_versus", the tail of the arcade entry of that name, the arguments behind its `records` and
    final_obs).
    `arcade` = (int32 config block on the device, global index of the ring's actor 0), which selects the plain entries, or
    (K consecutive blocks, that index, K), a game mixture, which selects the _mix entries: global actor g
    plays block g % K, and the step forms (`stats`) also take the ring's done_return / done_episodes (None without
    Ring(arcade_stats=True)); or (the duel's block, that index, ARCADE_SELFPLAY), self-play, which selects
    the _selfplay entries: global actors 2 i and 2 i + 1 are the two seats of game i (the entries refuse an odd actor count
    or index); or (the duel's block, that index, ARCADE_VERSUS, opponent), one learner per game, which
    selects the _versus entries: `opponent` holds actions, last_action (int32 [B]), last_reward (float32 [B]) and frames
    (uint8 [B * FRAME_BYTES]), whose pointers follow every other argument, in reset too."""
    K = None
    selfplay = len(arcade) == 3 and isinstance(arcade[2], str)
    if len(arcade) == 4:
        block, actor_base, tag, opp = arcade
        if tag != ARCADE_VERSUS:
            raise ValueError("arcade tuple: unknown entry family %r" % (tag,))
        _chk(block, "i32", ARCADE_CFG_WORDS, "arcade config")
        _chk(opp.actions, "i32", ring.B, "opponent.actions")
        _chk(opp.frames, "u8", ring.B * FRAME_BYTES, "opponent.frames")
        _chk(opp.last_action, "i32", ring.B, "opponent.last_action")
        _chk(opp.last_reward, "f32", ring.B, "opponent.last_reward")
        if opp.frames.data_ptr() % 16:
            raise ValueError("opponent.frames must be 16-byte aligned")
        versus = (ptr(opp.actions), ptr(opp.frames), ptr(opp.last_action), ptr(opp.last_reward))
    elif selfplay:
        block, actor_base, tag = arcade
        if tag != ARCADE_SELFPLAY:
            raise ValueError("arcade tuple: unknown entry family %r" % (tag,))
    elif len(arcade) == 3:
        block, actor_base, K = arcade
        K = int(K)
        if not 1 <= K <= ARCADE_MIX_MAX:
            raise ValueError("a game mixture holds 1..%d config blocks, not %d" % (ARCADE_MIX_MAX, K))
    else:
        block, actor_base = arcade
    _chk(block, "i32", ARCADE_CFG_WORDS * (K or 1), "arcade config")
    if getattr(ring, "arcade", None) is None:
        raise ValueError("an arcade environment needs a ring with game records (Ring(arcade=True))")
    for name, n in (("ep_steps", ring.B), ("episode", ring.B), ("arcade", ARCADE_RECORD * ring.B)):
        _chk(getattr(ring, name), "i32", n, "ring." + name)
    if actor_base < 0:
        raise ValueError("actor_base %d < 0" % actor_base)
    tail = (int(actor_base), ptr(ring.ep_steps), ptr(ring.episode), ptr(ring.arcade))
    if len(arcade) == 4:
        return "_versus", (ptr(block),) + tail, versus
    if K is None:
        return "_selfplay" if selfplay else "", (ptr(block),) + tail, ()
    done_return, done_episodes = getattr(ring, "done_return", None), getattr(ring, "done_episodes", None)
    if (done_return is None) != (done_episodes is None):
        raise ValueError("ring.done_return and ring.done_episodes go together")
    _chk(done_return, "f32", ring.B, "ring.done_return", optional=True)
    _chk(done_episodes, "i32", ring.B, "ring.done_episodes", optional=True)
    return "_mix", (ptr(block), K) + tail, ((ptr(done_return), ptr(done_episodes)) if stats else ())


def arcade_reset(ring, mask=None, arcade=None):
    """Start a new episode of every actor (where mask != 0)."""
    _chk(mask, "i32", ring.B, "mask", optional=True)
    mix, tail, opp = _arcade_args(ring, arcade, stats=False)       # (what follows the tail: the _versus entries' alone)
    _call("unreal_arcade%s_reset" % mix, ring.B, ring.H1, ptr(mask), ptr(ring.pos), ptr(ring.last_action),
          ptr(ring.last_reward), ptr(ring.count), ptr(ring.frames), *tail, *opp)


def arcade_step(ring, actions, active=None, out_reward=None, out_terminal=None, reset_on_terminal=True,
                track_score=False, arcade=None):
    B = ring.B
    _chk(actions, "i32", B, "actions")
    _chk(active, "i32", B, "active", optional=True)
    _chk(out_reward, "f32", B, "out_reward", optional=True)
    _chk(out_terminal, "i32", B, "out_terminal", optional=True)
    mix, tail, done = _arcade_args(ring, arcade)
    _call("unreal_arcade%s_step" % mix, B, ring.H1, ptr(actions), ptr(active), *_ring_args(ring, out_reward, out_terminal),
          int(reset_on_terminal), int(track_score), *tail, *done)


def _arcade_actions(A):
    if A != 4:
        raise ValueError("the arcade has 4 actions; A = %r" % (A,))


def arcade_rollout_step(ring, actions, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end,
                        next_idx=None, next_lar=None, lar_ld=0, lar_col0=0, A=4, base_actor=0, arcade=None,
                        final_obs=None):
    """arcade_step + rollout_advance (+ cur_idx and lar_fill for the NEXT step's rows) in one launch, as
    maze_rollout_step (`final_obs`: the _tl form)."""
    _arcade_actions(A)
    _chk(actions, "i32", ring.B, "actions")
    tl, fin = _final_obs_args(ring, final_obs)
    mix, tail, done = _arcade_args(ring, arcade)
    _call("unreal_arcade%s_rollout_step%s" % (mix, tl), ring.B, ring.H1, ptr(actions),
          *_rollout_args(ring, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end, next_idx, next_lar,
                         lar_ld, lar_col0, A, base_actor), *tail, *fin, *done)


def arcade_policy_rollout_step(ring, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, actions, out_reward, out_terminal, active,
                               active_log_t, n_steps, terminal_end, next_idx=None, next_lar=None, lar_ld=0, lar_col0=0,
                               A=4, base_actor=0, arcade=None, final_obs=None):
    """policy_step + arcade_rollout_step in one launch (bit-identical to the two launches; `final_obs`: the _tl form)."""
    B = ring.B
    _arcade_actions(A)
    tl, fin = _final_obs_args(ring, final_obs)
    _chk(X, "f32", (B - 1) * ldx + 256, "X"); _chk(Wp, "f32", 256 * A); _chk(bp, "f32", A); _chk(Wv, "f32", 256)
    _chk(bv, "f32", 1); _chk(u, "f64", B, "u"); _chk(pi_out, "f32", B * A); _chk(v_out, "f32", B)
    _chk(actions, "i32", B, "actions")
    mix, tail, done = _arcade_args(ring, arcade)
    _call("unreal_arcade%s_policy_rollout_step%s" % (mix, tl), B, ring.H1, ptr(X), int(ldx), ptr(Wp), ptr(bp), ptr(Wv),
          ptr(bv), ptr(u), ptr(pi_out), ptr(v_out), ptr(actions),
          *_rollout_args(ring, out_reward, out_terminal, active, active_log_t, n_steps, terminal_end, next_idx, next_lar,
                         lar_ld, lar_col0, A, base_actor), *tail, *fin, *done)


def maze_objective(ring, next_lar=None, lar_ld=0, lar_col0=0):
    """The objective vectors of a goal-sense maze: {gf / 32, gs / 32, d / 512} of every actor's record ->
    the current slot of ring.r_objective and, with `next_lar`, columns [lar_col0, lar_col0 + 3) of its rows (stride
    lar_ld): the objective columns of the next step's LSTM input."""
    rec, words = ring.actor_records, ring.record_words
    if rec is None or not getattr(ring, "sense_n", 0) or ring.objective_size != 3:
        raise ValueError("maze_objective needs the ring of a goal-sense maze (Ring(objective_size=3, sense=N))")
    B = ring.B
    _chk(rec, "i32", B * words, "ring records"); _chk(ring.r_objective, "f32", B * ring.H1 * 3, "ring.r_objective")
    _chk(ring.count, "i32", B, "ring.count")
    if next_lar is not None:
        if lar_col0 < 0 or lar_ld < lar_col0 + 3:
            raise ValueError("next_lar: lar_ld %d < lar_col0 %d + 3" % (lar_ld, lar_col0))
        _chk(next_lar, "f32", (B - 1) * lar_ld + lar_col0 + 3, "next_lar")
    _call("unreal_maze_objective", B, ring.H1, ptr(ring.count), ptr(rec), int(words), ptr(ring.r_objective),
          ptr(next_lar), int(lar_ld), int(lar_col0))


def check_depth_maze(maze):
    """Depth labels exist for first-person device mazes only: raises ValueError for the reference's map and
    every top-down maze.  `maze` as in _maze_args."""
    if maze is None or maze[0] == MAZE_TOP_DOWN:
        raise ValueError("depth labels need a first-person device maze (MazeConfig(view='first_person')); top-down mazes, "
                         "the arcade and host-fed environments are out of scope")


def maze_depth_labels(ring, maze):
    """The depth classes of every actor's current view -> the current slot of ring.r_depth, 12 bytes per
    slot.  `maze` as in _maze_args; every first-person view is served."""
    check_depth_maze(maze)
    if getattr(ring, "r_depth", None) is None:
        raise ValueError("maze_depth_labels needs a ring with depth labels (Ring(depth=True))")
    B = ring.B
    view, N, cfg, _, _, layout, _, _, heading = _maze_args(ring, maze)
    _chk(ring.r_depth, "u8", B * ring.H1 * DEPTH_POSITIONS, "ring.r_depth")
    _chk(ring.count, "i32", B, "ring.count"); _chk(ring.pos, "i32", 2 * B, "ring.pos")
    _call("unreal_maze_depth_labels", B, ring.H1, N, ptr(ring.count), ptr(ring.pos), heading, int(ring.record_words), cfg,
          layout, ptr(ring.r_depth))


def depth_loss_grad(rows, logits, ld, r_depth, frame_idx, active, scale, dlogits, loss, hits):
    """Softmax cross-entropy of 12 groups of 8 logits against the ring's depth labels: the label of row r,
    position j is r_depth[frame_idx[r] * 12 + j].  loss += scale * sum over active rows; dlogits [rows, 96] = scale *
    (p - onehot) on active rows, 0 elsewhere (None: forward only); hits (int32 [2]) += (arg max == label, counted)."""
    n = DEPTH_POSITIONS * DEPTH_CLASSES
    if rows <= 0 or ld < n:
        raise ValueError("depth_loss_grad: rows=%d ld=%d" % (rows, ld))
    _chk(logits, "f32", (rows - 1) * ld + n, "logits"); _chk(r_depth, "u8", DEPTH_POSITIONS, "r_depth")
    _chk(frame_idx, "i32", rows, "frame_idx"); _chk(active, "i32", rows, "active")
    _chk(dlogits, "f32", rows * n, "dlogits", optional=True); _chk(loss, "f32", 1, "loss"); _chk(hits, "i32", 2, "hits")
    _call("unreal_depth_loss_grad", rows, ptr(logits), int(ld), ptr(r_depth), ptr(frame_idx), ptr(active), float(scale),
          ptr(dlogits), ptr(loss), ptr(hits))


def pixel_change_u8(frames, idx_new, idx_old, denom, out):
    N = idx_new.numel()
    _chk(frames, "u8"); _chk(idx_new, "i32", N); _chk(idx_old, "i32", N); _chk(out, "f32", N * PC_CELLS)
    _call("unreal_pixel_change_u8", N, ptr(frames), ptr(idx_new), ptr(idx_old), float(denom), ptr(out))


def _philox_shape(n, row_len, row_stride, col0):
    row_len = n if row_len is None else int(row_len)
    row_stride = row_len if row_stride is None else int(row_stride)
    if row_len <= 0 or n % row_len or col0 < 0 or col0 + row_len > row_stride:
        raise ValueError("philox: n=%d row_len=%d row_stride=%d col0=%d" % (n, row_len, row_stride, col0))
    return row_len, row_stride, int(col0)


def philox_uniform(seed, stream_id, out, row_len=None, row_stride=None, col0=0):
    """out[i] = draw (i // row_len) * row_stride + col0 + i % row_len of stream (seed, stream_id)."""
    _chk(out, "f64")
    rl, rs, c0 = _philox_shape(out.numel(), row_len, row_stride, col0)
    _call("unreal_philox_uniform", int(seed), int(stream_id), out.numel(), rl, rs, c0, ptr(out))


def philox_randint(seed, stream_id, high, out, row_len=None, row_stride=None, col0=0):
    _chk(out, "i32")
    rl, rs, c0 = _philox_shape(out.numel(), row_len, row_stride, col0)
    _call("unreal_philox_randint", int(seed), int(stream_id), out.numel(), rl, rs, c0, int(high), ptr(out))


# ---- replay --------------------------------------------------------------------------------------
def replay_sample_seq(ring, L, start_draw, seq_idx, seq_len):
    B = ring.B
    _chk(start_draw, "i32", B); _chk(seq_idx, "i32", L * B); _chk(seq_len, "i32", B)
    _call("unreal_replay_sample_seq", B, ring.H, ring.H1, L, ptr(start_draw), ptr(ring.count),
          ptr(ring.r_terminal), ptr(seq_idx), ptr(seq_len))


def replay_sample_rp(ring, coin, u, rp_idx, rp_class, mode=0):
    B = ring.B
    _chk(coin, "i32", B); _chk(u, "f64", B); _chk(rp_idx, "i32", 3 * B); _chk(rp_class, "i32", B)
    _call("unreal_replay_sample_rp", B, ring.H, ring.H1, ptr(coin), ptr(u), ptr(ring.count),
          ptr(ring.r_reward), ptr(rp_idx), ptr(rp_class), int(mode))


HOSTFED_CLIP_REWARD, HOSTFED_TERMINAL_OBS = 1, 2   # unreal_hostfed_step flags (UNREAL_HOSTFED_*)


def hostfed_step(ring, staged, actions, rewards, terminals, active=None, out_reward=None, out_terminal=None,
                 reset_on_terminal=True, track_score=False, clip_reward=True, pc_denom=48.0 * 255.0, reset_staged=None,
                 terminal_obs=False):
    """One step of host-fed actors (include/unreal_hip.h: Lab, indoor and gym): `staged` holds one frame per actor,
    ring.frame_stride bytes apart.  The pixel change goes to ring.r_pc at 84 x 84 only.  terminal_obs: gym's terminal rule,
    with `reset_staged` the post-reset observations the next slot gets where terminal (required with reset_on_terminal)."""
    B = ring.B
    frame_dims(*ring.frame_shape)
    pc = ring.frame_shape == FRAME_SHAPE
    _chk(staged, "u8", B * ring.frame_stride, "staged")
    _chk(reset_staged, "u8", B * ring.frame_stride, "reset_staged", optional=not (terminal_obs and reset_on_terminal))
    _chk(actions, "i32", B, "actions"); _chk(rewards, "f32", B, "rewards"); _chk(terminals, "i32", B, "terminals")
    _chk(active, "i32", B, "active", optional=True)
    _chk(out_reward, "f32", B, "out_reward", optional=True); _chk(out_terminal, "i32", B, "out_terminal", optional=True)
    flags = (HOSTFED_CLIP_REWARD if clip_reward else 0) | (HOSTFED_TERMINAL_OBS if terminal_obs else 0)
    _call("unreal_hostfed_step", B, ring.H1, ring.frame_stride, ptr(staged), ptr(reset_staged), ptr(actions),
          ptr(rewards), ptr(terminals), ptr(active), ptr(ring.last_action), ptr(ring.last_reward), ptr(ring.count),
          ptr(ring.frames), ptr(ring.r_reward), ptr(ring.r_action), ptr(ring.r_terminal), ptr(ring.r_last_action),
          ptr(ring.r_last_reward), ptr(ring.r_pc) if pc else None, ptr(out_reward), ptr(out_terminal),
          ptr(ring.episode_reward), ptr(ring.score_out), ptr(ring.score_valid), int(reset_on_terminal), int(track_score),
          flags, float(pc_denom))


def hostfed_reset(ring, staged, mask=None):
    frame_dims(*ring.frame_shape)
    _chk(staged, "u8", ring.B * ring.frame_stride, "staged"); _chk(mask, "i32", ring.B, "mask", optional=True)
    _call("unreal_hostfed_reset", ring.B, ring.H1, ring.frame_stride, ptr(mask), ptr(staged), ptr(ring.last_action),
          ptr(ring.last_reward), ptr(ring.count), ptr(ring.frames))


def frame_resize(n, Hs, Ws, src, dst, mask=None):
    """dst [n,84,84,3] uint8 <- src [n,Hs,Ws,3] uint8 raw frames, bilinear with cv2 INTER_LINEAR's half-pixel rule in fp32,
    rounded to nearest-even (gym_environment.py:18-23); rows with mask == 0 are left as they are."""
    if n <= 0 or Hs < 1 or Ws < 1:
        raise ValueError("frame_resize: n=%d Hs=%d Ws=%d" % (n, Hs, Ws))
    _chk(src, "u8", n * Hs * Ws * 3, "src"); _chk(dst, "u8", n * FRAME_BYTES, "dst"); _chk(mask, "i32", n, optional=True)
    _call("unreal_frame_resize", n, Hs, Ws, ptr(src), ptr(mask), ptr(dst))


def base_returns(B, T, rewards, values, n_steps, boot_v, terminal_end, gamma, R_out, adv_out):
    for t in (rewards, values, R_out, adv_out):
        _chk(t, "f32", B * T)
    _chk(n_steps, "i32", B); _chk(boot_v, "f32", B); _chk(terminal_end, "i32", B)
    _call("unreal_base_returns", B, T, ptr(rewards), ptr(values), ptr(n_steps), ptr(boot_v),
          ptr(terminal_end), float(gamma), ptr(R_out), ptr(adv_out))


def base_returns_tl(B, T, rewards, values, n_steps, boot_v, terminal_end, gamma, lam, R_out, adv_out):
    """GAE(lam) returns and advantages; terminal_end 1: no bootstrap, 0 / 2: from boot_v.  lam = 1: n-step."""
    if not 0.0 <= float(lam) <= 1.0:
        raise ValueError("lambda = %r outside [0, 1]" % (lam,))
    for t in (rewards, values, R_out, adv_out):
        _chk(t, "f32", B * T)
    _chk(n_steps, "i32", B); _chk(boot_v, "f32", B); _chk(terminal_end, "i32", B)
    _call("unreal_base_returns_tl", B, T, ptr(rewards), ptr(values), ptr(n_steps), ptr(boot_v),
          ptr(terminal_end), float(gamma), float(lam), ptr(R_out), ptr(adv_out))


def boot_gather(ring, T, A, terminal_end, n_steps, actions, rewards, frame_idx, base_actor=0, carried_c=None,
                carried_h=None, ws_c=None, ws_h=None, c0=None, h0=None, xcat=None, ld=0, col0=256):
    """The bootstrap pass's inputs with time-limit bootstrapping.  `ring`: the B actors of the pass (a view:
    its first actor is `base_actor` of the ring the frame indices are meant for, whose final-observation slots start at
    ring.final_base).  Actors with terminal_end 2 get their final-observation slot, rows (n_steps - 1) B + b of ws_c / ws_h
    and of actions / rewards; the others their current slot, carried_c / carried_h and the ring's last action / reward.
    c0 None: no state (feed-forward); xcat None: no [one-hot last action | last reward] columns."""
    B = ring.B
    if T <= 0:
        raise ValueError("T = %r" % (T,))
    if getattr(ring, "final_obs", None) is None:
        raise ValueError("boot_gather needs a ring with a final-observation store (Ring(final_obs=True))")
    _chk(terminal_end, "i32", B, "terminal_end"); _chk(n_steps, "i32", B, "n_steps"); _chk(frame_idx, "i32", B, "frame_idx")
    _chk(actions, "i32", T * B, "actions"); _chk(rewards, "f32", T * B, "rewards")
    if c0 is not None:
        for t, n, name in ((carried_c, B, "carried_c"), (carried_h, B, "carried_h"), (ws_c, T * B, "ws_c"),
                           (ws_h, T * B, "ws_h"), (c0, B, "c0"), (h0, B, "h0")):
            _chk(t, "f32", n * 256, name)
    if xcat is not None:
        if not 0 < A < 256 or col0 < 0 or ld < col0 + A + 1:
            raise ValueError("xcat: A %d, ld %d, col0 %d" % (A, ld, col0))
        _chk(xcat, "f32", (B - 1) * ld + col0 + A + 1, "xcat")
    _call("unreal_boot_gather", B, int(T), ring.H1, int(base_actor), int(ring.final_base), int(A), ptr(ring.count),
          ptr(terminal_end), ptr(n_steps), ptr(ring.last_action), ptr(ring.last_reward), ptr(actions), ptr(rewards),
          ptr(carried_c), ptr(carried_h), ptr(ws_c), ptr(ws_h), ptr(frame_idx), ptr(c0), ptr(h0), ptr(xcat), int(ld),
          int(col0))


def vr_returns(ring, L, seq_idx, seq_len, boot_v, gamma, R_out, bonus=False):
    """`bonus`: a ring with r_bonus pays a replayed step r_reward + r_bonus; without one, or by default, r_reward."""
    B = ring.B
    _chk(seq_idx, "i32", L * B); _chk(seq_len, "i32", B); _chk(boot_v, "f32", B); _chk(R_out, "f32", (L - 1) * B)
    r_bonus = getattr(ring, "r_bonus", None) if bonus else None
    if r_bonus is not None:
        _chk(r_bonus, "f32", ring.r_reward.numel(), "r_bonus")
        _call("unreal_vr_returns_bonus", B, L, ptr(seq_idx), ptr(seq_len), ptr(ring.r_reward), ptr(r_bonus),
              ptr(ring.r_terminal), ptr(boot_v), float(gamma), ptr(R_out))
        return
    _call("unreal_vr_returns", B, L, ptr(seq_idx), ptr(seq_len), ptr(ring.r_reward), ptr(ring.r_terminal),
          ptr(boot_v), float(gamma), ptr(R_out))


# ---- exploration bonus (csrc/explore.hip) ------------------------------------------------------------------
EXPLORE_STREAM = 0x4558504C                   # counter word 2 of the multiplier draws ("EXPL")
EXPLORE_MAX_FEATURES = 1323                   # 21 x 21 x 3: an 84 x 84 frame at cell 4


def explore_features(H, W, cell, levels=8, vmax=255, bits=22):
    """F = (H / cell) (W / cell) 3 of the frame code; ValueError for parameters outside the kernels' ranges."""
    H, W, cell, levels, vmax, bits = int(H), int(W), int(cell), int(levels), int(vmax), int(bits)
    if H <= 0 or W <= 0 or cell < 2 or H % cell or W % cell:
        raise ValueError("explore: cell = %d must be >= 2 and divide the %d x %d frame" % (cell, H, W))
    F = (H // cell) * (W // cell) * 3
    if F > EXPLORE_MAX_FEATURES:
        raise ValueError("explore: %d features at cell %d, at most %d" % (F, cell, EXPLORE_MAX_FEATURES))
    if not (2 <= levels <= 64 and 1 <= vmax <= 255 and 10 <= bits <= 26):
        raise ValueError("explore: levels = %d (2..64), vmax = %d (1..255), bits = %d (10..26)" % (levels, vmax, bits))
    return F


def explore_multipliers(F, seed, mult):
    """mult[f] = word 0 of Philox4x32-10(seed, f, EXPLORE_STREAM) | 1 (uint32 kept in an int32 tensor)."""
    F = int(F)
    if not 0 < F <= EXPLORE_MAX_FEATURES:
        raise ValueError("explore_multipliers: F = %d" % F)
    _chk(mult, "i32", F, "mult")
    _call("unreal_explore_multipliers", F, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(mult))


def frame_codes(rows, frames, frame_stride, n_frames, H, W, idx, cell, levels, vmax, bits, mult, codes, gate=None):
    """codes[r] = the code of frame idx[r] of the pool (-1: idx outside [0, n_frames), or gated out).  `gate` = (B,
    active_log [rows], n_steps [B], terminal_end [B]): row t B + b is hashed iff active_log is set and the step does not
    end an episode.  A row that is not hashed reads no frame."""
    rows, n_frames, frame_stride = int(rows), int(n_frames), int(frame_stride)
    F = explore_features(H, W, cell, levels, vmax, bits)
    if rows <= 0 or n_frames <= 0 or frame_stride < int(H) * int(W) * 3 or frame_stride % 16:
        raise ValueError("frame_codes: rows=%d n_frames=%d frame_stride=%d" % (rows, n_frames, frame_stride))
    _chk(frames, "u8", n_frames * frame_stride, "frames"); _chk(idx, "i32", rows, "idx")
    _chk(mult, "i32", F, "mult"); _chk(codes, "i32", rows, "codes")
    B, act, ns, te = 0, None, None, None
    if gate is not None:
        B, act, ns, te = gate
        B = int(B)
        if B <= 0:
            raise ValueError("frame_codes: gate B = %d" % B)
        _chk(act, "i32", rows, "active_log"); _chk(ns, "i32", B, "n_steps"); _chk(te, "i32", B, "terminal_end")
    _call("unreal_frame_codes", rows, ptr(frames), frame_stride, n_frames, int(H), int(W), ptr(idx), B, ptr(act), ptr(ns),
          ptr(te), int(cell), int(levels), int(vmax), int(bits), ptr(mult), ptr(codes))


def count_add(rows, codes, table, bits):
    """table[code] += 1 for every code in [0, 2^bits) of codes[:rows] (int32 atomics)."""
    rows, bits = int(rows), int(bits)
    if rows <= 0 or not 10 <= bits <= 26:
        raise ValueError("count_add: rows=%d bits=%d" % (rows, bits))
    _chk(codes, "i32", rows, "codes"); _chk(table, "i32", 1 << bits, "table")
    _call("unreal_count_add", rows, ptr(codes), ptr(table), bits)


def count_bonus(rows, codes, table, bits, beta, rewards, active_log, frame_idx, bonus, rewards_total, r_bonus, stats_i,
                stats_f):
    """bonus = beta / sqrt(table[code]) of every counted row (0 elsewhere), rewards_total = rewards + bonus, r_bonus (None:
    no scatter) [frame_idx[r]] = bonus[r] on rows with active_log set; stats_i[2] += (rows with a bonus, those counted
    once), stats_f[1] += sum of bonus."""
    rows, bits, beta = int(rows), int(bits), float(beta)
    if rows <= 0 or not 10 <= bits <= 26 or not 0.0 <= beta < float("inf"):
        raise ValueError("count_bonus: rows=%d bits=%d beta=%r" % (rows, bits, beta))
    _chk(codes, "i32", rows, "codes"); _chk(table, "i32", 1 << bits, "table"); _chk(rewards, "f32", rows, "rewards")
    _chk(bonus, "f32", rows, "bonus"); _chk(rewards_total, "f32", rows, "rewards_total")
    _chk(stats_i, "i32", 2, "stats_i"); _chk(stats_f, "f32", 1, "stats_f")
    _chk(r_bonus, "f32", 1, "r_bonus", optional=True)
    if r_bonus is not None:
        _chk(active_log, "i32", rows, "active_log"); _chk(frame_idx, "i32", rows, "frame_idx")
    _call("unreal_count_bonus", rows, ptr(codes), ptr(table), bits, beta, ptr(rewards), ptr(active_log), ptr(frame_idx),
          0 if r_bonus is None else r_bonus.numel(), ptr(bonus), ptr(rewards_total), ptr(r_bonus), ptr(stats_i),
          ptr(stats_f))


def pc_returns(ring, L, seq_idx, seq_len, boot_qmax, gamma_pc, R_out):
    B = ring.B
    _chk(seq_idx, "i32", L * B); _chk(seq_len, "i32", B); _chk(boot_qmax, "f32", B * PC_CELLS)
    _chk(R_out, "f32", (L - 1) * B * PC_CELLS)
    _call("unreal_pc_returns", B, L, ptr(seq_idx), ptr(seq_len), ptr(ring.r_pc), ptr(ring.r_terminal),
          ptr(boot_qmax), float(gamma_pc), ptr(R_out))


def lar_fill(rows, A, last_action, last_reward, idx, xcat, ld, col0=256, clip=False):
    _chk(last_action, "i32"); _chk(last_reward, "f32"); _chk(idx, "i32", rows, optional=True)
    _chk(xcat, "f32", rows * ld)
    if idx is None and (last_action.numel() < rows or last_reward.numel() < rows):
        raise ValueError("lar_fill: per-row sources too short")
    _call("unreal_lar_fill", rows, A, ptr(last_action), ptr(last_reward), ptr(idx), ptr(xcat), ld, col0, int(clip))


def objective_put(ring, staged, active=None):
    """staged [B][obj] -> the current slot of every (active) actor."""
    obj = ring.objective_size
    if not obj:
        raise ValueError("this ring stores no objective vectors")
    _chk(staged, "f32", ring.B * obj, "staged objective"); _chk(active, "i32", ring.B, "active", optional=True)
    _call("unreal_objective_put", ring.B, ring.H1, obj, ptr(ring.count), ptr(active), ptr(staged), ptr(ring.r_objective))


def objective_fill(ring, rows, idx, xcat, ld, col0, slot_offset=0):
    obj = ring.objective_size
    if not obj:
        raise ValueError("this ring stores no objective vectors")
    _chk(idx, "i32", rows, "idx"); _chk(xcat, "f32", (rows - 1) * ld + col0 + obj, "xcat")
    _call("unreal_objective_fill", rows, obj, ring.H1, ptr(ring.r_objective), ptr(idx), slot_offset, ptr(xcat), ld, col0)


def gather_i32(src, idx, out):
    _chk(src, "i32"); _chk(idx, "i32"); _chk(out, "i32", idx.numel())
    _call("unreal_gather_i32", idx.numel(), ptr(src), ptr(idx), ptr(out))


def rollout_advance(B, terminal_t, active, active_log_t, n_steps, terminal_end):
    for t in (terminal_t, active, active_log_t, n_steps, terminal_end):
        _chk(t, "i32", B)
    _call("unreal_rollout_advance", B, ptr(terminal_t), ptr(active), ptr(active_log_t), ptr(n_steps),
          ptr(terminal_end))


def seq_mask(B, T, seq_len, mask):
    _chk(seq_len, "i32", B); _chk(mask, "i32", B * T)
    _call("unreal_seq_mask", B, T, ptr(seq_len), ptr(mask))


def seq_last_idx(B, seq_idx, seq_len, out):
    _chk(seq_idx, "i32", 2 * B); _chk(seq_len, "i32", B); _chk(out, "i32", B)
    _call("unreal_seq_last_idx", B, ptr(seq_idx), ptr(seq_len), ptr(out))


def rollout_stats(B, n_steps, score_valid, score_out, stats):
    _chk(n_steps, "i32", B); _chk(score_valid, "i32", B); _chk(score_out, "f32", B); _chk(stats, "f64", 3)
    _call("unreal_rollout_stats", B, ptr(n_steps), ptr(score_valid), ptr(score_out), ptr(stats))


def reset_state(B, terminal_end, c, h):
    _chk(terminal_end, "i32", B); _chk(c, "f32", B * 256); _chk(h, "f32", B * 256)
    _call("unreal_reset_state", B, ptr(terminal_end), ptr(c), ptr(h))


# ---- network -------------------------------------------------------------------------------------
ENC_PREPARED_BYTES = 45072          # include/unreal_hip.h: UNREAL_ENCODER_PREPARED_BYTES


def encoder_prepare(W1, b1, W2, scale, prepared=None):
    """The weights' share of encoder_fwd's prologue (scales + MFMA operand fragments) -> `prepared` (uint8
    [ENC_PREPARED_BYTES]); valid for these W1 / b1 / W2 values and this frame scale.  Returns the block."""
    _chk(W1, "f32", 3072); _chk(b1, "f32", 16); _chk(W2, "f32", 8192)
    if prepared is None:
        prepared = torch.empty(ENC_PREPARED_BYTES, dtype=torch.uint8, device=W1.device)
    _chk(prepared, "u8", ENC_PREPARED_BYTES, "prepared")
    _call("unreal_encoder_prepare", ptr(W1), ptr(b1), ptr(W2), float(scale), ptr(prepared), prepared.numel())
    return prepared


def encoder_fwd(frames, frame_idx, scale, W1, b1, W2, b2, f2_out, c1_out=None, n_frames_pool=None, relu_bits=None,
                f2_max=None, c1_max=None, prepared=None):
    """relu_bits: optional int16 [N * RELU_WORDS], bit (j % 16) of word j / 16 of a frame = f2[j] > 0.
    f2_max: optional absmax slot that receives max f2 (the A scale of the fc GEMM that follows).
    prepared: optional block from encoder_prepare(W1, b1, W2, scale) -- same results, shorter prologue per launch."""
    N = frame_idx.numel()
    _chk(frames, "u8"); _chk(frame_idx, "i32", N)
    _chk(W1, "f32", 3072); _chk(b1, "f32", 16); _chk(W2, "f32", 8192); _chk(b2, "f32", 32)
    _chk(f2_out, "f32", N * F2_DIM); _chk(c1_out, "f32", N * C1_DIM, optional=True)
    _chk(relu_bits, "i16", N * RELU_WORDS, "relu_bits", optional=True)
    _chk(f2_max, "f32", 1, "f2_max", optional=True); _chk(c1_max, "f32", 1, "c1_max", optional=True)
    _chk(prepared, "u8", ENC_PREPARED_BYTES, "prepared", optional=True)
    _call("unreal_encoder_fwd", N, ptr(frames), ptr(frame_idx), float(scale), ptr(W1), ptr(b1), ptr(W2), ptr(b2),
          ptr(c1_out), ptr(f2_out), ptr(relu_bits), ptr(f2_max), ptr(c1_max), ptr(prepared))


def encoder_bwd(frames, frame_idx, scale, W2, c1_saved, d2, dW1, db1, dW2, db2, c1_max=None, d2_max=None):
    """c1_max / d2_max: absmax slots covering c1_saved / d2 (None: reduced here with one extra launch each)."""
    N = frame_idx.numel()
    _chk(c1_max, "f32", 1, "c1_max", optional=True); _chk(d2_max, "f32", 1, "d2_max", optional=True)
    _chk(frames, "u8"); _chk(frame_idx, "i32", N); _chk(W2, "f32", 8192)
    _chk(c1_saved, "f32", N * C1_DIM); _chk(d2, "f32", N * F2_DIM)
    _chk(dW1, "f32", 3072); _chk(db1, "f32", 16); _chk(dW2, "f32", 8192); _chk(db2, "f32", 32)
    c1_max = _absmax_of(c1_saved, 1, N * C1_DIM, N * C1_DIM, c1_max)
    d2_max = _absmax_of(d2, 1, N * F2_DIM, N * F2_DIM, d2_max)
    _call("unreal_encoder_bwd", N, ptr(frames), ptr(frame_idx), float(scale), ptr(W2), ptr(c1_saved), ptr(c1_max), ptr(d2),
          ptr(d2_max), ptr(dW1), ptr(db1), ptr(dW2), ptr(db2))


def encoder_hw_fwd(frames, frame_idx, frame_shape, stride, scale, W1, b1, W2, b2, c1_out, f2_out, f2_max=None):
    """The conv trunk at frame_shape = (H, W) (csrc/encoder_hw.hip): frames uint8 `stride` bytes apart, c1_out
    [N, h1, w1, 16] (required), f2_out [N, h2, w2, 32]; f2_max: optional absmax slot that receives max f2."""
    H, W = int(frame_shape[0]), int(frame_shape[1])
    h1, w1, h2, w2, F = frame_dims(H, W)
    N = frame_idx.numel()
    if stride < H * W * 3:
        raise ValueError("frame stride %d < %d" % (stride, H * W * 3))
    _chk(frames, "u8", stride, "frames"); _chk(frame_idx, "i32", N, "frame_idx")
    _chk(W1, "f32", 3072, "W1"); _chk(b1, "f32", 16, "b1"); _chk(W2, "f32", 8192, "W2"); _chk(b2, "f32", 32, "b2")
    _chk(c1_out, "f32", N * h1 * w1 * 16, "c1_out"); _chk(f2_out, "f32", N * F, "f2_out")
    _chk(f2_max, "f32", 1, "f2_max", optional=True)
    _call("unreal_encoder_hw_fwd", N, H, W, ptr(frames), int(stride), ptr(frame_idx), float(scale), ptr(W1), ptr(b1),
          ptr(W2), ptr(b2), ptr(c1_out), ptr(f2_out), ptr(f2_max))


def encoder_hw_work_floats(N, frame_shape):
    """Floats of the work buffer encoder_hw_bwd needs for N frames of frame_shape (host-only query)."""
    import ctypes
    frame_dims(*frame_shape)
    out = ctypes.c_long(0)
    lib().call("unreal_encoder_hw_work_floats", int(N), int(frame_shape[0]), int(frame_shape[1]), ctypes.byref(out), None)
    return out.value


def encoder_hw_bwd(frames, frame_idx, frame_shape, stride, scale, W2, c1_saved, d2, dW1, db1, dW2, db2, work):
    """Backward of encoder_hw_fwd: d2 = d(loss)/d(conv2 pre-activation) [N, h2, w2, 32]; ADDS into dW1, db1, dW2, db2
    (deterministic: slab partials summed in a fixed order).  work: fp32, >= encoder_hw_work_floats(N, frame_shape)."""
    H, W = int(frame_shape[0]), int(frame_shape[1])
    h1, w1, h2, w2, F = frame_dims(H, W)
    N = frame_idx.numel()
    if stride < H * W * 3:
        raise ValueError("frame stride %d < %d" % (stride, H * W * 3))
    nw = encoder_hw_work_floats(N, (H, W))
    _chk(frames, "u8", stride, "frames"); _chk(frame_idx, "i32", N, "frame_idx"); _chk(W2, "f32", 8192, "W2")
    _chk(c1_saved, "f32", N * h1 * w1 * 16, "c1_saved"); _chk(d2, "f32", N * F, "d2")
    _chk(dW1, "f32", 3072, "dW1"); _chk(db1, "f32", 16, "db1"); _chk(dW2, "f32", 8192, "dW2"); _chk(db2, "f32", 32, "db2")
    _chk(work, "f32", nw, "work")
    _call("unreal_encoder_hw_bwd", N, H, W, ptr(frames), int(stride), ptr(frame_idx), float(scale), ptr(W2), ptr(c1_saved),
          ptr(d2), ptr(work), work.numel(), ptr(dW1), ptr(db1), ptr(dW2), ptr(db2))


def gemm(transA, transB, M, N, K, A, lda, B, ldb, C, ldc, bias=None, mask=None, ldm=0, flags=0, splitk=1):
    _chk(A, "f32", ((K - 1) * lda + M) if transA else ((M - 1) * lda + K), "A")
    _chk(B, "f32", ((N - 1) * ldb + K) if transB else ((K - 1) * ldb + N), "B")
    _chk(C, "f32", (M - 1) * ldc + N, "C")
    _chk(bias, "f32", N, "bias", optional=True)
    _chk(mask, "f32", (M - 1) * ldm + N if ldm else None, "mask", optional=True)
    _call("unreal_gemm_f32", int(transA), int(transB), M, N, K, ptr(A), lda, ptr(B), ldb, ptr(C), ldc, ptr(bias),
          ptr(mask), ldm, flags, splitk)


class AbsmaxPool(object):
    """Absmax slots (include/unreal_hip.h: one float on the device holding max |x| of a tensor) for one pass of the
    trainer: `reset()` zeroes them all with one fill, `new()` hands out the next one.  A producer kernel maxes its
    outputs into a slot, the fp16x2 GEMM that consumes the tensor derives the tensor's power-of-two scale from it."""

    def __init__(self, device, n=1024):
        self.buf = torch.zeros(n, dtype=torch.float32, device=device)
        self.n, self.next = n, 0

    def reset(self):
        self.buf.zero_()
        self.next = 0

    def new(self):
        if self.next >= self.n:
            raise RuntimeError("AbsmaxPool exhausted (%d slots): reset() it once per pass" % self.n)
        self.next += 1
        return self.buf[self.next - 1:self.next]


_SCRATCH = {}


def _scratch_slot(like):
    """A zeroed slot for callers that pass no absmax of their own (tests, one-off launches): ring of 64, stream-ordered."""
    dev = like.device
    st = _SCRATCH.get(dev)
    if st is None:
        st = _SCRATCH[dev] = [torch.zeros(64, dtype=torch.float32, device=dev), 0]
    st[1] = (st[1] + 1) % 64
    slot = st[0][st[1]:st[1] + 1]
    slot.zero_()
    return slot


def absmax(rows, cols, x, ld, slot):
    """slot = max(slot, max |x[r][c]|) over the rows x cols view of x (row stride ld)."""
    _chk(x, "f32", (rows - 1) * ld + cols, "x"); _chk(slot, "f32", 1, "slot")
    _call("unreal_absmax_f32", rows, cols, ptr(x), ld, ptr(slot))
    return slot


def _absmax_of(x, rows, cols, ld, slot):
    return slot if slot is not None else absmax(rows, cols, x, ld, _scratch_slot(x))


class SplitWeights:
    """fp16x2 shadow of one weight matrix as unreal_gemm_f32_split_nt wants its W operand: planes[t][n][k] (t = hi, lo of
    w * 2^k, k from the matrix's absmax slot `wmax`), rows padded with zeros to a multiple of 32 k.  `refresh()` re-reduces
    the maximum and re-splits from the live fp32 weights (after an optimiser step)."""

    def __init__(self, src, rows, cols, ld_src, transpose, offset=0, row_perm=0, wmax=None, defer=False):
        """wmax: a one-float view the caller owns (ShadowSet keeps the slots of all its shadows in one tensor, zeroed with one
        fill); defer: do not split now (a ShadowSet refreshes all its members together)."""
        self.src, self.rows, self.cols, self.ld_src, self.transpose, self.offset = src, rows, cols, ld_src, transpose, offset
        self.row_perm = row_perm
        self.N, self.K = (cols, rows) if transpose else (rows, cols)
        self.ldw = (self.K + 31) // 32 * 32
        self.plane = self.N * self.ldw
        self.planes = torch.zeros(2 * self.plane, dtype=torch.int16, device=src.device)
        self.wmax = torch.zeros(1, dtype=torch.float32, device=src.device) if wmax is None else wmax
        if not defer:
            self.refresh()

    def multi_descs(self):
        """-> (abs record or None, [split records]) for ShadowSet: pointers and sizes as Python ints."""
        if self.ld_src != self.cols:
            return None, None                         # a column window: not contiguous, refreshed by itself
        src = self.src.data_ptr() + 4 * self.offset
        return ((src, self.wmax.data_ptr(), self.rows * self.cols),
                [(src, self.planes.data_ptr(), self.wmax.data_ptr(), self.rows, self.cols, self.ld_src, int(bool(self.transpose)),
                  int(self.row_perm), self.ldw, self.plane)])

    def refresh(self):
        self.wmax.zero_()
        absmax(self.rows, self.cols, self.src[self.offset:], self.ld_src, self.wmax)
        split_f16x2(self.rows, self.cols, self.src[self.offset:], self.ld_src, self.transpose, self.planes, self.ldw,
                    self.plane, self.wmax, self.row_perm)


def split_f16x2(rows, cols, src, ld_src, transpose, dst, ld_dst, plane, wmax, row_perm=0):
    _chk(src, "f32", (rows - 1) * ld_src + cols, "src"); _chk(wmax, "f32", 1, "wmax")
    orows, ocols = (cols, rows) if transpose else (rows, cols)
    _chk(dst, "i16", plane + (orows - 1) * ld_dst + ocols, "dst")
    _call("unreal_split_f16x2", rows, cols, ptr(src), ld_src, int(bool(transpose)), int(row_perm), ptr(dst), ld_dst,
          plane, ptr(wmax))


class LstmKernelShadow:
    """Gate-interleaved fp16x2 shadow of the WHOLE BasicLSTMCell kernel [K_x + 256, 1024] as unreal_lstm_step_fwd(x=...)
    multiplies it: planes[t][1024][pad32(K_x) + 256] -- input rows, zero padding to a K tile, recurrent rows; one scale
    (absmax slot) for the whole kernel."""

    def __init__(self, kernel, K_x, wmax=None, defer=False):
        self.src, self.K_x, self.row_perm = kernel, K_x, 1
        self.kxpad = (K_x + 31) // 32 * 32
        self.N, self.K = 1024, self.kxpad + 256
        self.ldw = self.K
        self.plane = self.N * self.ldw
        self.planes = torch.zeros(2 * self.plane, dtype=torch.int16, device=kernel.device)
        self.wmax = torch.zeros(1, dtype=torch.float32, device=kernel.device) if wmax is None else wmax
        if not defer:
            self.refresh()

    def multi_descs(self):
        src, dst, wm = self.src.data_ptr(), self.planes.data_ptr(), self.wmax.data_ptr()
        return ((src, wm, (self.K_x + 256) * 1024),
                [(src, dst, wm, self.K_x, 1024, 1024, 1, 1, self.ldw, self.plane),
                 (src + 4 * self.K_x * 1024, dst + 2 * self.kxpad, wm, 256, 1024, 1024, 1, 1, self.ldw, self.plane)])

    def refresh(self):
        self.wmax.zero_()
        absmax(self.K_x + 256, 1024, self.src, 1024, self.wmax)
        split_f16x2(self.K_x, 1024, self.src, 1024, True, self.planes, self.ldw, self.plane, self.wmax, 1)
        split_f16x2(256, 1024, self.src[self.K_x * 1024:], 1024, True, self.planes[self.kxpad:], self.ldw, self.plane,
                    self.wmax, 1)


class ShadowSet(object):
    """All weight shadows of a network refreshed together: one fill of their absmax slots, one launch that reduces every
    matrix's maximum, one that writes every matrix's planes (unreal_shadow_refresh_multi) -- instead of fill + maximum +
    split per matrix.  `make` is called with a factory: wmax_view = slots[i:i + 1] for shadow i."""

    def __init__(self, device, n_shadows):
        self.device = device
        self.slots = torch.zeros(n_shadows, dtype=torch.float32, device=device)
        self.members, self._descs = [], None

    def slot(self):
        i = len(self.members)
        if i >= self.slots.numel():
            raise RuntimeError("ShadowSet: more shadows than slots")
        return self.slots[i:i + 1]

    def add(self, shadow):
        self.members.append(shadow)
        self._descs = None
        return shadow

    def _build(self):
        abs_rows, split_rows, singles = [], [], []
        ab, sb = 0, 0
        for m in self.members:
            a, sp = m.multi_descs()
            if a is None:
                singles.append(m)
                continue
            abs_rows.append([a[0], a[1], a[2], ab])
            ab += (a[2] + 8191) // 8192
            for r in sp:
                tiles_x = (r[4] + 31) // 32
                split_rows.append(list(r) + [tiles_x, sb])
                sb += tiles_x * ((r[3] + 31) // 32)
        mk = lambda rows: torch.tensor(rows, dtype=torch.int64).to(self.device).contiguous()
        self._descs = (mk(abs_rows), len(abs_rows), ab, mk(split_rows), len(split_rows), sb, singles)

    def refresh(self):
        if self._descs is None:
            self._build()
        a, na, ab, sp, ns, sb, singles = self._descs
        self.slots.zero_()
        if na:
            _call("unreal_shadow_refresh_multi", ptr(a), na, ab, ptr(sp), ns, sb)
        for m in singles:                    # (zeroed above; their own refresh would zero the slot again: harmless)
            m.refresh()


def gemm_split_nt(M, N, K, A, lda, W, C, ldc, bias=None, mask=None, ldm=0, flags=0, splitk=1, a_max=None, c_max=None):
    """C = A[M,K] @ W[N,K]^T (fp32-grade: fp16 hi + lo operands with per-tensor scales, 3 term pairs on the fp16 matrix
    cores); W is a SplitWeights.  a_max: absmax slot covering A (None: reduced here with one extra launch); c_max: slot
    that receives max |C|.
    mask: fp32 [M, ldm] with GEMM_RELU_MASK, or int16 bit words [M, ldm] with GEMM_RELU_BITS (encoder_fwd relu_bits)."""
    if W.N != N or W.K != K:
        raise ValueError("split weights are [%d,%d], GEMM wants [%d,%d]" % (W.N, W.K, N, K))
    _chk(A, "f32", (M - 1) * lda + K, "A"); _chk(C, "f32", (M - 1) * ldc + N, "C")
    _chk(bias, "f32", N, "bias", optional=True)
    if flags & GEMM_RELU_BITS:
        _chk(mask, "i16", (M - 1) * ldm + (N + 15) // 16, "mask bits")
    else:
        _chk(mask, "f32", (M - 1) * ldm + N if ldm else None, "mask", optional=True)
    _chk(a_max, "f32", 1, "a_max", optional=True); _chk(c_max, "f32", 1, "c_max", optional=True)
    if c_max is not None and (flags & GEMM_ATOMIC):
        raise ValueError("gemm_split_nt: the split-K / atomic epilogue cannot commit max |C| (c_max); reduce it with "
                         "ops.absmax after the launch")
    if K < 64 and not (flags & GEMM_RELU_BITS):
        # one or two K tiles: nothing to split for -- hi + lo carries 22 bits per element, which only pays off against the
        # rounding of a long accumulation (at K = 3 the split result is ~2.5x the fp32 chain's error).  Such products (none
        # on the trainer's path) go to the exact fp32-MFMA kernel with the weights the shadow was made from.
        if W.transpose:          # src is [K][N]
            gemm(False, False, M, N, K, A, lda, W.src[W.offset:], W.ld_src, C, ldc, bias, mask, ldm, flags, splitk)
        else:                    # src is [N][K]
            gemm(False, True, M, N, K, A, lda, W.src[W.offset:], W.ld_src, C, ldc, bias, mask, ldm, flags, splitk)
        if c_max is not None:
            absmax(M, N, C, ldc, c_max)
        return
    a_max = _absmax_of(A, M, K, lda, a_max)
    _call("unreal_gemm_f32_split_nt", M, N, K, ptr(A), lda, ptr(a_max), ptr(W.planes), W.ldw, W.plane, ptr(W.wmax), ptr(C), ldc,
          ptr(c_max), ptr(bias), ptr(mask), ldm, flags, splitk)


FEW_ROWS = 2048        # at most this many rows: a long-K product has too few tiles for the chip (gemm_split_nt_slabs)


def slab_count(M, N, K):
    """K slabs for gemm_split_nt_slabs, by the same-process A/B at N = 256, K = 2592 (tools/exp/fc_slabs_ab.py,
    profiles/r04_ab_summary.md 3e): 8 up to 32 tiles of 64 x 64 (<= 512 rows), 4 up to 64, 2 up to 128 (2048 rows); from 4096
    rows on the one-launch kernel wins.  0 = use the one-launch kernel."""
    if M > FEW_ROWS or K < 1024:
        return 0
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    return 8 if tiles <= 32 else 4 if tiles <= 64 else 2 if tiles <= 128 else 0


def gemm_split_nt_slabs(M, N, K, A, lda, W, C, ldc, partials, splitk, bias=None, flags=0, a_max=None, c_max=None):
    """gemm_split_nt for few rows and a long K: `splitk` K slabs in separate workgroups -> partials (>= splitk * M * pad4(N)
    floats), added in slab order by a second launch that applies bias / ReLU and commits max |C| (deterministic)."""
    if W.N != N or W.K != K:
        raise ValueError("split weights are [%d,%d], GEMM wants [%d,%d]" % (W.N, W.K, N, K))
    _chk(A, "f32", (M - 1) * lda + K, "A"); _chk(C, "f32", (M - 1) * ldc + N, "C")
    _chk(bias, "f32", N, "bias", optional=True); _chk(partials, "f32", splitk * M * ((N + 3) // 4 * 4), "partials")
    _chk(a_max, "f32", 1, "a_max", optional=True); _chk(c_max, "f32", 1, "c_max", optional=True)
    a_max = _absmax_of(A, M, K, lda, a_max)
    _call("unreal_gemm_f32_split_nt_slabs", M, N, K, ptr(A), lda, ptr(a_max), ptr(W.planes), W.ldw, W.plane, ptr(W.wmax), ptr(C),
          ldc, ptr(c_max), ptr(bias), flags, splitk, ptr(partials), partials.numel())


def gemm_split_tn(M, N, K, A, lda, B, ldb, C, ldc, splitk=1, colsum=None, a_max=None, b_max=None):
    """C[M,N] += A[K,M]^T @ B[K,N] (wgrad; fp32-grade on the fp16 matrix cores, split-K atomics into C);
    colsum[N] += column sums of B (the bias gradient of the same layer) when given.
    a_max / b_max: absmax slots covering A / B (None: reduced here with one extra launch each)."""
    _chk(A, "f32", (K - 1) * lda + M, "A"); _chk(B, "f32", (K - 1) * ldb + N, "B"); _chk(C, "f32", (M - 1) * ldc + N, "C")
    _chk(colsum, "f32", N, "colsum", optional=True)
    _chk(a_max, "f32", 1, "a_max", optional=True); _chk(b_max, "f32", 1, "b_max", optional=True)
    a_max = _absmax_of(A, K, M, lda, a_max)
    b_max = _absmax_of(B, K, N, ldb, b_max)
    _call("unreal_gemm_f32_split_tn", M, N, K, ptr(A), lda, ptr(a_max), ptr(B), ldb, ptr(b_max), ptr(C), ldc, ptr(colsum),
          splitk)


def lstm_step_fwd(rows, h_prev, Wh, gates, bias, c_prev, c_out, h_out, ld_hprev=256, ld_h=256, x=None, ldx=0, Kx=0,
                  x_max=None):
    """One BasicLSTMCell step with the gate math fused into the product.
    x None : gates (in: x-half pre-activations, out: activated gates) += h_prev @ Wh;
             Wh = SplitWeights(kernel recurrent rows, transpose=True, row_perm=1).
    x given: gates (out) = act([x | h_prev] @ kernel); Wh = LstmKernelShadow (gate-interleaved [1024, pad32(Kx) + 256])."""
    kxpad = (Kx + 31) // 32 * 32 if x is not None else 0
    if Wh.N != 1024 or Wh.K != kxpad + 256 or Wh.row_perm != 1:
        raise ValueError("lstm_step_fwd needs the gate-interleaved [1024,%d] shadow of the LSTM kernel" % (kxpad + 256))
    _chk(h_prev, "f32", (rows - 1) * ld_hprev + 256, "h_prev"); _chk(gates, "f32", rows * 1024, "gates")
    _chk(bias, "f32", 1024, "bias"); _chk(c_prev, "f32", rows * 256, "c_prev"); _chk(c_out, "f32", rows * 256, "c_out")
    _chk(h_out, "f32", (rows - 1) * ld_h + 256, "h_out")
    _chk(x, "f32", (rows - 1) * ldx + Kx if x is not None else None, "x", optional=True)
    _chk(x_max, "f32", 1, "x_max", optional=True)
    if x is not None:        # |h_prev| < 1 is covered by the kernel; x needs its slot
        x_max = _absmax_of(x, rows, Kx, ldx, x_max)
    _call("unreal_lstm_step_fwd", rows, ptr(x), ldx, Kx, ptr(x_max), ptr(h_prev), ld_hprev, ptr(Wh.planes), Wh.ldw, Wh.plane,
          ptr(Wh.wmax), ptr(gates), ptr(bias), ptr(c_prev), ptr(c_out), ptr(h_out), ld_h)


def lstm_gates_fwd(rows, pre, bias, c_prev, gates_act, c_out, h_out, ld_h=256):
    _chk(pre, "f32", rows * 1024); _chk(bias, "f32", 1024); _chk(c_prev, "f32", rows * 256)
    _chk(gates_act, "f32", rows * 1024, optional=True); _chk(c_out, "f32", rows * 256)
    _chk(h_out, "f32", (rows - 1) * ld_h + 256)
    _call("unreal_lstm_gates_fwd", rows, ptr(pre), ptr(bias), ptr(c_prev), ptr(gates_act), ptr(c_out), ptr(h_out),
          ld_h)


def lstm_gates_bwd(rows, dh_above, dh_rec, dc_io, gates_act, c_prev, c_new, dpre, c_max0=None, c_max1=None):
    _chk(dh_above, "f32", rows * 256); _chk(dh_rec, "f32", rows * 256, optional=True)
    _chk(dc_io, "f32", rows * 256); _chk(gates_act, "f32", rows * 1024); _chk(c_prev, "f32", rows * 256)
    _chk(c_new, "f32", rows * 256); _chk(dpre, "f32", rows * 1024)
    _chk(c_max0, "f32", 1, "c_max0", optional=True); _chk(c_max1, "f32", 1, "c_max1", optional=True)
    _call("unreal_lstm_gates_bwd", rows, ptr(dh_above), ptr(dh_rec), ptr(dc_io), ptr(gates_act), ptr(c_prev),
          ptr(c_new), ptr(dpre), ptr(c_max0), ptr(c_max1))


def lstm_bptt_step(rows, d_gates, Wh, dh_above, dc_io, gates_act, c_prev, c_new, dpre, a_max=None, c_max0=None,
                   c_max1=None):
    """dh_rec = d_gates @ Wh^T and, in the same launch, the gate backward of the earlier step (dh = dh_above + dh_rec).
    Wh: SplitWeights(kernel recurrent rows, transpose=False) -- [256, 1024]."""
    if Wh.N != 256 or Wh.K != 1024 or getattr(Wh, "row_perm", 0):
        raise ValueError("lstm_bptt_step needs the natural [256,1024] shadow of the recurrent kernel rows")
    _chk(d_gates, "f32", rows * 1024, "d_gates"); _chk(dh_above, "f32", rows * 256); _chk(dc_io, "f32", rows * 256)
    _chk(gates_act, "f32", rows * 1024); _chk(c_prev, "f32", rows * 256); _chk(c_new, "f32", rows * 256)
    _chk(dpre, "f32", rows * 1024)
    _chk(a_max, "f32", 1, "a_max", optional=True); _chk(c_max0, "f32", 1, "c_max0", optional=True)
    _chk(c_max1, "f32", 1, "c_max1", optional=True)
    a_max = _absmax_of(d_gates, rows, 1024, 1024, a_max)
    _call("unreal_lstm_bptt_step", rows, ptr(d_gates), ptr(a_max), ptr(Wh.planes), Wh.ldw, Wh.plane, ptr(Wh.wmax),
          ptr(dh_above), ptr(dc_io), ptr(gates_act), ptr(c_prev), ptr(c_new), ptr(dpre), ptr(c_max0), ptr(c_max1))


def linear_small_fwd(rows, K, NOUT, X, ldx, W, b, out, ldo):
    _chk(X, "f32", (rows - 1) * ldx + K); _chk(W, "f32", K * NOUT); _chk(b, "f32", NOUT)
    _chk(out, "f32", (rows - 1) * ldo + NOUT)
    _call("unreal_linear_small_fwd", rows, K, NOUT, ptr(X), ldx, ptr(W), ptr(b), ptr(out), ldo)


def linear_small_bwd(rows, K, NOUT, X, ldx, dO, ldo, W, dX, lddx, accumulate_dx, dW, db, dw_stride_k=0, dw_stride_n=0):
    _chk(X, "f32", (rows - 1) * ldx + K); _chk(dO, "f32", (rows - 1) * ldo + NOUT)
    _chk(W, "f32", K * NOUT, optional=dX is None)
    _chk(dX, "f32", (rows - 1) * lddx + K, optional=True)
    sk, sn = (dw_stride_k, dw_stride_n) if (dw_stride_k or dw_stride_n) else (NOUT, 1)
    _chk(dW, "f32", (K - 1) * sk + (NOUT - 1) * sn + 1)
    _chk(db, "f32", NOUT, optional=True)
    _call("unreal_linear_small_bwd", rows, K, NOUT, ptr(X), ldx, ptr(dO), ldo, ptr(W), ptr(dX), lddx,
          int(accumulate_dx), ptr(dW), int(dw_stride_k), int(dw_stride_n), ptr(db))


def policy_step(rows, A, X, ldx, Wp, bp, Wv, bv, u, pi_out, v_out, action):
    """pi, v and the sampled (u) or greedy (u None) action of `rows` feature rows in one launch."""
    _chk(X, "f32", (rows - 1) * ldx + 256, "X"); _chk(Wp, "f32", 256 * A); _chk(bp, "f32", A); _chk(Wv, "f32", 256)
    _chk(bv, "f32", 1); _chk(u, "f64", rows, "u", optional=True); _chk(pi_out, "f32", rows * A); _chk(v_out, "f32", rows)
    _chk(action, "i32", rows)
    _call("unreal_policy_step", rows, A, ptr(X), ldx, ptr(Wp), ptr(bp), ptr(Wv), ptr(bv), ptr(u), ptr(pi_out), ptr(v_out),
          ptr(action))


def softmax_sample(rows, A, logits_pi, ld, u=None, action=None):
    _chk(logits_pi, "f32", (rows - 1) * ld + A); _chk(u, "f64", rows, optional=True)
    _chk(action, "i32", rows, optional=True)
    _call("unreal_softmax_sample", rows, A, ptr(logits_pi), ld, ptr(u), ptr(action))


def base_loss_grad(rows, A, pi, ld_pi, v, action, adv, R, active, beta, grad_scale, dlogits, dv, losses):
    _chk(pi, "f32", (rows - 1) * ld_pi + A); _chk(v, "f32", rows); _chk(action, "i32", rows)
    _chk(adv, "f32", rows); _chk(R, "f32", rows); _chk(active, "i32", rows)
    _chk(dlogits, "f32", rows * A); _chk(dv, "f32", rows); _chk(losses, "f32", 3)
    _call("unreal_base_loss_grad", rows, A, ptr(pi), ld_pi, ptr(v), ptr(action), ptr(adv), ptr(R), ptr(active),
          float(beta), float(grad_scale), ptr(dlogits), ptr(dv), ptr(losses))


def ppo_heads_loss_grad(rows, A, X, ldx, Wp, bp, Wv, bv, pi_old, ld_old, action, adv, R, active, clip_eps, beta, grad_scale,
                        pi_out, v_out, dlogits, dv, losses, stats_i, stats_f):
    """Sample reuse: heads forward + clipped-surrogate loss and gradient of `rows` re-evaluated rollout rows in
    one launch.  pi_out / v_out as policy_step(u=None), bit for bit; dlogits / dv (None: forward only) as base_loss_grad's
    with the PPO policy term against pi_old; losses[3] += policy, value, entropy; stats_i[2] += (clipped, counted) rows;
    stats_f[2] += (sum rho - 1 - ln rho, sum |rho - 1|)."""
    rows, A, ldx, ld_old = int(rows), int(A), int(ldx), int(ld_old)
    if rows <= 0 or not 2 <= A <= 18 or ldx < 256 or ld_old < A:
        raise ValueError("ppo_heads_loss_grad: rows=%d A=%d ldx=%d ld_old=%d" % (rows, A, ldx, ld_old))
    if not 0.0 < float(clip_eps) < 1.0:
        raise ValueError("ppo_heads_loss_grad: clip_eps = %r outside (0, 1)" % (clip_eps,))
    _chk(X, "f32", (rows - 1) * ldx + 256, "X"); _chk(Wp, "f32", 256 * A, "Wp"); _chk(bp, "f32", A, "bp")
    _chk(Wv, "f32", 256, "Wv"); _chk(bv, "f32", 1, "bv"); _chk(pi_old, "f32", (rows - 1) * ld_old + A, "pi_old")
    _chk(action, "i32", rows, "action"); _chk(adv, "f32", rows, "adv"); _chk(R, "f32", rows, "R")
    _chk(active, "i32", rows, "active"); _chk(pi_out, "f32", rows * A, "pi_out"); _chk(v_out, "f32", rows, "v_out")
    _chk(dlogits, "f32", rows * A, "dlogits", optional=True); _chk(dv, "f32", rows, "dv", optional=dlogits is None)
    _chk(losses, "f32", 3, "losses"); _chk(stats_i, "i32", 2, "stats_i"); _chk(stats_f, "f32", 2, "stats_f")
    _call("unreal_ppo_heads_loss_grad", rows, A, ptr(X), ldx, ptr(Wp), ptr(bp), ptr(Wv), ptr(bv), ptr(pi_old), ld_old,
          ptr(action), ptr(adv), ptr(R), ptr(active), float(clip_eps), float(beta), float(grad_scale), ptr(pi_out),
          ptr(v_out), ptr(dlogits), ptr(dv) if dlogits is not None else None, ptr(losses), ptr(stats_i), ptr(stats_f))


def vr_loss_grad(rows, v, R, mask, grad_scale, dv, loss):
    _chk(v, "f32", rows); _chk(R, "f32", rows); _chk(mask, "i32", rows); _chk(dv, "f32", rows); _chk(loss, "f32", 1)
    _call("unreal_vr_loss_grad", rows, ptr(v), ptr(R), ptr(mask), float(grad_scale), ptr(dv), ptr(loss))


def rp_loss_grad(rows, logits, cls, grad_scale, prob, dlogits, loss):
    _chk(logits, "f32", rows * 3); _chk(cls, "i32", rows); _chk(prob, "f32", rows * 3, optional=True)
    _chk(dlogits, "f32", rows * 3); _chk(loss, "f32", 1)
    _call("unreal_rp_loss_grad", rows, ptr(logits), ptr(cls), float(grad_scale), ptr(prob), ptr(dlogits), ptr(loss))


def colsum(rows, cols, X, ld, out):
    _chk(X, "f32", (rows - 1) * ld + cols); _chk(out, "f32", cols)
    _call("unreal_colsum", rows, cols, ptr(X), ld, ptr(out))


def relu_mask(rows, cols, d, ldd, src, lds):
    _chk(d, "f32", (rows - 1) * ldd + cols); _chk(src, "f32", (rows - 1) * lds + cols)
    _call("unreal_relu_mask", rows, cols, ptr(d), ldd, ptr(src), lds)


def pc_deconv_fwd(N, A, hp, Wv, bv, Wa, ba, qmax=None, action=None, target=None, mask=None, lam=0.0,
                  grad_scale=1.0, d_dec=None, loss=None, hp_max=None, ddec_max=None):
    """hp_max: absmax slot covering hp (None: reduced here with one extra launch); ddec_max: slot that receives an upper
    bound of max |d_dec| (training mode; what pc_deconv_bwd scales its d_dec planes by)."""
    _chk(hp, "f32", N * F2_DIM); _chk(Wv, "f32", 512); _chk(bv, "f32", 1); _chk(Wa, "f32", 512 * A); _chk(ba, "f32", A)
    _chk(qmax, "f32", N * PC_CELLS, optional=True); _chk(action, "i32", N, optional=True)
    _chk(target, "f32", N * PC_CELLS, optional=True); _chk(mask, "i32", N, optional=True)
    _chk(d_dec, "f32", N * PC_CELLS * (1 + A), optional=True); _chk(loss, "f32", 1, optional=True)
    _chk(hp_max, "f32", 1, "hp_max", optional=True); _chk(ddec_max, "f32", 1, "ddec_max", optional=True)
    hp_max = _absmax_of(hp, N, F2_DIM, F2_DIM, hp_max)
    _call("unreal_pc_deconv_fwd", N, A, ptr(hp), ptr(hp_max), ptr(Wv), ptr(bv), ptr(Wa), ptr(ba), ptr(qmax), ptr(action),
          ptr(target), ptr(mask), float(lam), float(grad_scale), ptr(d_dec), ptr(ddec_max), ptr(loss))


def pc_deconv_bwd(N, A, hp, d_dec, Wv, Wa, d_hp, dWv, dbv, dWa, dba, dhp_max=None, hp_max=None, ddec_max=None):
    """hp_max / ddec_max: absmax slots covering hp / d_dec (None: reduced here with one extra launch each)."""
    _chk(hp, "f32", N * F2_DIM); _chk(d_dec, "f32", N * PC_CELLS * (1 + A)); _chk(Wv, "f32", 512)
    _chk(Wa, "f32", 512 * A); _chk(d_hp, "f32", N * F2_DIM); _chk(dWv, "f32", 512); _chk(dbv, "f32", 1)
    _chk(dWa, "f32", 512 * A); _chk(dba, "f32", A)
    _chk(dhp_max, "f32", 1, "dhp_max", optional=True)
    _chk(hp_max, "f32", 1, "hp_max", optional=True); _chk(ddec_max, "f32", 1, "ddec_max", optional=True)
    hp_max = _absmax_of(hp, N, F2_DIM, F2_DIM, hp_max)
    ddec_max = _absmax_of(d_dec, N, PC_CELLS * (1 + A), PC_CELLS * (1 + A), ddec_max)
    _call("unreal_pc_deconv_bwd", N, A, ptr(hp), ptr(hp_max), ptr(d_dec), ptr(ddec_max), ptr(Wv), ptr(Wa), ptr(d_hp),
          ptr(dhp_max), ptr(dWv), ptr(dbv), ptr(dWa), ptr(dba))


def pc_deconv_train(N, A, hp, Wv, bv, Wa, ba, action, target, mask, lam, grad_scale, loss, d_hp, dWv, dbv, dWa, dba,
                    dhp_max=None, hp_max=None, d_dec=None):
    """pc_deconv_fwd (training mode) + pc_deconv_bwd in one launch; d_dec stays on chip (optional output for inspection)."""
    _chk(hp, "f32", N * F2_DIM); _chk(Wv, "f32", 512); _chk(bv, "f32", 1); _chk(Wa, "f32", 512 * A); _chk(ba, "f32", A)
    _chk(action, "i32", N); _chk(target, "f32", N * PC_CELLS); _chk(mask, "i32", N); _chk(loss, "f32", 1)
    _chk(d_hp, "f32", N * F2_DIM); _chk(dWv, "f32", 512); _chk(dbv, "f32", 1); _chk(dWa, "f32", 512 * A); _chk(dba, "f32", A)
    _chk(dhp_max, "f32", 1, "dhp_max", optional=True); _chk(hp_max, "f32", 1, "hp_max", optional=True)
    _chk(d_dec, "f32", N * PC_CELLS * (1 + A), optional=True)
    hp_max = _absmax_of(hp, N, F2_DIM, F2_DIM, hp_max)
    _call("unreal_pc_deconv_train", N, A, ptr(hp), ptr(hp_max), ptr(Wv), ptr(bv), ptr(Wa), ptr(ba), ptr(action), ptr(target),
          ptr(mask), float(lam), float(grad_scale), ptr(loss), ptr(d_hp), ptr(dhp_max), ptr(dWv), ptr(dbv), ptr(dWa), ptr(dba),
          ptr(d_dec))


def axpy(alpha, x, y):
    """y += alpha * x (f32 device vectors)."""
    _chk(x, "f32"); _chk(y, "f32", x.numel())
    _call("unreal_axpy_f32", x.numel(), float(alpha), ptr(x), ptr(y))


def copy_(dst, src):
    """dst[:] = src for device tensors of one 4-byte dtype (f32 / i32), as a kernel of this library."""
    if dst.dtype != src.dtype or dst.dtype not in (torch.float32, torch.int32):
        raise ValueError("copy_: %s <- %s" % (dst.dtype, src.dtype))
    if not (dst.is_cuda and src.is_cuda and dst.is_contiguous() and src.is_contiguous()):
        raise ValueError("copy_ needs contiguous device tensors (no CPU fallback)")
    if dst.numel() != src.numel():
        raise ValueError("copy_: %d <- %d elements" % (dst.numel(), src.numel()))
    _call("unreal_copy_words", dst.numel(), ptr(src), ptr(dst))
    return dst


# ---- optimiser -----------------------------------------------------------------------------------
def grad_norm(grad, scratch, norm_out):
    _chk(grad, "f32"); _chk(scratch, "f32", 256); _chk(norm_out, "f32", 1)
    _call("unreal_grad_norm", ptr(grad), grad.numel(), ptr(scratch), ptr(norm_out))


def rmsprop_step(var, ms, mom, grad, lr, decay, momentum, eps, clip_norm, norm):
    n = var.numel()
    _chk(var, "f32"); _chk(ms, "f32", n); _chk(mom, "f32", n); _chk(grad, "f32", n)
    _chk(norm, "f32", 1, optional=True)
    _call("unreal_rmsprop_step", ptr(var), ptr(ms), ptr(mom), ptr(grad), n, float(lr), float(decay),
          float(momentum), float(eps), float(clip_norm), ptr(norm))


def adam_step(var, m, v, grad, lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip_norm, norm):
    """Global-norm clip + Adam / AdamW on flat buffers: PyTorch's arithmetic in fp32, bc1 = 1 - beta1^t and
    bc2 = 1 - beta2^t from the caller's step count; norm from grad_norm (None with clip_norm <= 0)."""
    n = var.numel()
    _chk(var, "f32", name="var"); _chk(m, "f32", n, "m"); _chk(v, "f32", n, "v"); _chk(grad, "f32", n, "grad")
    _chk(norm, "f32", 1, "norm", optional=not clip_norm > 0)
    _call("unreal_adam_step", ptr(var), ptr(m), ptr(v), ptr(grad), n, float(lr), float(beta1), float(beta2), float(eps),
          float(weight_decay), float(bc1), float(bc2), float(clip_norm), ptr(norm))


def adv_normalize(rows, adv, active, eps, adv_out, stats):
    """Masked advantage normalisation: adv_out = (adv - mean) / (std + eps) over the rows with active != 0, 0 on
    the others (adv itself with fewer than 2 active rows); stats[3] += mean, std, 1."""
    rows = int(rows)
    if rows <= 0:
        raise ValueError("adv_normalize: rows=%d" % rows)
    if not 0.0 < float(eps) < float("inf"):
        raise ValueError("adv_normalize: eps = %r, a finite number > 0" % (eps,))
    _chk(adv, "f32", rows, "adv"); _chk(active, "i32", rows, "active"); _chk(adv_out, "f32", rows, "adv_out")
    _chk(stats, "f32", 3, "stats")
    if adv_out.data_ptr() == adv.data_ptr():
        raise ValueError("adv_normalize: adv_out must not alias adv")
    _call("unreal_adv_normalize", rows, ptr(adv), ptr(active), float(eps), ptr(adv_out), ptr(stats))


def minibatch_gather(T, Bg, Bm, j0, A, frame_idx, actions, active, adv, R, pi, frame_idx_out, actions_out, active_out,
                     adv_out, R_out, pi_out, side=0, ld=256, xcat=None, xcat_out=None, c0=None, h0=None, c0_out=None,
                     h0_out=None):
    """Minibatched reuse epochs: rows t * Bg + j0 + j of a rollout over Bg actors -> rows t * Bm + j (t < T,
    j < Bm) of every per-row stream of a reuse pass, in one launch; bit for bit.  With an LSTM (all six of xcat .. h0_out)
    also the `side` columns from column 256 of the xcat rows (leading dimension `ld` on both sides) and the start state of
    the actors [j0, j0 + Bm); feed-forward: none of the six."""
    T, Bg, Bm, j0, A, side, ld = int(T), int(Bg), int(Bm), int(j0), int(A), int(side), int(ld)
    if T <= 0 or Bm <= 0 or j0 < 0 or j0 + Bm > Bg or not 2 <= A <= 18:
        raise ValueError("minibatch_gather: T=%d Bg=%d Bm=%d j0=%d A=%d" % (T, Bg, Bm, j0, A))
    if side < 0 or 256 + side > ld:
        raise ValueError("minibatch_gather: side=%d does not fit in ld=%d" % (side, ld))
    lstm = (xcat, xcat_out, c0, h0, c0_out, h0_out)
    if any(t is not None for t in lstm) and any(t is None for t in lstm):
        raise ValueError("minibatch_gather: xcat, xcat_out, c0, h0, c0_out, h0_out go together (all, or none without an LSTM)")
    src, dst = T * Bg, T * Bm
    for t, dt, n, name in ((frame_idx, "i32", src, "frame_idx"), (actions, "i32", src, "actions"),
                           (active, "i32", src, "active"), (adv, "f32", src, "adv"), (R, "f32", src, "R"),
                           (pi, "f32", src * A, "pi"), (frame_idx_out, "i32", dst, "frame_idx_out"),
                           (actions_out, "i32", dst, "actions_out"), (active_out, "i32", dst, "active_out"),
                           (adv_out, "f32", dst, "adv_out"), (R_out, "f32", dst, "R_out"), (pi_out, "f32", dst * A, "pi_out")):
        _chk(t, dt, n, name)
    if xcat is not None:
        _chk(xcat, "f32", (src - 1) * ld + 256 + side, "xcat"); _chk(xcat_out, "f32", (dst - 1) * ld + 256 + side, "xcat_out")
        _chk(c0, "f32", Bg * 256, "c0"); _chk(h0, "f32", Bg * 256, "h0")
        _chk(c0_out, "f32", Bm * 256, "c0_out"); _chk(h0_out, "f32", Bm * 256, "h0_out")
        if any(t.data_ptr() % 16 for t in (c0, h0, c0_out, h0_out)):
            raise ValueError("minibatch_gather: c0 / h0 must be 16-byte aligned")
    _call("unreal_minibatch_gather", T, Bg, Bm, j0, A, ptr(frame_idx), ptr(actions), ptr(active), ptr(adv), ptr(R), ptr(pi),
          ptr(frame_idx_out), ptr(actions_out), ptr(active_out), ptr(adv_out), ptr(R_out), ptr(pi_out), side, ld, ptr(xcat),
          ptr(xcat_out), ptr(c0), ptr(h0), ptr(c0_out), ptr(h0_out))
