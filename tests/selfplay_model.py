"""Host model of the device arcade's self-play duel in plain Python / numpy, written from the rules in
include/unreal_hip.h and the issue's text, not from the kernel.  It is built on HostDuel (tests/duel_model.py), whose
state, serve draw, return segments and render it uses as they are.

TwoSeatDuel is the canonical game of one pair: HostDuel with the scripted follower replaced by seat 1's move and with
both seats' rewards.  mirror() is M.  HostSeat is one ACTOR with HostDuel's interface: like a workgroup of the device it
owns a full copy of its pair's game, steps it with its own action and its partner's, and keeps its own view (record,
frame, reward).  Its partner's actions come from a script (a list it consumes, or noop without one), so
OracleTrainer(envs=...) accepts it.

Fixed here: M is applied whatever the state (a reset record's by = 0 is 86 in seat 1's view; a waiting ball is not drawn);
word 13 counts the tick in which `theirs` reaches `points`, once, as word 12 does for `mine`."""
import numpy as np

try:
    from duel_model import HostDuel
    from arcade_model import pixel_change, NOOP, FIRE, RIGHT, LEFT
except ImportError:            # imported as tests.<module>
    from tests.duel_model import HostDuel
    from tests.arcade_model import pixel_change, NOOP, FIRE, RIGHT, LEFT


def mirror(rec):
    """M of a record or of an array of records [..., 16] -> a new array."""
    r = np.array(rec, dtype=np.int32, copy=True)
    m = r.copy()
    m[..., 0], m[..., 6] = r[..., 6], r[..., 0]             # px <-> ox
    m[..., 2] = 86 - r[..., 2]                              # by
    m[..., 4] = -r[..., 4]                                  # vy
    m[..., 7], m[..., 8] = r[..., 8], r[..., 7]             # mine <-> theirs
    m[..., 10], m[..., 11] = r[..., 11], r[..., 10]         # points won <-> points lost
    m[..., 12], m[..., 13] = r[..., 13], r[..., 12]         # own matches won <-> the other seat's
    return m


class TwoSeatDuel(HostDuel):
    """The canonical game of the pair whose seat 0 is global actor g0 (even): `conf` is an ArcadeSelfPlay."""

    def __init__(self, conf, g0, seed=0):
        assert g0 % 2 == 0
        self.other_matches = 0
        HostDuel.__init__(self, conf.scripted, g0, seed, frames=False)      # (opponent_width = paddle_width)

    def record(self):
        rec = HostDuel.record(self).copy()
        rec[13] = self.other_matches
        return rec

    def _micro_step2(self):
        """-> (seat 0's reward, seat 1's reward, a point was made)."""
        c = self.c
        w = c.paddle_width
        tx = self.bx + self.vx
        if tx < 2 or tx + 1 > 81:
            self.events.add("wall_left" if tx < 2 else "wall_right")
            self.vx = -self.vx
        else:
            self.bx = tx
        ty = self.by + self.vy
        if self.vy > 0 and ty + 1 == 78 and self.bx + 1 >= self.px and self.bx <= self.px + w - 1:
            seg = self._segment(self.bx, self.px, w)
            self.vy, self.vx = -1, (-2, -1, 1, 2)[seg]
            self.events.add("paddle_%d" % seg)
            return c.return_reward, 0, False
        if self.vy < 0 and ty == 9 and self.bx + 1 >= self.ox and self.bx <= self.ox + w - 1:
            seg = self._segment(self.bx, self.ox, w)
            self.vy, self.vx = 1, (-2, -1, 1, 2)[seg]
            self.events.add("opp_%d" % seg)
            return 0, c.return_reward, False
        if ty + 1 > 83:                                      # a point for seat 1
            self.theirs += 1
            self.totals[1] += 1
            if self.theirs == c.points:
                self.other_matches += 1
            self.wait = 0
            self.events.add("point_lost")
            return c.lose_reward, c.win_reward, True
        if ty < 6:                                           # a point for seat 0
            self.mine += 1
            self.totals[0] += 1
            if self.mine == c.points:
                self.totals[2] += 1
            self.wait = 0
            self.events.add("point_won")
            return c.win_reward, c.lose_reward, True
        self.by = ty
        return 0, 0, False

    def tick(self, a0, a1):
        """One tick: seat 0's paddle, seat 1's paddle, the serve or the ball -> (r0, r1)."""
        c = self.c
        hi = 82 - c.paddle_width
        if a0 == RIGHT:
            self.px = min(self.px + c.paddle_speed, hi)
        elif a0 == LEFT:
            self.px = max(self.px - c.paddle_speed, 2)
        if a1 == RIGHT:
            self.ox = min(self.ox + c.paddle_speed, hi)
        elif a1 == LEFT:
            self.ox = max(self.ox - c.paddle_speed, 2)
        r0 = r1 = 0
        if self.wait >= 0:
            if a0 == FIRE or a1 == FIRE or (c.serve_wait > 0 and self.wait >= c.serve_wait):
                self.events.add("serve_fire0" if a0 == FIRE else "serve_fire1" if a1 == FIRE else "serve_auto")
                self._serve()                                # keyed by self.g = seat 0's global index
            else:
                self.wait += 1
        else:
            for _ in range(c.ball_speed):
                d0, d1, point = self._micro_step2()
                r0 += d0
                r1 += d1
                if point:
                    break
        return r0, r1

    def ended(self):
        return self.mine >= self.c.points or self.theirs >= self.c.points

    def step(self, a0, a1):
        """One agent step, without the reset -> (r0, r1, terminal).  events: HostDuel's, with serve_fire0 / serve_fire1
        for the seat whose fire served (seat 0's when both fire), end_win / end_lose from seat 0's side."""
        c = self.c
        self.events = set()
        self.ep_steps += 1
        r0 = r1 = 0
        for tick in range(c.action_repeat):
            d0, d1 = self.tick(int(a0), int(a1))
            r0 += d0
            r1 += d1
            if self.ended():
                break
        terminal = self.ended() or self.ep_steps >= c.max_episode_steps
        if terminal:
            self.events.add("end_win" if self.mine >= c.points else "end_lose" if self.theirs >= c.points else "end_timeout")
        return r0, r1, terminal


def render_record(conf, rec):
    """HostDuel.render of a 16-word record under the self-play config `conf` (opponent_width = paddle_width)."""
    h = HostDuel.__new__(HostDuel)
    h.c = conf.scripted
    h.px, h.bx, h.by, h.vx, h.vy, h.wait, h.ox, h.mine, h.theirs = [int(v) for v in rec[:9]]
    return h.render()


class HostSeat(object):
    """Global actor g: seat g & 1 of game g >> 1, with HostDuel's interface.  `partner`: the partner's actions, one per
    process() call, consumed from the front (None: the partner always plays noop)."""

    def __init__(self, conf, g=0, seed=0, frames=True, partner=None):
        self.conf, self.c, self.g, self.seat, self.frames = conf, conf.scripted, int(g), int(g) & 1, frames
        self.partner = partner
        self.game = TwoSeatDuel(conf, int(g) & ~1, seed)     # its constructor resets once (episode 0)
        self.events = set()
        self.success = False
        self.frame = self.last_state = None
        self.last_action, self.last_reward = 0, 0
        self._view()

    ep_steps = property(lambda self: self.game.ep_steps)
    episode = property(lambda self: self.game.episode)

    def record(self):
        rec = self.game.record()
        return mirror(rec) if self.seat else rec

    @property
    def totals(self):
        return [int(v) for v in self.record()[10:13]]

    def _view(self):
        if self.frames:
            self.frame = render_record(self.conf, self.record())
            self.last_state = {'image': self.frame / 255.0}

    def reset(self):
        self.game.reset()
        self.last_action, self.last_reward = 0, 0
        self._view()

    def process(self, action, flag=0):
        a = int(action)
        ap = NOOP if self.partner is None else int(self.partner.pop(0))
        r0, r1, terminal = self.game.step(ap if self.seat else a, a if self.seat else ap)
        reward = r1 if self.seat else r0
        self.events = self.game.events
        rec = self.record()
        self.success = bool(terminal and rec[7] >= self.c.points)
        pc = None
        if self.frames:
            old = self.frame
            self._view()
            pc = pixel_change(self.frame, old)
        self.last_action, self.last_reward = a, reward
        return self.last_state, reward, terminal, pc

    def stop(self):
        pass


def host_batch(conf, B, seed, actor_base=0, frames=True, scripts=None):
    """The seats [actor_base, actor_base + B) of a device environment with key `seed`; scripts[b]: seat b's partner list."""
    return [HostSeat(conf, actor_base + b, seed, frames=frames, partner=None if scripts is None else scripts[b])
            for b in range(B)]


def step_pairs(seats, acts, active=None):
    """One plain step of a whole environment of HostSeats (scripts filled here): a pair steps when both seats are active;
    a terminal resets.  -> (rewards, terminals, pixel changes, stepped) per seat (None where idle)."""
    B = len(seats)
    out = [(None, None, None, False)] * B
    for i in range(0, B, 2):
        if active is not None and not (active[i] and active[i + 1]):
            continue
        for b in (i, i + 1):
            seats[b].partner = [int(acts[b ^ 1])]
            _, r, t, pc = seats[b].process(acts[b])
            out[b] = (r, t, pc, True)
    return out


# ---- the traces the GPU test compares step by step; tests/test_selfplay_cpu.py checks on this model alone that they hold
# every event ---------------------------------------------------------------------------------------------------------------
TRACE_B, TRACE_STEPS, TRACE_PAIR_FRAMES = 64, 300, 3        # actors, steps, pairs whose frames and pixel change are compared
TRACE_SEED = 1
TRACE_SETTINGS = [dict(),
                  dict(points=2, paddle_width=4, ball_speed=4, win_reward=7, lose_reward=-3, return_reward=2,
                       max_episode_steps=60),
                  dict(points=1, paddle_width=24, ball_speed=1, serve_wait=0, max_episode_steps=150),
                  dict(points=9, paddle_width=24, paddle_speed=8, ball_speed=3, action_repeat=3)]
EVERY_EVENT = {"wall_left", "wall_right", "paddle_0", "paddle_1", "paddle_2", "paddle_3", "opp_0", "opp_1", "opp_2", "opp_3",
               "point_won", "point_lost", "serve_fire0", "serve_fire1", "serve_auto", "end_win", "end_lose", "end_timeout"}


def trace_inputs(k):
    """Actions and active flags of random trace k -> int32 [TRACE_STEPS, TRACE_B] each (duel_model.trace_inputs' draw)."""
    rs = np.random.RandomState(100 * k + 1)
    acts = rs.randint(0, 4, (TRACE_STEPS, TRACE_B)).astype(np.int32)
    active = (rs.rand(TRACE_STEPS, TRACE_B) < 0.9).astype(np.int32)
    return acts, active
