"""Evaluation harness, after /root/reference/evaluate.py:92-169, 250-275: run the policy of a
(restored) network WITHOUT learning for a number of episodes and report return / success statistics.  The
reference evaluates one MINOS episode at a time with batch-1 session calls; here B maze actors roll in
lock-step on the device with the same kernels the trainer uses (policy sampled like `choose_action`, or
greedy).  With `simulator=` the actors are host-fed indoor (MINOS-contract) simulators instead, at the network's
image_shape (main.py:196), rewards divided by termination_time.  The maze has no step limit (maze_environment.py:114-118), so `max_episode_steps` bounds an episode;
such episodes count as failures ("success := terminal").  With `maze=` (a name given to
Environment.register_maze_config) the actors run that configured maze: success is reaching the goal (terminal with reward
+1), and a time-out is the environment's own (its max_episode_steps); `max_episode_steps` here bounds episodes only when
the config sets no limit.  On a navigation maze success is an episode with at least one goal, read from the
per-actor goals_total / apples_total counters; with goal_respawn an episode ends only at its time-out.  On a goal-sense
maze without goal_respawn the result also holds `start_distance`, the mean path distance d0 from start to
goal of the counted episodes, and `spl`, the mean of success * d0 / max(d0, episode length in steps): every action is a
step, turns and looks included, so an agent on the shortest path scores d0 / (d0 + its turns).  On a forage maze
 the result also holds `pickups_per_episode`, the mean number of collected pickups of kinds A, B, C, D, and on a
no_goal maze success is an episode whose final step collected an ends_episode kind with a reward > 0.  With `arcade=` (a
name given to Environment.register_arcade_config) the actors play that game: success is a cleared wall, every
other ending (last life, the config's max_episode_steps) counts under `timeouts`, and the result holds
`bricks_per_episode` and `lives_lost_per_episode` from differences of the records' running totals.  On the duel
 success is a match won, `timeouts` counts the episodes that ended at the step limit, `losses` those the opponent
won, and the differences of the totals are `points_won_per_episode` and `points_lost_per_episode`.  On invaders
 success is a cleared wave, every other ending (last life, invasion, step limit) counts under `timeouts`, and the
differences are `aliens_per_episode` and `lives_lost_per_episode` (an invasion counts the lives that were left).  On
crossing success is the config's `crossings` reached, every other ending counts under `timeouts`, and the
differences are `crossings_per_episode` and `hits_per_episode`.  On every game
`mean_length` counts agent steps: with the config's `action_repeat = k` an episode of that length ran up to k
game ticks per step.  With `arcade=` the name of a game mixture (Environment.register_arcade_mix) actor b plays
task b mod K; the result keeps the overall keys over all counted episodes (`timeouts`: the sum of the tasks') and adds
`tasks`, one dict per task with the keys and meanings of a single-game evaluation of that task's game, over the episodes of
that task's actors (the duel's `losses` by the task's own `points`).  With `arcade=` the name of a self-play game
(Environment.register_arcade_selfplay) the network plays seat 0 against the scripted opponent: exactly the
evaluation of the duel config `.scripted`, the transfer metric of a self-play run.  `versus=other_network` (a self-play name
only) plays the two networks head to head on the self-play kernels instead: B / 2 games, in game i `network` sits in seat
i mod 2 and `other_network` in the other; both networks are evaluated on every row with LSTM states of their own, and a
fixed per-row mask picks each row's action.  The result holds the duel's keys from `network`'s side, one episode per game,
and `versus=True`."""
import torch

from . import ops
from .environment.maze_environment import batched_maze_environment
from .model.model import PathWS
from .train.trainer import PhiloxDraws


class Evaluate(object):
    def __init__(self, network, batch_size=64, device="cuda:0", seed=0xE7A1, greedy=False, draws=None, simulator=None,
                 termination_time=50.0, maze=None, arcade=None, versus=None):
        self.net, self.B, self.greedy = network, int(batch_size), greedy
        self.versus = versus
        if versus is not None:
            from .environment.environment import Environment
            if simulator is not None or arcade is None or \
                    getattr(Environment.arcade_config(arcade), "game", None) != "selfplay":
                raise ValueError("versus needs arcade= the name of a self-play game (Environment.register_arcade_selfplay)")
            if self.B % 2:
                raise ValueError("versus plays batch_size / 2 games: batch_size = %d must be even" % self.B)
        self.device = torch.device(device)
        self.draws = draws if draws is not None else PhiloxDraws(seed)
        B, A = self.B, network._action_size
        self.maze_config = None
        self.arcade_config = None
        if simulator is None and arcade is not None:
            from .environment.environment import Environment
            from .environment.arcade_environment import BatchedArcadeEnvironment
            self.arcade_config = Environment.arcade_config(arcade)
            if self.arcade_config.game == "selfplay" and versus is None:
                self.arcade_config = self.arcade_config.scripted      # seat 0 against the scripted opponent
            self.env = BatchedArcadeEnvironment(B, 2, self.device, config=self.arcade_config, seed=seed)
            network.lar_bounded = False        # a step can pay more than 1 (Trainer.prepare)
        elif simulator is None:
            if maze is not None:
                from .environment.environment import Environment
                if maze not in Environment.MAZE_CONFIG:
                    raise KeyError("maze %r: call Environment.register_maze_config(name, layouts, ...) first" % maze)
                self.maze_config = Environment.MAZE_CONFIG[maze]
            self.env = batched_maze_environment(B, 2, self.device, config=self.maze_config, seed=seed)
            if self.env.ring.objective_size != network._objective_size:
                raise ValueError("the network's objective_size %d differs from the maze's %d"
                                 % (network._objective_size, self.env.ring.objective_size))
            if self.maze_config is not None and self.maze_config.reward_bound > 1:
                network.lar_bounded = False    # raw navigation rewards in the LSTM input (Trainer.prepare)
        else:
            from .environment.hostfed_environment import HostFedEnvironment
            if tuple(getattr(simulator, "image_shape", (84, 84))) != tuple(network.image_shape):
                raise ValueError("simulator.image_shape %r != the network's image_shape %r"
                                 % (getattr(simulator, "image_shape", (84, 84)), network.image_shape))
            self.env = HostFedEnvironment(simulator, B, 2, self.device, action_size=A, clip_reward=False,
                                          objective_size=network._objective_size, reward_divisor=termination_time,
                                          frame_shape=network.image_shape)
            network.lar_bounded = False        # raw rewards and measurement vectors in the LSTM input (Trainer.prepare)
        network.bind_frame_scale(self.env.frame_scale)
        self.ws = PathWS(B, B, self.device, save_c1=False, lstm=network._use_lstm, xld=network.xld, **network.ws_kw)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=self.device)
        self.pi, self.v = z(B * A, torch.float32), z(B, torch.float32)
        self.u, self.actions = z(B, torch.float64), z(B, torch.int32)
        self.rewards, self.terminals = z(B, torch.float32), z(B, torch.int32)
        if versus is not None:                 # the other network: its own workspace (LSTM state), outputs and actions
            if versus._action_size != A:
                raise ValueError("versus: the other network has %d actions, not %d" % (versus._action_size, A))
            versus.lar_bounded = False
            versus.bind_frame_scale(self.env.frame_scale)
            self.ws2 = PathWS(B, B, self.device, save_c1=False, lstm=versus._use_lstm, xld=versus.xld, **versus.ws_kw)
            self.pi2, self.v2, self.actions2 = z(B * A, torch.float32), z(B, torch.float32), z(B, torch.int32)
            self.played = z(B, torch.int32)
            b = torch.arange(B, device=self.device)
            self.mine = (b % 2) == ((b // 2) % 2)              # rows in which `network` sits: seat i mod 2 of game i

    def _policy(self, net, ws, pi, v, actions):
        """`net`'s policy on all B rows of the environment's current observations -> actions."""
        B, ring = self.B, self.env.ring
        net.begin_pass()
        ring.cur_idx(out=ws.frame_idx[:B])
        net.encode_rows(ring, ws, 0, B, lar_from_ring=False, save_c1=False, lstm_x=False)
        if net._use_lstm:
            net.lstm_step(ws, 0, B, fused_x=True)
        feat, ld = net.features(ws, 0)
        net.policy_step(B, feat, ld, None if self.greedy else self.u, pi, v, actions)

    def _step_versus(self):
        """One lock-step step of the B / 2 games: both networks on all rows (one draw per row serves both), the row's own
        network's action by the mask, the self-play step, then each network's LSTM state carried on its own."""
        B = self.B
        if not self.greedy:
            self.draws.uniform(self.u)
        self._policy(self.net, self.ws, self.pi, self.v, self.actions)
        self._policy(self.versus, self.ws2, self.pi2, self.v2, self.actions2)
        self.played.copy_(torch.where(self.mine, self.actions, self.actions2))
        self.env.process(self.played, None, self.rewards, self.terminals, reset_on_terminal=True, track_score=True)
        for net, ws in ((self.net, self.ws), (self.versus, self.ws2)):
            if net._use_lstm:
                ops.copy_(ws.c0, ws.c[:B * 256])
                ops.copy_(ws.h0, ws.h[:B * 256])
                ops.reset_state(B, self.terminals, ws.c0, ws.h0)

    def _step(self):
        """One lock-step policy + environment step of the B actors (reset on terminal, scores tracked)."""
        B, net, ws, ring = self.B, self.net, self.ws, self.env.ring
        net.begin_pass()
        ring.cur_idx(out=ws.frame_idx[:B])
        net.encode_rows(ring, ws, 0, B, lar_from_ring=False, save_c1=False, lstm_x=False)
        if net._use_lstm:
            net.lstm_step(ws, 0, B, fused_x=True)
        feat, ld = net.features(ws, 0)
        if not self.greedy:
            self.draws.uniform(self.u)
        net.policy_step(B, feat, ld, None if self.greedy else self.u, self.pi, self.v, self.actions)
        self.env.process(self.actions, None, self.rewards, self.terminals, reset_on_terminal=True,
                         track_score=True)
        if net._use_lstm:                      # carry the state; zero it where the episode ended
            ops.copy_(ws.c0, ws.c[:B * 256])
            ops.copy_(ws.h0, ws.h[:B * 256])
            ops.reset_state(B, self.terminals, ws.c0, ws.h0)

    @staticmethod
    def _arcade_result(conf, eps):
        """The statistics of one game's counted episodes `eps`: (return, length, first total's gain, second total's gain,
        won), in the order they ended."""
        n = len(eps)
        returns = [e[0] for e in eps]
        bricks, lost = [e[2] for e in eps], [e[3] for e in eps]
        successes = sum(int(e[4]) for e in eps)
        mean = sum(returns) / n
        res = dict(episodes=n, success_rate=successes / float(n), mean_return=mean,
                   return_std=(sum((r - mean) ** 2 for r in returns) / n) ** 0.5,
                   mean_length=sum(e[1] for e in eps) / float(n))
        if conf.game == "duel":
            # an episode starts at 0 : 0, so the opponent's score is the episode's points lost
            losses = sum(int(not e[4] and e[3] >= conf.points) for e in eps)
            res.update(timeouts=n - successes - losses, losses=losses, points_won_per_episode=sum(bricks) / float(n),
                       points_lost_per_episode=sum(lost) / float(n))
        elif conf.game == "crossing":
            res.update(timeouts=n - successes, crossings_per_episode=sum(bricks) / float(n),
                       hits_per_episode=sum(lost) / float(n))
        elif conf.game == "invaders":
            res.update(timeouts=n - successes, aliens_per_episode=sum(bricks) / float(n),
                       lives_lost_per_episode=sum(lost) / float(n))
        else:
            res.update(timeouts=n - successes, bricks_per_episode=sum(bricks) / float(n),
                       lives_lost_per_episode=sum(lost) / float(n))
        return res

    def _process_versus(self, n_episodes, one_episode_per_actor):
        """Head to head: one episode per game, counted on `network`'s row of the pair, whose record holds its
        own points won (word 10), points lost (11) and matches won (12)."""
        B, ring = self.B, self.env.ring
        rows = [b for b in range(B) if (b % 2) == ((b // 2) % 2)]
        tot = ring.actor_records[:, 10:13]
        ep0 = tot.cpu().numpy().copy()
        steps, counted = [0] * B, [False] * B
        eps = []
        if one_episode_per_actor:
            n_episodes = len(rows)
        while len(eps) < n_episodes:
            self._step_versus()
            term = self.terminals.cpu().numpy()
            score = ring.score_out.cpu().numpy()
            now = tot.cpu().numpy()
            for b in rows:
                steps[b] += 1
                if not term[b]:
                    continue
                if not (one_episode_per_actor and counted[b]):
                    eps.append((float(score[b]), steps[b], int(now[b, 0] - ep0[b, 0]), int(now[b, 1] - ep0[b, 1]),
                                bool(now[b, 2] - ep0[b, 2] > 0)))
                ep0[b] = now[b]
                steps[b] = 0; counted[b] = True
        res = self._arcade_result(self.arcade_config.scripted, eps)
        res["versus"] = True
        return res

    def _process_arcade(self, n_episodes, one_episode_per_actor):
        """The arcade's statistics: every episode ends in the environment (lives, wall or points, max_episode_steps).  A
        game mixture: the overall keys over every counted episode, and `tasks`: per task, what a single-game
        evaluation of its game returns, over the episodes of the task's actors."""
        B, ring = self.B, self.env.ring
        # Breakout: bricks, lives lost, walls cleared; duel: points won, points lost, matches won; invaders: aliens shot,
        # lives lost, waves cleared; crossing: crossings, hits, targets reached.  Never zeroed.
        tot = ring.actor_records[:, 10:13]
        ep0 = tot.cpu().numpy().copy()
        steps, counted = [0] * B, [False] * B
        eps, task_of_ep = [], []
        task = self.env.task_of_actor()
        if one_episode_per_actor:
            n_episodes = B
        while len(eps) < n_episodes:
            self._step()
            term = self.terminals.cpu().numpy()
            score = ring.score_out.cpu().numpy()
            now = tot.cpu().numpy()
            for b in range(B):
                steps[b] += 1
                if not term[b]:
                    continue
                if not (one_episode_per_actor and counted[b]):
                    eps.append((float(score[b]), steps[b], int(now[b, 0] - ep0[b, 0]), int(now[b, 1] - ep0[b, 1]),
                                bool(now[b, 2] - ep0[b, 2] > 0)))
                    task_of_ep.append(int(task[b]))
                ep0[b] = now[b]
                steps[b] = 0; counted[b] = True
        if self.arcade_config.game != "mix":
            return self._arcade_result(self.arcade_config, eps)
        tasks = []
        for k, conf in enumerate(self.arcade_config.tasks):
            own = [e for e, t in zip(eps, task_of_ep) if t == k]
            tasks.append(self._arcade_result(conf, own) if own else dict(episodes=0))   # (no episode: nothing to average)
        n = len(eps)
        returns = [e[0] for e in eps]
        mean = sum(returns) / n
        return dict(episodes=n, success_rate=sum(int(e[4]) for e in eps) / float(n), mean_return=mean,
                    return_std=(sum((r - mean) ** 2 for r in returns) / n) ** 0.5,
                    mean_length=sum(e[1] for e in eps) / float(n), timeouts=sum(t.get("timeouts", 0) for t in tasks), tasks=tasks)

    def process(self, n_episodes, max_episode_steps=2000, one_episode_per_actor=False):
        """-> dict(episodes, success_rate, mean_return, return_std, mean_length, timeouts, goals_per_episode,
        apples_per_episode[, start_distance, spl][, pickups_per_episode]).
        On a forage maze `pickups_per_episode` holds the mean number of collected pickups of kinds A, B, C, D
        per counted episode (differences of record words 4..7); on a no_goal maze success is an episode whose final step
        collected an ends_episode kind with a reward > 0, read from those totals before and after that step.
        `one_episode_per_actor`: count only the FIRST episode of each of the B lock-step actors and stop when all B have
        finished or timed out (n_episodes is ignored).  Stopping at the first n finished episodes instead over-represents
        short episodes whenever actors restart while others are still in their first one."""
        B, A, net, ws, ring = self.B, self.net._action_size, self.net, self.ws, self.env.ring
        net.refresh_shadows()
        self.env.reset()
        ring.episode_reward.zero_()
        if net._use_lstm:
            ws.c0.zero_()
            ws.h0.zero_()
        if self.versus is not None:
            self.versus.refresh_shadows()
            if self.versus._use_lstm:
                self.ws2.c0.zero_()
                self.ws2.h0.zero_()
            return self._process_versus(n_episodes, one_episode_per_actor)
        if self.arcade_config is not None:
            return self._process_arcade(n_episodes, one_episode_per_actor)
        steps = [0] * B
        done, returns, lengths, successes, timeouts = 0, [], [], 0, 0
        cfg = self.maze_config
        env_limit = cfg is not None and cfg.max_episode_steps > 0       # episodes end in the environment
        configured = cfg is not None
        nav = cfg is not None and cfg.nav
        counted = [False] * B
        goals, apples = [], []                 # per counted episode
        if nav:                                # goals_total / apples_total (never zeroed by a reset): per-episode differences
            forage = cfg.forage
            tot = ring.actor_records[:, 3:8] if forage else ring.actor_records[:, 3:5]
            ep0 = tot.cpu().numpy().copy()
            before = ep0.copy()                # forage: the totals before the step
            kinds = []                         # per counted episode: collected A, B, C, D
            winning = [k for k, (r, _, ends) in enumerate(cfg.pickups or (), 1) if ends and r > 0]
        # goal sense: path efficiency.  d0 = word 7 of the actor's record after the reset that started the episode
        sense = cfg is not None and cfg.goal_sense and not cfg.goal_respawn
        start_d, spl = [], []
        if sense:
            d0 = ring.actor_records[:, 7].cpu().numpy().copy()
        if one_episode_per_actor:
            n_episodes = B
        while done < n_episodes:
            self._step()
            term = self.terminals.cpu().numpy()
            rew = self.rewards.cpu().numpy()
            score = ring.score_out.cpu().numpy()
            now = tot.cpu().numpy() if nav else None
            d_now = ring.actor_records[:, 7].cpu().numpy() if sense else None
            force = torch.zeros(B, dtype=torch.int32)
            ep_r = None
            for b in range(B):
                steps[b] += 1
                skip = one_episode_per_actor and counted[b]
                ended = bool(term[b]) or (not env_limit and steps[b] >= max_episode_steps)
                if ended and not skip:
                    n_goals = int(now[b, 0] - ep0[b, 0]) if nav else int(bool(term[b]) and rew[b] == 1.0)
                    goals.append(n_goals)
                    apples.append(int(now[b, 1] - ep0[b, 1]) if nav else 0)
                    if nav and forage:
                        kinds.append([int(v) for v in now[b, 1:5] - ep0[b, 1:5]])
                if ended and nav:
                    ep0[b] = now[b]
                if term[b]:
                    if not skip:
                        returns.append(float(score[b])); lengths.append(steps[b]); done += 1
                        success = not configured or (goals[-1] > 0 if nav else rew[b] == 1.0)
                        if nav and cfg.no_goal:        # the final step collected a winning kind
                            success = any(now[b, 1 + k] > before[b, 1 + k] for k in winning)
                        if success:
                            successes += 1
                        else:
                            timeouts += 1              # the configured maze's own time-out
                        if sense:
                            start_d.append(int(d0[b]))
                            spl.append(d0[b] / float(max(d0[b], steps[b])) if success else 0.0)
                    if sense:
                        d0[b] = d_now[b]               # the step's own reset has started the next episode
                    steps[b] = 0; counted[b] = True
                elif not env_limit and steps[b] >= max_episode_steps:
                    if ep_r is None:
                        ep_r = ring.episode_reward.cpu()
                    if not skip:
                        timeouts += 1; done += 1
                        returns.append(float(ep_r[b])); lengths.append(max_episode_steps)
                        if sense:
                            start_d.append(int(d0[b])); spl.append(0.0)
                    steps[b] = 0; force[b] = 1; counted[b] = True
            if nav and forage:
                before = now.copy()
            if int(force.sum()):                   # abandon timed-out episodes
                m = force.to(self.device)
                self.env.reset(m)
                ring.episode_reward.mul_((1 - m).to(torch.float32))
                if sense:
                    forced = force.numpy().astype(bool)                    # (running episodes keep theirs)
                    d0[forced] = ring.actor_records[:, 7].cpu().numpy()[forced]
                if net._use_lstm:
                    ops.reset_state(B, m, ws.c0, ws.h0)
        n = len(returns)
        mean = sum(returns) / n
        res = dict(episodes=n, success_rate=successes / float(n), mean_return=mean,
                   return_std=(sum((r - mean) ** 2 for r in returns) / n) ** 0.5,
                   mean_length=sum(lengths) / float(n), timeouts=timeouts, goals_per_episode=sum(goals) / float(n),
                   apples_per_episode=sum(apples) / float(n))
        if sense:
            res.update(start_distance=sum(start_d) / float(n), spl=sum(spl) / float(n))
        if nav and forage:
            res.update(pickups_per_episode=[sum(k[i] for k in kinds) / float(n) for i in range(4)])
        return res
