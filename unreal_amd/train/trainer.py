"""Batched actor-learner: `Trainer.process()` for B maze actors per GPU on gfx950 kernels.

Mirrors /root/reference/train/trainer.py: ctor 31-128, prepare 132-135, stop 137-138,
_anneal_learning_rate 140-144, choose_action 147-148, set_start_time 172-173,
_fill_experience 176-205, _process_base 218-336, _process_pc 339-380, _process_vr 383-412,
_process_rp 415-436, process 438-636.

What changes, and only this: the reference runs `parallel_size` Python threads, each
rolling ONE environment with batch-1 session calls and applying its own clipped gradient to shared
RMSProp slots.  Here ONE call advances all B actors of this GPU by <= n_step_TD steps in lock-step
(an actor whose episode ends stops for the rest of the call, exactly like the reference's `break`),
samples B pixel-control / value-replay / reward-prediction batches from the device ring, and makes
one update with the MEAN over actors of the reference's per-actor gradient (sums over time), one
global-norm clip and one RMSProp step.  With B == 1 this is the reference algorithm; staleness is 0.
The rollout's activations are kept in HBM and reused by the backward pass (the reference recomputes
the same forward with the same synced weights, trainer.py:457,543-570).

`groups=G` restores update density on the batched path: the B actors of the GPU are dealt into G groups of B/G and
one process() call runs G complete actor-learner passes one after the other -- group g rolls out with the weights
group g-1 has just updated, its mean gradient is clipped and applied by itself (G RMSProp steps per call).  G = 1 is
the lock-step learner above; G = B is the reference's algorithm executed actor after actor (zero staleness, the
order in which hogwild threads would take the lock if there were one).

Per-actor random draws come from a counter RNG (Philox) on the device; `draws` can be replaced to
replay a recorded stream (parity tests).  TF-only arguments are accepted and ignored.

How the schedule is laid out.  `_rollout` = prologue, exactly one of four step schedules (`_rollout_steps_device` /
`_rollout_steps_host` in lock-step, `_rollout_steps_overlapped` / `_rollout_steps_split` as half-batches on two streams),
`_rollout_bootstrap`, `_rollout_returns`; every schedule forwards rows [t B + b0, t B + b0 + n) through the one body
`_policy_step`, reads the rows' buffers through `_block` and tells a device environment what to prepare of step t + 1
through `_next_rows`.  The loss branches of an update (`_train_base`, `_train_replay`, `_train_rp`) take the `PassState` they
work on explicitly: the trainer itself, or the minibatch twin `self.mb`.  Pixel control and value replay are lanes of ONE
replay pass, `_train_replay(c, lanes)`: ("pc", "vr") by default, one lane per pass otherwise; a width's workspaces come from
`_replay_set` and are never written in c0 / h0.
"""
import time
from types import SimpleNamespace

import torch

from .. import ops
from ..environment.environment import Environment
from ..environment.maze_environment import batched_maze_environment
from ..model.model import UnrealModel, PathWS, GradWS
from .experience import Experience

PERFORMANCE_LOG_INTERVAL = 2000


def log_uniform(lo, hi, rate):
    """Initial learning rate (main.py:61-65): exp((1-rate) log lo + rate log hi) = 7.0711e-4 by default."""
    import math
    return math.exp(math.log(lo) * (1 - rate) + math.log(hi) * rate)


class PhiloxDraws(object):
    """Device draws; every call consumes a fresh Philox stream id.  Every rank makes the same sequence of calls and
    reads its own actors' columns [rank*B, (rank+1)*B) of the call's global draw, so the trajectories of a job do not
    depend on how many GPUs its actors are sharded over (batch=None: a plain stream, single process)."""

    def __init__(self, seed, rank=0, batch=None, world_size=1):
        self.seed = int(seed)
        self.counter = 1
        self.batch = None if batch is None else int(batch)
        self.stride = None if batch is None else int(batch) * int(world_size)
        self.col0 = 0 if batch is None else int(rank) * int(batch)

    def _next(self):
        self.counter += 1
        return self.counter

    def uniform(self, out):
        ops.philox_uniform(self.seed, self._next(), out, self.batch, self.stride, self.col0)
        return out

    def randint(self, high, out):
        ops.philox_randint(self.seed, self._next(), high, out, self.batch, self.stride, self.col0)
        return out


class PassState(object):
    """What the loss branches of ONE update read and write, sized for `Bg` actors: the path and gradient workspaces, the
    replay samples' buffers, the heads' outputs and gradients, the ring the replay branches sample (`ring`) and the ring the
    base rows' frame indices point into (`base_ring`).  The Trainer is its own for a whole group; with reuse_minibatches > 1
    a second one, sized for a block of the group's actors, also holds the block's compacted rollout rows.
    The Trainer's pass methods take theirs as the argument `c`."""


class Trainer(PassState):
    @staticmethod
    def check_rollout_options(env_type, env_name, bootstrap_timeouts, gae_lambda):
        """-> (bootstrap_timeouts, gae_lambda) as the trainer keeps them; ValueError for what is out of scope: gae_lambda
        outside [0, 1]; bootstrap_timeouts on anything but the device arcade and first-person device mazes without
        goal_sense (top-down and goal-sense mazes keep no final observation, host-fed environments own their resets)."""
        if gae_lambda is not None:
            if isinstance(gae_lambda, bool) or not isinstance(gae_lambda, (int, float)) or not 0.0 <= gae_lambda <= 1.0:
                raise ValueError("gae_lambda = %r: a number in [0, 1], or None for the n-step return" % (gae_lambda,))
            gae_lambda = float(gae_lambda)
        if bootstrap_timeouts:
            if env_type == "maze":
                from ..environment.maze_environment import check_final_obs
                check_final_obs(Environment.MAZE_CONFIG.get(env_name))
            elif env_type != "arcade":
                raise ValueError("bootstrap_timeouts is out of scope for host-fed environments (env_type=%r): it needs "
                                 "env_type 'arcade' or a first-person 'maze' config without goal_sense" % (env_type,))
        return bool(bootstrap_timeouts), gae_lambda

    @staticmethod
    def check_depth_prediction(env_type, env_name, use_depth_prediction, depth_lambda=1.0):
        """-> (use_depth_prediction, depth_lambda) as the trainer keeps them; ValueError for what is out of scope (DESIGN
        §7p): the labels are the wall distances of a first-person device maze, so top-down mazes, the arcade and host-fed
        environments have none; depth_lambda must be a finite number >= 0."""
        if not use_depth_prediction:
            return False, float(depth_lambda)
        if isinstance(depth_lambda, bool) or not isinstance(depth_lambda, (int, float)) or not 0.0 <= depth_lambda < float("inf"):
            raise ValueError("depth_lambda = %r: a finite number >= 0" % (depth_lambda,))
        if env_type == "maze":
            from ..environment.maze_environment import check_depth_labels
            check_depth_labels(Environment.MAZE_CONFIG.get(env_name))
        elif env_type == "arcade":
            raise ValueError("use_depth_prediction is out of scope for the arcade: it needs a first-person 'maze' config")
        else:
            raise ValueError("use_depth_prediction is out of scope for host-fed environments (env_type=%r): it needs a "
                             "first-person 'maze' config" % (env_type,))
        return True, float(depth_lambda)

    REUSE_EPOCHS_MAX = 16

    @staticmethod
    def check_reuse_options(env_type, reuse_epochs, ppo_clip):
        """-> (reuse_epochs, ppo_clip) as the trainer keeps them; ValueError for what is out of scope:
        reuse_epochs must be an int in 1..16 and ppo_clip a finite number with 0 < ppo_clip < 1; more than one update per
        rollout needs a device environment ('maze', 'arcade'), as groups > 1 does."""
        if isinstance(reuse_epochs, bool) or not isinstance(reuse_epochs, int) or \
                not 1 <= reuse_epochs <= Trainer.REUSE_EPOCHS_MAX:
            raise ValueError("reuse_epochs = %r: an int in 1..%d" % (reuse_epochs, Trainer.REUSE_EPOCHS_MAX))
        if isinstance(ppo_clip, bool) or not isinstance(ppo_clip, (int, float)) or not 0.0 < ppo_clip < 1.0:
            raise ValueError("ppo_clip = %r: a number with 0 < ppo_clip < 1" % (ppo_clip,))
        if reuse_epochs > 1 and env_type not in ("maze", "arcade"):
            raise ValueError("reuse_epochs > 1 is out of scope for host-fed environments (env_type=%r): it needs "
                             "env_type 'maze' or 'arcade'" % (env_type,))
        return int(reuse_epochs), float(ppo_clip)

    @staticmethod
    def check_minibatch_options(env_type, batch_size, groups, reuse_minibatches):
        """-> reuse_minibatches as the trainer keeps it; ValueError for what is out of scope: an int >= 1 that
        divides the actors of a group, batch_size // groups; more than one needs a device environment ('maze', 'arcade'),
        as reuse_epochs > 1 does."""
        M = reuse_minibatches
        if isinstance(M, bool) or not isinstance(M, int) or M < 1:
            raise ValueError("reuse_minibatches = %r: an int >= 1" % (M,))
        if M > 1:
            if env_type not in ("maze", "arcade"):
                raise ValueError("reuse_minibatches > 1 is out of scope for host-fed environments (env_type=%r): it needs "
                                 "env_type 'maze' or 'arcade'" % (env_type,))
            B, G = int(batch_size), int(groups)
            if G < 1 or B % G or (B // G) % M:
                raise ValueError("reuse_minibatches = %d must divide the %d // %d actors of a group" % (M, B, G))
        return int(M)

    @staticmethod
    def check_selfplay_options(env_type, env_name, batch_size, groups):
        """-> whether (env_type, env_name) is a self-play game (Environment.register_arcade_selfplay).  Its
        actors 2 i and 2 i + 1 are the seats of one game, so everything stepped at once holds whole pairs: ValueError
        unless this rank's batch_size and a group's batch_size // groups are even.  (The split rollout cuts a group with
        the environment's view(), which refuses an odd bound.)"""
        if env_type != "arcade" or getattr(Environment.arcade_config(env_name), "game", None) != "selfplay":
            return False
        B, G = int(batch_size), int(groups)
        if B % 2 or (G >= 1 and B % G == 0 and (B // G) % 2):
            raise ValueError("self-play actors come in pairs: batch_size = %d per rank and batch_size // groups = %d // %d "
                             "must be even" % (B, B, G))
        return True

    MAX_OPPONENTS = 16

    @staticmethod
    def check_opponent_options(env_type, env_name, batch_size, groups, opponent_pool, opponent_snapshot_every=100):
        """-> (opponent_pool K, opponent_snapshot_every N) as the trainer keeps them.  K = 0: no pool (N is
        still checked).  ValueError for what is out of scope: K no int in 0..16, N no int >= 1; K > 0 on anything but
        env_type 'arcade' with a self-play name (Environment.register_arcade_selfplay; host-fed environments own their
        opponents), or a K that does not divide the batch_size // groups actors of a group."""
        K, N = opponent_pool, opponent_snapshot_every
        if isinstance(K, bool) or not isinstance(K, int) or not 0 <= K <= Trainer.MAX_OPPONENTS:
            raise ValueError("opponent_pool = %r: an int in 0..%d" % (K, Trainer.MAX_OPPONENTS))
        if isinstance(N, bool) or not isinstance(N, int) or N < 1:
            raise ValueError("opponent_snapshot_every = %r: an int >= 1 (optimiser updates)" % (N,))
        if K == 0:
            return 0, N
        if env_type != "arcade" or getattr(Environment.arcade_config(env_name), "game", None) != "selfplay":
            raise ValueError("opponent_pool = %d needs env_type='arcade' with a self-play game (Environment."
                             "register_arcade_selfplay), not %r / %r" % (K, env_type, env_name))
        B, G = int(batch_size), int(groups)
        if G < 1 or B % G or (B // G) % K:
            raise ValueError("opponent_pool = %d must divide the %d // %d actors of a group" % (K, B, G))
        return K, N

    @staticmethod
    def opponent_slots(Bg, K):
        """The pool slot every row of a group plays against -> a list of Bg ints: rows [k Bg / K, (k + 1) Bg / K) play
        slot k.  A function of the index alone, as the mixtures' tasks are.  ValueError unless K in 1..16 divides Bg."""
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= Trainer.MAX_OPPONENTS or Bg < 1 or Bg % K:
            raise ValueError("opponent_pool = %r must be in 1..%d and divide the %d actors of a group"
                             % (K, Trainer.MAX_OPPONENTS, Bg))
        return [b // (Bg // K) for b in range(Bg)]

    @staticmethod
    def opponent_snapshot(K, N, updates, snapshots):
        """The pool's rule at the end of a process() call -> (slot the current weights go into, or None; the new number
        of snapshots).  With u = `updates` applied so far and s = `snapshots` taken: if u // N > s, slot 1 + (s mod (K - 1))
        is overwritten and s becomes u // N (a call that crosses several multiples of N takes one snapshot).  Slot 0 is
        the present self and K = 1 never snapshots."""
        if K < 2 or updates // N <= snapshots:
            return None, snapshots
        return 1 + snapshots % (K - 1), updates // N

    @staticmethod
    def minibatch_order(epoch, M):
        """The blocks of a group's actors in the order epoch `epoch` (1-based) visits them: (i + epoch - 1) mod M."""
        return [(i + epoch - 1) % M for i in range(M)]

    EXPLORE_CELLS = (4, 6, 7, 12, 14, 21)

    @staticmethod
    def check_explore_options(env_type, explore_beta, explore_cell=7, explore_levels=8, explore_bits=22):
        """-> (explore_beta, explore_cell, explore_levels, explore_bits) as the trainer keeps them; ValueError for what is
        out of scope: explore_beta must be a finite number >= 0, explore_cell one of 4, 6, 7, 12, 14, 21 (the
        divisors of 84 with at most 1323 features), explore_levels an int in 2..64, explore_bits an int in 10..26; a bonus
        (explore_beta > 0) needs a device environment ('maze', 'arcade'): the frames are hashed where the rollout left
        them, in the device ring."""
        b = explore_beta
        if isinstance(b, bool) or not isinstance(b, (int, float)) or not 0.0 <= b < float("inf"):
            raise ValueError("explore_beta = %r: a finite number >= 0" % (b,))
        for name, v, ok in (("explore_cell", explore_cell, lambda v: v in Trainer.EXPLORE_CELLS),
                            ("explore_levels", explore_levels, lambda v: 2 <= v <= 64),
                            ("explore_bits", explore_bits, lambda v: 10 <= v <= 26)):
            if isinstance(v, bool) or not isinstance(v, int) or not ok(v):
                raise ValueError("%s = %r: explore_cell one of %r, explore_levels an int in 2..64, explore_bits an int in "
                                 "10..26" % (name, v, Trainer.EXPLORE_CELLS))
        if b > 0 and env_type not in ("maze", "arcade"):
            raise ValueError("explore_beta > 0 is out of scope for host-fed environments (env_type=%r): it needs "
                             "env_type 'maze' or 'arcade'" % (env_type,))
        return float(b), int(explore_cell), int(explore_levels), int(explore_bits)

    @staticmethod
    def check_optim_options(normalize_advantages, adv_norm_eps=1e-8):
        """-> (normalize_advantages, adv_norm_eps) as the trainer keeps them; ValueError for what is out of scope (DESIGN
        §7s): normalize_advantages must be a bool and adv_norm_eps a finite number > 0 (checked even when the option is
        off).  Every environment type may normalise: the statistics are taken over the rollout's own rows."""
        if not isinstance(normalize_advantages, bool):
            raise ValueError("normalize_advantages = %r: a bool" % (normalize_advantages,))
        e = adv_norm_eps
        if isinstance(e, bool) or not isinstance(e, (int, float)) or not 0.0 < e < float("inf"):
            raise ValueError("adv_norm_eps = %r: a finite number > 0" % (e,))
        return normalize_advantages, float(e)

    def __init__(self, thread_index, global_network, initial_learning_rate, learning_rate_input, grad_applier,
                 env_type, env_name, use_lstm, use_pixel_change, use_value_replay, use_reward_prediction,
                 pixel_change_lambda, entropy_beta, local_t_max, n_step_TD, gamma, gamma_pc,
                 experience_history_size, max_global_time_step, device, segnet_param_dict=None,
                 image_shape=(84, 84), is_training=True, n_classes=0, random_state=None, termination_time=50.0,
                 segnet_lambda=1.0, dropout=0.0, batch_size=1, world_size=1, rank=0, seed=0xA3C, draws=None,
                 grad_sync=None, simulator=None, groups=1, overlap_host=None, bootstrap_timeouts=False, gae_lambda=None,
                 use_depth_prediction=False, depth_lambda=1.0, reuse_epochs=1, ppo_clip=0.2, explore_beta=0.0,
                 explore_cell=7, explore_levels=8, explore_bits=22, normalize_advantages=False, adv_norm_eps=1e-8,
                 reuse_minibatches=1, opponent_pool=0, opponent_snapshot_every=100):
        # opponent pool, off by default: every game has one learner, the other paddle is played by one of
        # opponent_pool frozen copies of the network, refreshed every opponent_snapshot_every updates
        self.opponent_pool, self.opponent_snapshot_every = self.check_opponent_options(
            env_type, env_name, batch_size, groups, opponent_pool, opponent_snapshot_every)
        # minibatched reuse epochs, off by default: a rollout is consumed as reuse_epochs * reuse_minibatches
        # clipped-surrogate updates, each on one block of the group's actors
        self.reuse_minibatches = self.check_minibatch_options(env_type, batch_size, groups, reuse_minibatches)
        # advantage normalisation, off by default: the policy loss of every update of a rollout reads
        # (adv - mean) / (std + eps) over the rollout's active rows; self.adv, self.R and the value loss stay raw
        self.normalize_advantages, self.adv_norm_eps = self.check_optim_options(normalize_advantages, adv_norm_eps)
        # exploration bonus, off by default: explore_beta / sqrt(count of the next frame's code) joins the
        # reward of the base returns and of value replay
        self.explore_beta, self.explore_cell, self.explore_levels, self.explore_bits = self.check_explore_options(
            env_type, explore_beta, explore_cell, explore_levels, explore_bits)
        # sample reuse, off by default: reuse_epochs updates per rollout, the later ones clipped-surrogate
        # (PPO) steps on the same rows against the rollout's policy
        self.reuse_epochs, self.ppo_clip = self.check_reuse_options(env_type, reuse_epochs, ppo_clip)
        # rollout options, both off by default: an episode cut off at max_episode_steps bootstraps from
        # V(final observation) instead of 0; GAE(lambda) replaces the n-step return
        self.bootstrap_timeouts, self.gae_lambda = self.check_rollout_options(env_type, env_name, bootstrap_timeouts,
                                                                              gae_lambda)
        # depth prediction, off by default: one more head on the base features, trained on the rollout rows
        self.use_depth_prediction, self.depth_lambda = self.check_depth_prediction(env_type, env_name,
                                                                                   use_depth_prediction, depth_lambda)
        if self.use_depth_prediction != bool(getattr(global_network, "_use_depth_prediction", False)):
            raise ValueError("Trainer(use_depth_prediction=%r) but the network was built with use_depth_prediction=%r"
                             % (self.use_depth_prediction, getattr(global_network, "_use_depth_prediction", False)))
        # device environments: stepped and rendered by kernels (no simulator, sub-ranges of actors, fused rollout step)
        self.device_env = env_type in ("maze", "arcade")
        if not self.device_env and simulator is None:
            raise NotImplementedError("env_type=%r needs a host simulator object (simulator=...); only 'maze' and "
                                      "'arcade' run entirely on the device" % env_type)
        self.simulator = simulator
        # host-fed actors: alternate two half-batches between the host (simulators, staging) and the device.  None = on
        # from 2048 actors: measured with a cost-free simulator the halves win 1.22x at 4096 actors (654 k vs 537 k
        # env-steps/s) and lose 0.85x at 1024 (the device phase of a step is then too short to be worth twice the
        # launches); with a simulator that dominates the step the two schedules are within 5 %
        self._overlap_request = overlap_host
        # upstream replay semantics for host-fed (Lab-contract) actors: zero / non-zero reward buckets and reward
        # clipping (train/experience_lab_ver.py:14,18,76-80); this fork's buckets for the maze (train/experience.py)
        self.rp_mode = 1 if env_type == "lab" else 0      # indoor, gym: this fork's train/experience.py, like the maze
        self.thread_index = thread_index
        self.learning_rate_input = learning_rate_input
        self.env_type, self.env_name = env_type, env_name
        self.use_lstm = use_lstm
        self.use_pixel_change = use_pixel_change
        self.use_value_replay = use_value_replay
        self.use_reward_prediction = use_reward_prediction
        self.pixel_change_lambda = pixel_change_lambda
        self.entropy_beta = entropy_beta
        self.local_t_max, self.n_step_TD = local_t_max, n_step_TD
        self.gamma, self.gamma_pc = gamma, gamma_pc
        self.experience_history_size = experience_history_size
        self.max_global_time_step = max_global_time_step
        self.action_size = Environment.get_action_size(env_type, env_name)
        self.objective_size = Environment.get_objective_size(env_type, env_name)
        # a goal-sense maze feeds its measurement vector to the LSTM: the network must have its columns
        net_obj = getattr(global_network, "_objective_size", 0)
        if env_type == "maze" and net_obj != self.objective_size:
            raise ValueError("the network's objective_size %d differs from the environment's %d (Environment."
                             "get_objective_size(%r, %r))" % (net_obj, self.objective_size, env_type, env_name))
        # frame size: the network's image_shape must be the environment's (main.py:196 builds both from the MINOS config)
        self.image_shape = tuple(int(x) for x in Environment.get_image_shape(env_type, env_name))
        net_shape = tuple(getattr(global_network, "image_shape", (84, 84)))
        if net_shape != self.image_shape:
            raise ValueError("the network's image_shape %r differs from the environment's %r (Environment.get_image_shape"
                             "(%r, %r))" % (net_shape, self.image_shape, env_type, env_name))
        self.device = torch.device(device if device not in (None, "/gpu:0", "/cpu:0") else "cuda:0")
        self.B = int(batch_size)                     # actors of this rank
        self.groups = int(groups)                    # sequential updates per process() call
        if self.groups < 1 or self.B % self.groups:
            raise ValueError("groups=%d must divide batch_size=%d" % (self.groups, self.B))
        if self.groups > 1 and not self.device_env:
            raise NotImplementedError("groups > 1 needs an environment that steps a sub-range of its actors (maze, "
                                      "arcade)")
        self.Bg = self.B // self.groups              # actors per group = batch of every kernel launch
        # (with a pool every actor is a learner: the pairs' even-count rule does not apply)
        self.selfplay = True if self.opponent_pool else self.check_selfplay_options(env_type, env_name, self.B,
                                                                                    self.groups)
        self.updates = 0                             # optimiser updates applied so far (the pool's clock)
        self.world_size, self.rank = int(world_size), int(rank)
        self.grad_scale = 1.0 / float(self.Bg * self.world_size)
        self.grad_sync = grad_sync
        self.local_network = global_network          # one parameter copy per GPU (sync_from is a no-op)
        self.grad_applier = grad_applier
        self.apply_gradients = grad_applier.minimize_local(None, global_network.get_vars(),
                                                           global_network.get_vars(), thread_index)
        self.sync = self.local_network.sync_from(global_network)
        self.initial_learning_rate = initial_learning_rate
        self._own_draws = draws is None
        self.draws = draws if draws is not None else PhiloxDraws(seed, self.rank, self.B, self.world_size)
        self.seed = int(seed)                        # also the key of a configured maze's reset draws
        self.local_t = 0
        self.episode_reward = 0
        self.prev_local_t = -1
        self.start_time = time.time()
        self.environment = None
        self.experience = None
        self.last_losses = {}
        self.last_grad_norm = None
        self.time_grad_sync = False                  # bench.py: time the gradient exchange of every update
        self._sync_events = []

    # ---------------------------------------------------------------------------------------------------
    def prepare(self, termination_time=50.0, termination_dist_value=-10.0):
        B, A, dev = self.B, self.action_size, self.device
        T, Ta = self.n_step_TD, self.local_t_max
        if self.env_type == "maze":
            # a registered maze config (Environment.register_maze_config): layouts and reset draws follow the GLOBAL actor
            # index, so a job over W ranks runs what one process with all W * B actors would
            self.environment = batched_maze_environment(B, self.experience_history_size, dev,
                                                        config=Environment.MAZE_CONFIG.get(self.env_name),
                                                        actor_base=self.rank * B, actors_total=self.world_size * B,
                                                        seed=self.seed, final_obs=self.bootstrap_timeouts,
                                                        depth_labels=self.use_depth_prediction,
                                                        bonus=self.explore_beta > 0)
        elif self.env_type == "arcade":
            from ..environment.arcade_environment import BatchedArcadeEnvironment
            self.environment = BatchedArcadeEnvironment(B, self.experience_history_size, dev,
                                                        config=Environment.arcade_config(self.env_name),
                                                        actor_base=self.rank * B, actors_total=self.world_size * B,
                                                        seed=self.seed, final_obs=self.bootstrap_timeouts,
                                                        bonus=self.explore_beta > 0, versus=self.opponent_pool > 0)
        else:
            from ..environment.hostfed_environment import HostFedEnvironment
            indoor = self.env_type == "indoor"
            if indoor and getattr(self.simulator, "objective_size", 0) != self.objective_size:
                raise ValueError("simulator.objective_size != Environment.get_objective_size(%r, %r) = %d"
                                 % (self.env_type, self.env_name, self.objective_size))
            if indoor and tuple(getattr(self.simulator, "image_shape", (84, 84))) != self.image_shape:
                raise ValueError("simulator.image_shape %r != Environment.get_image_shape(%r, %r) = %r"
                                 % (getattr(self.simulator, "image_shape", (84, 84)), self.env_type, self.env_name,
                                    self.image_shape))
            gym = self.env_type == "gym"        # raw frames, resized on the device; rewards unclipped (experience.py)
            if gym and not hasattr(self.simulator, "frame_shape"):
                raise ValueError("env_type='gym' needs a simulator with frame_shape (gym_environment.GymBatchSimulator)")
            self.environment = HostFedEnvironment(self.simulator, B, self.experience_history_size, dev,
                                                  action_size=A, clip_reward=not (indoor or gym),
                                                  objective_size=self.objective_size,
                                                  reward_divisor=termination_time if indoor else 1.0,
                                                  raw_frame_shape=self.simulator.frame_shape if gym else None,
                                                  frame_shape=self.image_shape if indoor else None)
        self.overlap_host = False
        if not self.device_env:
            want = self._overlap_request if self._overlap_request is not None else (B % 2 == 0 and B >= 2048)
            if want:
                self.environment.enable_parts(2)
                self.overlap_host = True
        self.full_environment = self.environment
        self.full_ring = self.ring = self.environment.ring
        self.local_network.bind_frame_scale(self.environment.frame_scale)
        # [last action | last reward] columns of the LSTM input: within 1 for the maze (rewards -1 / 0 / +1); host-fed
        # actors feed raw rewards and measurement vectors, whose maximum is reduced per pass (model.encode_rows)
        # (navigation mazes with a reward beyond 1 feed it raw too: experience.py, unclipped; so does the arcade, where a
        # step can pay more than 1)
        conf = Environment.MAZE_CONFIG.get(self.env_name) if self.env_type == "maze" else None
        self.local_network.lar_bounded = self.env_type == "maze" and (conf is None or conf.reward_bound <= 1)
        self.experience = Experience(self.experience_history_size, ring=self.full_ring)
        B = self.Bg                                  # everything below is sized for ONE group
        M = self.reuse_minibatches
        reuse = self.reuse_epochs > 1 or M > 1
        self._alloc_pass(self, B, reuse)
        f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
        i = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        d = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)
        self.full_lstm_c, self.full_lstm_h = f(self.B * 256), f(self.B * 256)
        self.pi, self.v = f(T * B * A), f(T * B)
        self.actions, self.rewards, self.terminals = i(T * B), f(T * B), i(T * B)
        self.active_log, self.active = i(T * B), i(B)
        self.n_steps, self.terminal_end = i(B), i(B)
        self.boot_v, self.R, self.adv = f(B), f(T * B), f(T * B)
        self.u_act = d(T * B)
        self.losses = f(8)            # policy, value, entropy, pc, vr, rp, depth
        if self.use_depth_prediction:
            self.dp_hits = i(2)       # positions predicted right, positions counted: summed over a call's groups
        self.stats = d(3)
        self.loss_sum = f(8)          # losses summed over the groups of one process() call
        if reuse:                     # sample reuse: a call's sums over its reuse updates
            self.reuse_stats_i, self.reuse_stats_f = i(2), f(2)   # (clipped, counted) rows; (sum rho - 1 - ln rho, sum |rho - 1|)
            self.reuse_loss_sum = f(8)
        if self.explore_beta > 0:     # exploration bonus
            self._prepare_explore(T * B, dev)
        if self.normalize_advantages:  # advantage normalisation: a group's rows; (sum of means, of stds, groups)
            self.adv_norm, self.adv_stats = f(T * B), f(3)
        self.mb = None
        if M > 1:                     # minibatched reuse epochs: the twin of the state above for ONE block
            Bm = B // M
            mb = self.mb = PassState()
            mb.local_network, mb.block = self.local_network, None
            self._alloc_pass(mb, Bm, True)
            # the block's rows of the rollout, compacted by unreal_minibatch_gather: behaviour policy, actions, the policy
            # loss's advantages (normalised over the WHOLE rollout when normalisation is on), returns, active flags
            mb.pi, mb.actions, mb.adv, mb.R, mb.active_log = f(T * Bm * A), i(T * Bm), f(T * Bm), f(T * Bm), i(T * Bm)
            mb.adv_norm = mb.adv
            mb.losses = self.losses
            if self.use_depth_prediction:
                mb.dp_hits = self.dp_hits
            mb.reuse_stats_i, mb.reuse_stats_f = self.reuse_stats_i, self.reuse_stats_f
        self._fill_calls = 0
        self._full = False
        self._group_views = []
        for g in range(self.groups):
            b0, b1 = g * self.Bg, (g + 1) * self.Bg
            env = self.full_environment if self.groups == 1 else self.full_environment.view(b0, b1)
            self._group_views.append((env, self.full_lstm_c[b0 * 256:b1 * 256], self.full_lstm_h[b0 * 256:b1 * 256], b0))
        self._block_views = None
        if self.reuse_minibatches > 1:
            # per block of every group: the block's actors as a ring of their own (the replay branches sample it, indices
            # relative to the view) and the first actor's column of this rank's draws
            Bm = self.Bg // self.reuse_minibatches
            self._block_views = [[(ops.ring_view(env.ring, m * Bm, (m + 1) * Bm), b0 + m * Bm)
                                  for m in range(self.reuse_minibatches)] for env, _, _, b0 in self._group_views]
        if self.opponent_pool:
            self._prepare_opponents()
        self._select_group(0)
        self._rollout_split_setup()

    # ---- opponent pool ---------------------------------------------------------------------
    def _prepare_opponents(self):
        """K frozen copies of the network, a workspace per slot for Bg / K rows, LSTM state for all B opponents, the
        opponents' own draws and the buffers of a group's rollout."""
        from ..model.model import UnrealModel
        K, B, Bg, A, dev, net = self.opponent_pool, self.B, self.Bg, self.action_size, self.device, self.local_network
        T, Bk = self.n_step_TD, self.Bg // self.opponent_pool
        self.opponents = []
        for k in range(K):
            o = UnrealModel(A, net._objective_size, -1 - k, net._use_lstm, net._use_pixel_change, net._use_value_replay,
                            net._use_reward_prediction, net._pixel_change_lambda, net._entropy_beta, dev,
                            image_shape=net.image_shape, use_depth_prediction=net._use_depth_prediction)
            o.lar_bounded = False                    # a step can pay more than 1 (as Evaluate binds `versus`)
            o.bind_frame_scale(self.full_environment.frame_scale)
            o.sync_from(net)
            self.opponents.append(o)
        self.opponent_snapshots = 0                  # snapshots taken so far
        self._opp_taken = [0] * K                    # the update count every slot's weights are from
        self._opp_ws = [PathWS(Bk, Bk, dev, save_c1=False, lstm=self.use_lstm, xld=net.xld, **net.ws_kw) for _ in range(K)]
        for ws in self._opp_ws:                      # opponent.frames of a block is read with frame index b
            ws.frame_idx[:Bk].copy_(torch.arange(Bk, dtype=torch.int32))
        f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
        self.full_opp_c, self.full_opp_h = f(B * 256), f(B * 256)
        self.opp_pi, self.opp_v = f(Bg * A), f(Bg)
        self.opp_u = torch.zeros(T * Bg, dtype=torch.float64, device=dev)
        self.opponent_actions = torch.zeros(T * Bg, dtype=torch.int32, device=dev)
        # a stream of the opponents' own, keyed like the learner's by rank and batch: the learner's draws are what they
        # are without a pool
        self.opp_draws = PhiloxDraws(self.seed ^ 0x4F505053, self.rank, self.B, self.world_size)
        # per group and slot: the block's opponent buffers and LSTM state
        self._opp_views = []
        for env, _, _, b0 in self._group_views:
            blocks = []
            for k in range(K):
                r0, g0 = k * Bk, b0 + k * Bk
                blocks.append((env.opponent.view(r0, r0 + Bk), self.full_opp_c[g0 * 256:(g0 + Bk) * 256],
                               self.full_opp_h[g0 * 256:(g0 + Bk) * 256]))
            self._opp_views.append(blocks)
        # the learners' match totals (record words 12, 13) at the last opponent_scores(reset=True)
        self._opp_score_base = self.full_ring.actor_records[:, 12:14].clone()

    def _opponents_act(self, u, log=None):
        """Step 1 of an environment step with a pool: every slot's network on its block's opponent.frames (encoder, fc,
        LSTM step from the block's carried state, policy and draw with `u` [Bg]) -> opponent.actions (and `log` [Bg])."""
        Bk = self.Bg // self.opponent_pool
        for k, (net, ws, (opp, c, h)) in enumerate(zip(self.opponents, self._opp_ws, self._opp_views[self.group])):
            net.begin_pass()
            if self.use_lstm:
                ops.copy_(ws.c0, c)
                ops.copy_(ws.h0, h)
            net.encode_rows(opp, ws, 0, Bk, lar_from_ring=False, save_c1=False, lstm_x=False)
            if self.use_lstm:
                net.lstm_step(ws, 0, Bk, fused_x=True)
            feat, ld = net.features(ws, 0)
            r0 = k * Bk
            net.policy_step(Bk, feat, ld, u[r0:r0 + Bk], self.opp_pi[r0 * 4:(r0 + Bk) * 4], self.opp_v[r0:r0 + Bk],
                            opp.actions)
        if log is not None:
            ops.copy_(log, self.environment.opponent.actions)

    def _opponents_carry(self, terminals):
        """Step 3: the opponents' LSTM state advances and is zeroed where `terminals` != 0 (flag 2 included).  The fill
        passes the step's terminals; the rollout passes terminal_end, which stays set for the rest of the rollout once
        an actor's match has ended, so the opponent of an actor that sits the remaining steps out starts the next call,
        the next match's first step, from zero state."""
        if not self.use_lstm:
            return
        Bk = self.Bg // self.opponent_pool
        for k, (ws, (opp, c, h)) in enumerate(zip(self._opp_ws, self._opp_views[self.group])):
            ops.copy_(c, ws.c[:Bk * 256])
            ops.copy_(h, ws.h[:Bk * 256])
            ops.reset_state(Bk, terminals[k * Bk:(k + 1) * Bk], c, h)

    def _refresh_present_self(self):
        """Slot 0 is the present self: at the start of every process() call it equals the learner's weights."""
        self.opponents[0].sync_from(self.local_network)
        self._opp_taken[0] = self.updates
        for o in self.opponents:
            o.refresh_shadows(only_if_stale=True)

    def _snapshot_opponents(self):
        """The end of a process() call: the pool's rule (opponent_snapshot)."""
        slot, self.opponent_snapshots = self.opponent_snapshot(self.opponent_pool, self.opponent_snapshot_every,
                                                               self.updates, self.opponent_snapshots)
        if slot is not None:
            self.opponents[slot].sync_from(self.local_network)
            self._opp_taken[slot] = self.updates

    def _need_pool(self):
        if not self.opponent_pool or self.environment is None:
            raise ValueError("needs a prepared trainer with an opponent pool (Trainer(opponent_pool=K > 0))")

    def opponent(self, k):
        """Slot k's frozen network, usable as Evaluate(net, arcade=name, versus=tr.opponent(k))."""
        self._need_pool()
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < self.opponent_pool:
            raise ValueError("opponent slot %r outside 0..%d" % (k, self.opponent_pool - 1))
        return self.opponents[k]

    def opponent_ages(self):
        """Per slot: how many optimiser updates ago its weights were the learner's."""
        self._need_pool()
        return [self.updates - t for t in self._opp_taken]

    def opponent_scores(self, reset=True):
        """Per slot: matches won and lost by the learners of its blocks (this rank's, over every group) since the last
        reset -> a list of dict(slot, won, lost), from the differences of record words 12 and 13.  One device read."""
        self._need_pool()
        rec = self.full_ring.actor_records[:, 12:14]
        gain = (rec - self._opp_score_base).cpu().numpy().reshape(self.groups, self.opponent_pool, -1, 2)
        if reset:
            self._opp_score_base.copy_(rec)
        return [dict(slot=k, won=int(gain[:, k, :, 0].sum()), lost=int(gain[:, k, :, 1].sum()))
                for k in range(self.opponent_pool)]

    def opponent_state(self):
        """What a checkpoint carries of the pool: the K flat parameter vectors, the update count u and the snapshot
        count s (and the update count every slot is from)."""
        self._need_pool()
        return dict(params=[o.params.flat.detach().cpu().clone() for o in self.opponents], updates=int(self.updates),
                    snapshots=int(self.opponent_snapshots), taken=[int(t) for t in self._opp_taken])

    def load_opponent_state(self, d):
        """The inverse of opponent_state().  `d` None (a checkpoint written without a pool): every slot is refilled from
        the network's present weights, with a warning."""
        self._need_pool()
        if d is None:
            import warnings
            warnings.warn("the checkpoint holds no opponent pool: every slot restarts from the restored weights")
            for o in self.opponents:
                o.sync_from(self.local_network)
            self._opp_taken = [self.updates] * self.opponent_pool
            self.opponent_snapshots = self.updates // self.opponent_snapshot_every
            return
        if len(d["params"]) != self.opponent_pool:
            raise ValueError("the checkpoint's pool holds %d slots, this trainer's %d" % (len(d["params"]), self.opponent_pool))
        for o, flat in zip(self.opponents, d["params"]):
            if flat.numel() != o.params.flat.numel():
                raise ValueError("the checkpoint's pool holds networks of %d parameters, not %d"
                                 % (flat.numel(), o.params.flat.numel()))
            o.params.flat.copy_(flat)
            o.mark_params_changed()
        self.updates, self.opponent_snapshots = int(d["updates"]), int(d["snapshots"])
        self._opp_taken = [int(t) for t in d.get("taken", [self.updates] * self.opponent_pool)]

    def _alloc_pass(self, c, B, reuse):
        """The workspaces and buffers of the loss branches of one update over B actors, as attributes of `c`: the trainer
        itself for a group, or the minibatch twin for a block.  `reuse`: with the re-evaluated heads."""
        A, dev = self.action_size, self.device
        T, Ta = self.n_step_TD, self.local_t_max
        c.Bg = B
        c.grad_scale = 1.0 / float(B * self.world_size)
        lstm = self.use_lstm
        xld = self.local_network.xld
        wkw = self.local_network.ws_kw                # conv activation sizes of the network's frame size
        c.base_ws = PathWS(T * B, B, dev, save_c1=True, lstm=lstm, xld=xld, **wkw)
        c.boot_ws = PathWS(B, B, dev, save_c1=False, lstm=lstm, xld=xld, **wkw)
        c.rp_ws = PathWS(3 * B, B, dev, save_c1=True, lstm=False, xld=xld, **wkw) if self.use_reward_prediction else None
        # the replay passes of an update (_train_replay): pixel control and value replay as the two lanes of ONE pass over
        # 2B replayed sequences, or one pass of one lane per task that is on.  Decided HERE, once (the class default is
        # read at prepare() time only).
        lanes = tuple(n for n, on in (("pc", self.use_pixel_change), ("vr", self.use_value_replay)) if on)
        c.replay_passes = (lanes,) if self.batch_aux_default and len(lanes) == 2 else tuple((n,) for n in lanes)
        c.replay_width = len(c.replay_passes[0]) if lanes else 0
        one_lane = c.replay_width == 1             # (a one-lane pass shares the update's gradient workspace)
        rows = max(T, Ta if one_lane else 0, 3 if self.use_reward_prediction else 0) * B
        c.gws = GradWS(rows, B, dev, lstm=lstm, pc=self.use_pixel_change and one_lane, A=A, f2_dim=wkw["f2_dim"])
        # the configured width's workspaces; another width's are allocated on first use: next to the two-lane pass the
        # one-lane workspaces would be ~5 GB of dead HBM per rank at 4096 actors
        c.replay = {}
        if lanes:
            self._replay_set(c, c.replay_width)
        f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
        i = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        d = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)
        c.dlogits, c.dv = f(max(T, Ta) * B * A), f(max(T, Ta) * B)
        if self.use_depth_prediction:
            from ..model.model import DEPTH_HIDDEN, DEPTH_OUT
            c.dp_hidden, c.dp_d_hidden = f(T * B * DEPTH_HIDDEN), f(T * B * DEPTH_HIDDEN)
            c.dp_logits, c.dp_dlogits = f(T * B * DEPTH_OUT), f(T * B * DEPTH_OUT)
        if lanes:                     # what the lanes' heads write (a pass has at most one lane of a kind)
            c.seq_act = i(Ta * B)
            c.aux_v, c.aux_R, c.aux_boot_v = f(Ta * B), f(Ta * B), f(B)
            if self.use_pixel_change:
                c.boot_hp, c.boot_qmax = f(B * ops.F2_DIM), f(B * ops.PC_CELLS)
        if self.use_reward_prediction:
            c.rp_coin, c.rp_u, c.rp_class = i(B), d(B), i(B)
            c.rp_logits, c.rp_dlogits = f(B * 3), f(B * 3)
        if reuse:                     # sample reuse: the re-evaluated heads
            c.pi_new, c.v_new = f(T * B * A), f(T * B)

    def _replay_set(self, c, S):
        """The workspaces and sample buffers of a replay pass over S lanes of pass state `c` -> c.replay[S]: allocated by
        _alloc_pass for the configured width and on first use for another one (the full-size tests run one lane on a
        trainer prepared for two).  Sequence S b + s of the path workspace `ws` and of the bootstrap workspace `boot_ws` is
        lane s's sample of actor b.  Both belong to the replay pass alone and NOTHING ever writes their c0 / h0: they are
        the zero state every replayed sequence starts from (model.py:395,461) as they were allocated, at every width.
        One lane works in the update's own gradient workspace, grown to the pass's rows; more lanes have their own."""
        r = c.replay.get(S)
        if r is not None:
            return r
        B, Ta, A, dev, net = c.Bg, self.local_t_max, self.action_size, self.device, self.local_network
        L, rows = Ta + 1, Ta * B
        kw = dict(lstm=self.use_lstm, xld=net.xld, **net.ws_kw)
        i = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        r = c.replay[S] = SimpleNamespace()
        r.ws = PathWS(S * rows, S * B, dev, save_c1=True, **kw)
        r.boot_ws = PathWS(S * B, S * B, dev, save_c1=False, **kw)
        if S == 1:
            r.gws = c.gws
            r.gws.ensure_rows(rows, B, dev)
        else:
            r.gws = GradWS(S * rows, S * B, dev, lstm=self.use_lstm, pc=self.use_pixel_change, A=A, pc_rows=rows,
                           f2_dim=net.ws_kw["f2_dim"])
        # lane s's sample: L frame indices per actor (seq_idx[s], a slice of seq_idx_cat), their count, the mask of its rows
        r.seq_idx_cat = i(S * L * B)
        r.seq_idx = [r.seq_idx_cat[s * L * B:(s + 1) * L * B] for s in range(S)]
        r.seq_len, r.seq_start = [i(B) for _ in range(S)], [i(B) for _ in range(S)]
        r.seq_mask = [i(Ta * B) for _ in range(S)]
        lane = torch.arange(S, dtype=torch.int32)
        q = torch.arange(rows, dtype=torch.int32)
        r.map_seq = (q[:, None] + lane * (L * B)).reshape(-1).contiguous().to(dev)               # [S q + s] = s L B + q
        # the bootstrap frames' indices, lane after lane, and their place in boot_ws (one lane: staged in place)
        r.last, r.map_boot = r.boot_ws.frame_idx, None
        if S > 1:
            b = torch.arange(B, dtype=torch.int32)
            r.last, r.map_boot = i(S * B), (b[:, None] + lane * B).reshape(-1).contiguous().to(dev)   # [S b + s] = s B + b
        return r

    def _prepare_explore(self, rows, dev):
        """The exploration bonus's buffers: the hash's multipliers, ONE count table for this trainer (its
        groups add to it in turn; per rank: not all-reduced, and not checkpointed, like the replay), and a group's rows."""
        H, W = self.ring.frame_shape
        scale = float(self.environment.frame_scale)
        vmax = int(round(1.0 / scale)) if scale > 0 else 0
        if not 1 <= vmax <= 255:
            raise ValueError("explore_beta > 0: the environment's frame_scale %r gives a byte range of %d, outside 1..255"
                             % (scale, vmax))
        self.explore_vmax = vmax
        F = ops.explore_features(H, W, self.explore_cell, self.explore_levels, vmax, self.explore_bits)
        i = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        f = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
        self.explore_mult = i(F)
        ops.explore_multipliers(F, self.seed, self.explore_mult)
        self.explore_table = i(1 << self.explore_bits)
        self.explore_codes, self.explore_next_idx = i(rows), i(rows)
        self.explore_bonus, self.rewards_total = f(rows), f(rows)
        self.explore_stats_i, self.explore_stats_f = i(2), f(1)   # (earning rows, those counted once); sum of bonus

    def explore_counts(self):
        """The count table of the exploration bonus: int32 [2^explore_bits] on the device."""
        if self.explore_beta <= 0:
            raise ValueError("explore_counts needs Trainer(explore_beta > 0): no table is kept")
        if self.environment is None:
            self.prepare()
        return self.explore_table

    def _explore_rewards(self):
        """[Exploration bonus] of the rollout just made: the code of every earning row's NEXT observation --
        row (t, b)'s is the frame row (t + 1, b) read, the last row's the actor's current slot --, the counts, then
        rewards_total = rewards + explore_beta / sqrt(count) and the ring's r_bonus.  Three launches and a copy, no sync."""
        B, T, ws, ring = self.Bg, self.n_step_TD, self.base_ws, self.ring
        rows = T * B
        H, W = ring.frame_shape
        if T > 1:
            ops.copy_(self.explore_next_idx[:rows - B], ws.frame_idx[B:rows])
        ring.cur_idx(out=self.explore_next_idx[rows - B:rows])
        ops.frame_codes(rows, ring.frames, ring.frame_stride, ring.B * ring.H1, H, W, self.explore_next_idx,
                        self.explore_cell, self.explore_levels, self.explore_vmax, self.explore_bits, self.explore_mult,
                        self.explore_codes, gate=(B, self.active_log, self.n_steps, self.terminal_end))
        ops.count_add(rows, self.explore_codes, self.explore_table, self.explore_bits)
        ops.count_bonus(rows, self.explore_codes, self.explore_table, self.explore_bits, self.explore_beta, self.rewards,
                        self.active_log, ws.frame_idx, self.explore_bonus, self.rewards_total, ring.r_bonus,
                        self.explore_stats_i, self.explore_stats_f)

    def _select_group(self, g):
        """Point the pipeline at the actors [g*Bg, (g+1)*Bg): environment / ring views, carried LSTM state, draws."""
        env, c, h, b0 = self._group_views[g]
        self.group = g
        self.environment, self.ring, self.lstm_c, self.lstm_h = env, env.ring, c, h
        self.base_ring = env.ring                    # (PassState: a group's base rows and replay samples share its ring)
        self._point_draws(self.Bg, b0)

    def _point_draws(self, batch, b0):
        """The trainer's own draws serve `batch` actors from actor b0 of this rank on."""
        if self._own_draws:
            self.draws.batch = batch
            self.draws.col0 = self.rank * self.B + b0
        if self.opponent_pool and batch == self.Bg and getattr(self, "opp_draws", None) is not None:
            self.opp_draws.batch = batch             # (the opponents draw per group, never per minibatch block)
            self.opp_draws.col0 = self.rank * self.B + b0

    def stop(self):
        if self.environment is not None:
            self.environment.stop()

    def set_start_time(self, start_time):
        self.start_time = start_time

    def task_scores(self, reset=True):
        """Per-task scores of a game mixture (Environment.register_arcade_mix) since the last reset -> a list
        of dict(name, game, episodes, mean_return), one per task, over the episodes this rank's actors finished
        (mean_return None where a task finished none).  One device read of the ring's per-actor accumulators, summed by
        the actors' tasks on the host; `reset` zeroes them.  ValueError for anything but a mixture."""
        env = self.full_environment if self.environment is not None else None
        ring = env.ring if env is not None else None
        if ring is None or getattr(ring, "done_return", None) is None:
            raise ValueError("task_scores needs a prepared trainer on a game mixture (Environment.register_arcade_mix)")
        acc = torch.stack((ring.done_return.double(), ring.done_episodes.double())).cpu().numpy()
        if reset:
            ring.done_return.zero_()
            ring.done_episodes.zero_()
        task = env.task_of_actor()
        out = []
        for k, (name, conf) in enumerate(zip(env.config.task_names, env.config.tasks)):
            n = int(acc[1, task == k].sum())
            out.append(dict(name=name, game=conf.game, episodes=n,
                            mean_return=float(acc[0, task == k].sum()) / n if n else None))
        return out

    def _anneal_learning_rate(self, global_time_step):
        lr = self.initial_learning_rate * (self.max_global_time_step - global_time_step) / self.max_global_time_step
        return max(lr, 0.0)

    def choose_action(self, pi_values, u):
        """Inverse-CDF draw (numpy RandomState.choice semantics) -- done on device by ops.softmax_sample."""
        raise NotImplementedError("actions are drawn on the device; see ops.softmax_sample")

    # ---------------------------------------------------------------------------------------------------
    def _block(self, t, b0=0, n=None):
        """Rows [t B + b0, t B + b0 + n) of the rollout's buffers (n None: the whole time row-block t) -> the views
        (u_act, pi, v, actions, rewards, terminals, active_log)."""
        B, A = self.Bg, self.action_size
        r0 = t * B + b0
        r1 = r0 + (B if n is None else n)
        s = slice(r0, r1)
        return (self.u_act[s], self.pi[r0 * A:r1 * A], self.v[s], self.actions[s], self.rewards[s], self.terminals[s],
                self.active_log[s])

    def _next_rows(self, ws, t, b0=0, n=None):
        """What a device environment's step t of the actors [b0, b0 + n) prepares of step t + 1, as the keywords of its
        rollout_step: the rows' frame indices and, with the LSTM on, their [last action | last reward] columns; none
        after the last step."""
        B = self.Bg
        if t + 1 >= self.n_step_TD:
            return {}
        r1 = (t + 1) * B + b0
        nxt = dict(next_idx=ws.frame_idx[r1:r1 + (B if n is None else n)])
        if self.use_lstm:
            nxt.update(next_lar=ws.xcat[r1 * ws.xld:], lar_ld=ws.xld, lar_col0=256, A=self.action_size)
        return nxt

    def _policy_step(self, ws, t, b0=0, n=None, actor_ring=None, slots=None, prefilled=False, heads=True, encoded=False):
        """Forward the current observations of the actors [b0, b0 + n) (n None: all) as rows [t B + b0, t B + b0 + n) of `ws`
        and, unless the environment step does it, draw their actions into the rows' _block(); -> (feat, ld).
        `actor_ring`: the ring view of exactly these actors (a half-batch on its own stream); `slots`: that stream's running
        absmax pair (model.encode_rows).  `prefilled`: the previous environment step has already written the rows'
        frame indices and last_action_reward columns.  `heads` False: the caller's environment step computes pi / V /
        action itself (fused launch).  `encoded`: the previous environment step has also run the conv encoder on the rows'
        frames (fuse_env_encoder)."""
        B, net = self.Bg, self.local_network
        n = B if n is None else n
        r0 = t * B + b0
        if not prefilled:
            (self.ring if actor_ring is None else actor_ring).cur_idx(out=ws.frame_idx[r0:r0 + n], base_actor=b0)
        # (a goal-sense maze's step has also written the objective columns: no objective_fill launch at t > 0)
        net.encode_rows(self.ring, ws, r0, n, lar_from_ring=False, save_c1=ws.c1 is not None, actor_ring=actor_ring,
                        lar_prefilled=prefilled and self.use_lstm, lstm_x=False, slots=slots,
                        objective_prefilled=prefilled and self.use_lstm and self.device_env, encoded=encoded)
        if self.use_lstm:
            net.lstm_step(ws, t, B, b0, n, fused_x=True)
        feat, ld = net.features(ws, r0)
        if heads:
            u, pi, v, actions = self._block(t, b0, n)[:4]
            net.policy_step(n, feat, ld, u, pi, v, actions)
        return feat, ld

    FILL_SYNC_EVERY = 64
    GROUP_SYNC_EVERY = 16

    def _fill_experience(self, sess=None):
        """One policy step per call until every actor's replay is full (trainer.py:176-205)."""
        # weights are frozen while the replay fills: split them on the first call (or after an announced load)
        self.local_network.refresh_shadows(only_if_stale=self._fill_calls > 0)
        self.local_network.begin_pass()
        for g in range(self.groups):
            self._select_group(g)
            self._fill_group()
        self._select_group(0)
        self._fill_calls += 1
        # bound the queue of un-synchronised dispatches: a fill call is ~12 launches and returns at once, so a caller's
        # `while not full: process()` loop would put ~24 k dispatches in flight within a second -- rocprofv3's counter
        # thread does not survive that (profiles/r02_pmc_fault.log).  The fill is untimed; a sync every 64 calls is free.
        if self._fill_calls % self.FILL_SYNC_EVERY == 0:
            torch.cuda.current_stream().synchronize()
        if self._fill_calls >= self.experience_history_size:
            full = self.experience.is_full()
            if self.world_size > 1:            # every rank leaves the fill phase in the SAME call (the learn phase
                from .. import parallel        # issues one gradient all-reduce per call: ranks must stay paired)
                full = parallel.all_true(full, self.device)
            if full:
                self.full_environment.reset()  # trainer.py:203-205
                self._full = True

    def _fill_group(self):
        B, ws = self.Bg, self.base_ws
        if self.use_lstm:
            ops.copy_(ws.c0, self.lstm_c)
            ops.copy_(ws.h0, self.lstm_h)
        self.draws.uniform(self.u_act[:B])
        if self.opponent_pool:                 # the opponents move first
            self.opp_draws.uniform(self.opp_u[:B])
            self._opponents_act(self.opp_u[:B], self.opponent_actions[:B])
        self._policy_step(ws, 0)
        self.environment.process(self.actions[:B], None, self.rewards[:B], self.terminals[:B],
                                 reset_on_terminal=True, track_score=False)
        if self.use_lstm:                      # state advances; NOT reset on terminal here (:201-202)
            ops.copy_(self.lstm_c, ws.c[:B * 256])
            ops.copy_(self.lstm_h, ws.h[:B * 256])
        if self.opponent_pool:
            self._opponents_carry(self.terminals[:B])

    def _rollout_steps_overlapped(self):
        """The T rollout steps for host-fed actors in two half-batches: while the host steps / stages one half (its
        simulators live on the CPU), the device ingests and forwards the other half on that half's own stream.  Same
        kernels, same rows, same draws as the lock-step loop -- only the schedule differs."""
        T, ws, env = self.n_step_TD, self.base_ws, self.environment
        parts = env.parts
        main = torch.cuda.current_stream()
        start = torch.cuda.Event()
        start.record(main)

        def forward(k, t):          # on part k's stream: policy forward of its actors for step t + action D2H request
            p = parts[k]
            b0, n = p["b0"], p["b1"] - p["b0"]
            self._policy_step(ws, t, b0, n, actor_ring=p["ring"])
            env.part_request_actions(k, self._block(t, b0, n)[3], self.active[b0:b0 + n])

        for k, p in enumerate(parts):
            with torch.cuda.stream(p["stream"]):
                p["stream"].wait_event(start)
                forward(k, 0)
        for t in range(T):
            for k, p in enumerate(parts):
                b0, n = p["b0"], p["b1"] - p["b0"]
                _, _, _, actions, rewards, terminals, active_log = self._block(t, b0, n)
                env.part_host_step(k, has_active=True)           # host: the other part's device work runs meanwhile
                with torch.cuda.stream(p["stream"]):
                    env.part_ingest(k, actions, self.active[b0:b0 + n], rewards, terminals, reset_on_terminal=True,
                                    track_score=True)
                    ops.rollout_advance(n, terminals, self.active[b0:b0 + n], active_log, self.n_steps[b0:b0 + n],
                                        self.terminal_end[b0:b0 + n])
                    if t + 1 < T:
                        forward(k, t + 1)
        for p in parts:                                          # join: the learner continues on the caller's stream
            done = torch.cuda.Event()
            done.record(p["stream"])
            main.wait_event(done)

    # Maze actors: the T rollout steps as `rollout_parts` half-batches on their own HIP streams.  A
    # step is a chain of five dependent launches (conv encoder, fc, LSTM cell, policy + draw, environment) of which only
    # the first fills the chip; with two halves in flight one half's latency-bound launches run beside the other half's
    # encoder.  Same kernels, same rows, same draws as the lock-step loop.  0 / 1 = off.  Decided by same-process A/B
    # (tools/exp/rollout_split_ab.py, profiles/r04_ab_summary.md).
    rollout_parts_default = 0
    ROLLOUT_SPLIT_MIN_ACTORS = 2048
    # Maze rollout: policy head + softmax + action draw inside the environment step's launch (unreal_maze_policy_rollout_step,
    # bit-identical to unreal_policy_step + unreal_maze_rollout_step; one ~5-7 us launch less per step)
    fuse_policy_env = True
    # Top-down maze rollout at > 1024 actors (the step kernel's 8-actors-per-workgroup regime): the environment step of
    # t < T - 1 also runs the conv encoder of step t + 1 on the frames it produces, from registers
    # (unreal_maze_policy_rollout_step_encode, bit-identical to the step's launch + unreal_encoder_fwd: the frame is not
    # read back, one launch less per step).  Step 0 and the bootstrap frame keep the stand-alone encoder.  False: the two
    # launches.  Same-process A/B: tools/bench_rollout_fused.py, profiles/r06_ab_summary.md.
    fuse_env_encoder = True
    FUSE_ENV_ENCODER_MIN_ACTORS = 1025

    def _rollout_split_setup(self):
        """Per group: the halves' environment views, streams and running absmax slot pairs (built once)."""
        n_parts = self.rollout_parts_default
        self._split = None
        if not self.device_env or n_parts < 2 or self.Bg % n_parts or self.Bg < self.ROLLOUT_SPLIT_MIN_ACTORS:
            return
        if self.objective_size:                # goal-sense mazes take the lock-step loop
            return
        if self.bootstrap_timeouts:            # so does time-limit bootstrapping
            return
        if self.opponent_pool:                 # and the opponent pool
            return
        Bp = self.Bg // n_parts
        streams = [torch.cuda.Stream(device=self.device) for _ in range(n_parts)]
        self._split = []
        for env, _, _, _ in self._group_views:
            self._split.append([dict(b0=k * Bp, n=Bp, env=env.view(k * Bp, (k + 1) * Bp), stream=streams[k])
                                for k in range(n_parts)])

    def _rollout_steps_split(self):
        T, ws, net = self.n_step_TD, self.base_ws, self.local_network
        parts = self._split[self.group]
        main = torch.cuda.current_stream()
        s_f2, s_x, _ = net.ws_slots(ws)
        start = torch.cuda.Event()
        start.record(main)
        for p in parts:
            p["slots"] = (net.new_slot(), net.new_slot())
            p["stream"].wait_event(start)
        for t in range(T):
            for p in parts:
                b0, n = p["b0"], p["n"]
                _, _, _, actions, rewards, terminals, active_log = self._block(t, b0, n)
                with torch.cuda.stream(p["stream"]):
                    self._policy_step(ws, t, b0, n, actor_ring=p["env"].ring, slots=p["slots"], prefilled=t > 0)
                    p["env"].rollout_step(actions, rewards, terminals, self.active[b0:b0 + n], active_log,
                                          self.n_steps[b0:b0 + n], self.terminal_end[b0:b0 + n], index_parent=True,
                                          **self._next_rows(ws, t, b0, n))
        for p in parts:                                          # join: the learner continues on the caller's stream
            done = torch.cuda.Event()
            done.record(p["stream"])
            main.wait_event(done)
        for p in parts:                                          # the halves' running maxima cover the workspace's rows
            ops.absmax(1, 1, p["slots"][0], 1, s_f2)
            ops.absmax(1, 1, p["slots"][1], 1, s_x)

    def _rollout(self):
        """[Base A3C] n_step_TD steps of every actor of the group, bootstrap value, n-step returns (trainer.py:218-336).
        Exactly one schedule runs the steps: host-fed actors in lock-step or as two half-batches (overlap_host), device
        actors in lock-step or as half-batches on two streams (_rollout_split_setup)."""
        ws = self.base_ws
        if self.use_lstm:
            ops.copy_(ws.c0, self.lstm_c)           # start_lstm_state
            ops.copy_(ws.h0, self.lstm_h)
        self.active.fill_(1)
        self.n_steps.zero_()
        self.terminal_end.zero_()
        self.draws.uniform(self.u_act)
        if self.opponent_pool:
            self.opp_draws.uniform(self.opp_u)
        if self.overlap_host:
            self._rollout_steps_overlapped()
        elif self._split is not None:
            self._rollout_steps_split()
        elif self.device_env:
            self._rollout_steps_device()
        else:
            self._rollout_steps_host()
        self._rollout_bootstrap()
        self._rollout_returns()

    def _rollout_steps_device(self):
        """The T lock-step steps of a device environment: the maze / arcade step kernel also does the loop bookkeeping and
        prepares step t + 1 (_next_rows); with fuse_policy_env the policy head + draw run inside its launch, with
        fuse_env_encoder also the conv encoder of the next step's frames (rows t + 1 of ws: f2, saved conv1, ReLU bits,
        absmax slots)."""
        B, T, A, ws, net, env = self.Bg, self.n_step_TD, self.action_size, self.base_ws, self.local_network, self.environment
        pool = self.opponent_pool > 0
        fuse_policy = self.fuse_policy_env
        fuse_encoder = (fuse_policy and self.fuse_env_encoder and B >= self.FUSE_ENV_ENCODER_MIN_ACTORS and A == 4 and
                        getattr(env, "fused_encoder_ok", False) and not net.hw and
                        net.enc_prepared is not None and ws.c1 is not None and ws.f2_bits is not None)
        encoded = False
        for t in range(T):
            u, pi, v, actions, rewards, terminals, active_log = self._block(t)
            if pool:                           # the opponents move first; their state is carried after the step
                self._opponents_act(self.opp_u[t * B:(t + 1) * B], self.opponent_actions[t * B:(t + 1) * B])
            feat, ld = self._policy_step(ws, t, prefilled=t > 0, heads=not fuse_policy, encoded=encoded)
            step = (rewards, terminals, self.active, active_log, self.n_steps, self.terminal_end)
            nxt = self._next_rows(ws, t)
            encoded = fuse_encoder and t + 1 < T
            if encoded:
                r1 = (t + 1) * B
                s_f2, _, s_c1 = net.ws_slots(ws)
                env.policy_rollout_step_encode(net, feat, ld, u, pi, v, actions, *step, ws.f2[r1 * net.F:],
                                               ws.c1[r1 * net.c1_dim:], ws.f2_bits[r1 * ops.RELU_WORDS:], s_f2, s_c1, **nxt)
            elif fuse_policy:
                env.policy_rollout_step(net, feat, ld, u, pi, v, actions, *step, **nxt)
            else:
                env.rollout_step(actions, *step, **nxt)
            if pool:
                self._opponents_carry(self.terminal_end)

    def _rollout_steps_host(self):
        """The T lock-step steps of host-fed actors: policy step, the simulators' step, the loop bookkeeping."""
        B, ws = self.Bg, self.base_ws
        for t in range(self.n_step_TD):
            _, _, _, actions, rewards, terminals, active_log = self._block(t)
            self._policy_step(ws, t)
            self.environment.process(actions, self.active, rewards, terminals, reset_on_terminal=True, track_score=True)
            ops.rollout_advance(B, terminals, self.active, active_log, self.n_steps, self.terminal_end)

    def _rollout_bootstrap(self):
        """The carried LSTM state advances to the last step's; boot_v = V(s_T) for actors still running, with the LSTM
        state NOT advanced (model.py:687-704); the state of an actor whose episode ended is reset (trainer.py:293)."""
        B, T, A, ws, net = self.Bg, self.n_step_TD, self.action_size, self.base_ws, self.local_network
        if self.use_lstm:
            ops.copy_(self.lstm_c, ws.c[(T - 1) * B * 256:T * B * 256])
            ops.copy_(self.lstm_h, ws.h[(T - 1) * B * 256:T * B * 256])
        bw = self.boot_ws
        if self.use_lstm:
            ops.copy_(bw.c0, self.lstm_c)
            ops.copy_(bw.h0, self.lstm_h)
        if self.bootstrap_timeouts:
            # an actor cut off at the step limit (terminal_end 2) is valued at its final observation, with the state and
            # the action / reward of its last step; the others as below.  The final-observation slots are the whole
            # ring's, so the pass reads the frames by indices into it
            lstm = self.use_lstm
            ops.boot_gather(self.ring, T, A, self.terminal_end, self.n_steps, self.actions, self.rewards, bw.frame_idx[:B],
                            base_actor=self._group_views[self.group][3],
                            carried_c=self.lstm_c if lstm else None, carried_h=self.lstm_h if lstm else None,
                            ws_c=ws.c if lstm else None, ws_h=ws.h if lstm else None, c0=bw.c0 if lstm else None,
                            h0=bw.h0 if lstm else None, xcat=bw.xcat if lstm else None, ld=bw.xld, col0=256)
            feat, ld = net.trunk_forward(self.full_ring, bw, 1, B, lar_from_ring=False, save_c1=False, lar_prefilled=True)
        else:
            self.ring.cur_idx(out=bw.frame_idx[:B])
            feat, ld = net.trunk_forward(self.ring, bw, 1, B, lar_from_ring=False, save_c1=False,
                                         clip_lar=self.rp_mode == 1,   # frame.get_action_reward(): stored (clipped) reward
                                         objective_slot_offset=-1)     # ... and the objective of frame.state (:300)
        net.value_forward(B, feat, ld, self.boot_v)
        if self.use_lstm:                      # episode ended -> reset_state() (trainer.py:293)
            ops.reset_state(B, self.terminal_end, self.lstm_c, self.lstm_h)

    def _rollout_returns(self):
        """R and the advantages of the rollout's rows: n-step returns, or GAE(lambda) / time-limit bootstrapping."""
        B, T = self.Bg, self.n_step_TD
        rewards = self.rewards
        if self.explore_beta > 0:              # the returns see rewards + bonus; self.rewards stays extrinsic
            self._explore_rewards()
            rewards = self.rewards_total
        if self.bootstrap_timeouts or self.gae_lambda is not None:
            ops.base_returns_tl(B, T, rewards, self.v, self.n_steps, self.boot_v, self.terminal_end, self.gamma,
                                1.0 if self.gae_lambda is None else self.gae_lambda, self.R, self.adv)
        else:
            ops.base_returns(B, T, rewards, self.v, self.n_steps, self.boot_v, self.terminal_end, self.gamma,
                             self.R, self.adv)
        if self.normalize_advantages:          # after GAE and the bonus have shaped self.adv, which stays raw
            ops.adv_normalize(T * B, self.adv, self.active_log, self.adv_norm_eps, self.adv_norm, self.adv_stats)

    def _train_base(self, c, reuse=False):
        """Loss and backward of the rollout's rows.  `c`: the pass state holding the rows (the trainer itself; the minibatch
        twin: one block's rows).  `reuse`: the rows have been re-evaluated with the current weights (reuse_gradients):
        heads, clipped-surrogate loss against the rollout's policy c.pi and gradient in one launch."""
        B, T, A, ws, net, g, p = c.Bg, self.n_step_TD, self.action_size, c.base_ws, self.local_network, \
            self.local_network.g, self.local_network.p
        rows = T * B
        feat, ld = net.features(ws)
        adv = c.adv_norm if self.normalize_advantages else c.adv      # the policy loss's advantages
        if reuse:
            ops.ppo_heads_loss_grad(rows, A, feat, ld, p["W_base_fc_p"], p["b_base_fc_p"], p["W_base_fc_v"],
                                    p["b_base_fc_v"], c.pi, A, c.actions, adv, c.R, c.active_log,
                                    self.ppo_clip, self.entropy_beta, c.grad_scale, c.pi_new, c.v_new,
                                    c.dlogits, c.dv, c.losses[0:3], c.reuse_stats_i, c.reuse_stats_f)
        else:
            ops.base_loss_grad(rows, A, c.pi, A, c.v, c.actions, adv, c.R, c.active_log,
                               self.entropy_beta, c.grad_scale, c.dlogits, c.dv, c.losses[0:3])
        d_feat = c.gws.d_feat
        ops.linear_small_bwd(rows, 256, A, feat, ld, c.dlogits, A, p["W_base_fc_p"], d_feat, 256, False,
                             g["W_base_fc_p"], g["b_base_fc_p"])
        ops.linear_small_bwd(rows, 256, 1, feat, ld, c.dv, 1, p["W_base_fc_v"], d_feat, 256, True,
                             g["W_base_fc_v"], g["b_base_fc_v"])
        if self.use_depth_prediction:
            self._train_depth(c, rows, feat, ld, d_feat)
        net.trunk_backward(c.base_ring, ws, c.gws, T, B, d_feat, h0_nonzero=True)

    def _train_depth(self, c, rows, feat, ld, d_feat):
        """[Depth prediction] on the rollout's rows: head forward, cross-entropy against the ring's labels of
        the frames the encoder read, head backward; the head's share of d(loss)/d(feat) is added into d_feat."""
        from ..model.model import DEPTH_OUT
        net, ws = self.local_network, c.base_ws
        net.depth_head_forward(rows, feat, ld, c.dp_hidden, c.dp_logits)
        ops.depth_loss_grad(rows, c.dp_logits, DEPTH_OUT, c.base_ring.r_depth, ws.frame_idx, c.active_log,
                            self.depth_lambda * c.grad_scale, c.dp_dlogits, c.losses[6:7], c.dp_hits)
        net.depth_head_backward(rows, feat, ld, c.dp_hidden, c.dp_dlogits, c.dp_d_hidden, d_feat, 256)

    # Pixel-control head, training pass: loss + backward of the two deconvolutions in ONE launch (unreal_pc_deconv_train:
    # d_dec stays on chip, hp is staged once; 22 KB of HBM traffic per frame instead of 49).  False: the two-launch form.
    fuse_pc_deconv = True
    keep_d_dec = False       # True: the one-launch form also writes d_dec to gws.d_dec (the full-size tests read it)

    def _pc_deconv_loss_backward(self, c, gws, rows, mask, d_hp, s_hp):
        """gws.hp (relu(pc_fc1), max in slot s_hp), c.seq_act, gws.pc_R -> losses[3], d_hp, the deconv parameter
        gradients; returns the slot holding max |d_hp| (model.py:411-443, 542-557 and their gradients)."""
        A, net = self.action_size, self.local_network
        p, g = net.p, net.g
        s_dhp = net.new_slot()             # max |d_hp|: committed by the deconv backward, read by the pc_fc1 dgrad
        if self.fuse_pc_deconv:
            ops.pc_deconv_train(rows, A, gws.hp, p["W_pc_deconv_v"], p["b_pc_deconv_v"], p["W_pc_deconv_a"], p["b_pc_deconv_a"],
                                c.seq_act, gws.pc_R, mask, self.pixel_change_lambda, c.grad_scale, c.losses[3:4], d_hp,
                                g["W_pc_deconv_v"], g["b_pc_deconv_v"], g["W_pc_deconv_a"], g["b_pc_deconv_a"], dhp_max=s_dhp,
                                hp_max=s_hp, d_dec=gws.ensure_d_dec(rows, A) if self.keep_d_dec else None)
            return s_dhp
        s_dd = net.new_slot()              # bound of max |d_dec|: committed by the deconv forward
        d_dec = gws.ensure_d_dec(rows, A)
        ops.pc_deconv_fwd(rows, A, gws.hp, p["W_pc_deconv_v"], p["b_pc_deconv_v"], p["W_pc_deconv_a"],
                          p["b_pc_deconv_a"], action=c.seq_act, target=gws.pc_R, mask=mask,
                          lam=self.pixel_change_lambda, grad_scale=c.grad_scale, d_dec=d_dec,
                          loss=c.losses[3:4], hp_max=s_hp, ddec_max=s_dd)
        ops.pc_deconv_bwd(rows, A, gws.hp, d_dec, p["W_pc_deconv_v"], p["W_pc_deconv_a"], d_hp,
                          g["W_pc_deconv_v"], g["b_pc_deconv_v"], g["W_pc_deconv_a"], g["b_pc_deconv_a"], dhp_max=s_dhp,
                          hp_max=s_hp, ddec_max=s_dd)
        return s_dhp

    batch_aux_default = True       # class default, read by prepare() only (A/B tools build a second Trainer with it off)

    def _train_replay(self, c, lanes):
        """[Pixel change] / [Value replay] (trainer.py:339-412) as ONE trunk pass over S = len(lanes) replayed sequences
        per actor; `lanes`: "pc" / "vr" in the reference's order.  Sequence S b + s is actor b's sample for lane s, so a
        lane's rows are every S-th row of the workspace: it reads them with the leading dimension times S from offset
        s ld (d_feat: s 256), and every trunk kernel -- encoder, fc, the T recurrent steps, their backward -- runs once at
        S times the rows.  Draws (one per lane, in lane order), sampling, targets, heads and losses are per lane.  The
        default flag set runs ("pc", "vr"); one task alone, or batch_aux_default off, one lane per pass."""
        B, Ta, net = c.Bg, self.local_t_max, self.local_network
        S, L, rows = len(lanes), Ta + 1, Ta * B
        r = self._replay_set(c, S)
        ws, bw, gws = r.ws, r.boot_ws, r.gws
        for s in range(S):                                       # experience.sample_sequence(local_t_max + 1)
            self.draws.randint(self.experience_history_size - L - 1, r.seq_start[s])
            ops.replay_sample_seq(c.ring, L, r.seq_start[s], r.seq_idx[s], r.seq_len[s])
            ops.seq_last_idx(B, r.seq_idx[s], r.seq_len[s], r.last[s * B:(s + 1) * B])
            ops.seq_mask(B, Ta, r.seq_len[s], r.seq_mask[s])
        # bootstrap frames of every sample, from the zero LSTM state (_replay_set) -> the lanes' targets
        if S > 1:
            ops.gather_i32(r.last, r.map_boot, bw.frame_idx[:S * B])
        feat, ld = net.trunk_forward(c.ring, bw, 1, S * B, lar_from_ring=True, save_c1=False)
        for s, lane in enumerate(lanes):
            (self._pc_targets if lane == "pc" else self._vr_targets)(c, r, s, feat[s * ld:], S * ld, B)
        # the S B sequences through the trunk -> the lanes' heads, losses and d_feat
        ops.gather_i32(r.seq_idx_cat, r.map_seq, ws.frame_idx[:S * rows])
        feat, ld = net.trunk_forward(c.ring, ws, Ta, S * B, lar_from_ring=True, save_c1=True)
        for s, lane in enumerate(lanes):
            (self._pc_head if lane == "pc" else self._vr_head)(c, r, s, feat[s * ld:], S * ld, rows,
                                                               gws.d_feat[s * 256:], S * 256)
        net.trunk_backward(c.ring, ws, gws, Ta, S * B, gws.d_feat)

    def _pc_targets(self, c, r, s, feat, ld, rows):
        """Lane s's pixel-control targets r.gws.pc_R from the features of its `rows` bootstrap frames (model.py:411-443)."""
        A, net, gws = self.action_size, self.local_network, r.gws
        p = net.p
        gws.ensure_pc(self.local_t_max * c.Bg, A)      # (a lane in the update's own gradient workspace: allocated once)
        s_bhp = net.new_slot()             # max of the bootstrap frames' hp: committed by the pc_fc1 GEMM
        net.pc_head_forward(rows, feat, ld, c.boot_hp, ws=r.boot_ws, hp_max=s_bhp)
        ops.pc_deconv_fwd(rows, A, c.boot_hp, p["W_pc_deconv_v"], p["b_pc_deconv_v"], p["W_pc_deconv_a"],
                          p["b_pc_deconv_a"], qmax=c.boot_qmax, hp_max=s_bhp)
        ops.pc_returns(c.ring, self.local_t_max + 1, r.seq_idx[s], r.seq_len[s], c.boot_qmax, self.gamma_pc, gws.pc_R)

    def _pc_head(self, c, r, s, feat, ld, rows, d_feat, ldd):
        """Lane s's pixel-control head on its `rows` rows of the sequence trunk: loss, parameter gradients, d_feat."""
        net, gws = self.local_network, r.gws
        g = net.g
        s_hp = net.new_slot()              # max hp: committed by the pc_fc1 GEMM
        net.pc_head_forward(rows, feat, ld, gws.hp, ws=r.ws, hp_max=s_hp)
        ops.gather_i32(c.ring.r_action, r.seq_idx[s][:rows], c.seq_act)
        d_hp = gws.d_hp if gws.d_hp is not None else gws.d_f2
        s_dhp = self._pc_deconv_loss_backward(c, gws, rows, r.seq_mask[s], d_hp, s_hp)
        from ..model.model import _splitk
        ops.gemm_split_tn(256, 2592, rows, feat, ld, d_hp, 2592, g["W_pc_fc1"], 2592,
                          splitk=_splitk(256, 2592, rows), colsum=g["b_pc_fc1"],
                          a_max=net._one if self.use_lstm else r.ws.s_x, b_max=s_dhp)
        ops.gemm_split_nt(rows, 256, 2592, d_hp, 2592, net.shadow["pc_fc1_dgrad"], d_feat, ldd, a_max=s_dhp)

    def _vr_targets(self, c, r, s, feat, ld, rows):
        """Lane s's value-replay returns c.aux_R from the features of its `rows` bootstrap frames (model.py:446-470)."""
        self.local_network.value_forward(rows, feat, ld, c.aux_boot_v)
        ops.vr_returns(c.ring, self.local_t_max + 1, r.seq_idx[s], r.seq_len[s], c.aux_boot_v, self.gamma, c.aux_R,
                       bonus=True)

    def _vr_head(self, c, r, s, feat, ld, rows, d_feat, ldd):
        """Lane s's value head on its `rows` rows of the sequence trunk: loss, parameter gradients, d_feat."""
        net = self.local_network
        p, g = net.p, net.g
        net.value_forward(rows, feat, ld, c.aux_v)
        ops.vr_loss_grad(rows, c.aux_v, c.aux_R, r.seq_mask[s], c.grad_scale, c.dv, c.losses[4:5])
        ops.linear_small_bwd(rows, 256, 1, feat, ld, c.dv, 1, p["W_base_fc_v"], d_feat, ldd, False,
                             g["W_base_fc_v"], g["b_base_fc_v"])

    def _train_rp(self, c):
        """[Reward prediction] (trainer.py:415-436, model.py:473-488, 569-576)."""
        B, net, ws = c.Bg, self.local_network, c.rp_ws
        p, g, gws = net.p, net.g, c.gws
        self.draws.randint(2, c.rp_coin)
        self.draws.uniform(c.rp_u)
        ops.replay_sample_rp(c.ring, c.rp_coin, c.rp_u, ws.frame_idx[:3 * B], c.rp_class, self.rp_mode)
        s_c1 = net.new_slot()              # max of the conv1 activation: the c1 scale of the conv backward below
        F = net.F                          # 2592 at 84 x 84; the rp fc is [3F, 3] (model.py:480-484)
        net.encoder_forward(c.ring, ws.frame_idx[:3 * B], ws.f2, ws.c1, c1_max=s_c1, ws=ws)
        ops.linear_small_fwd(B, 3 * F, 3, ws.f2, 3 * F, p["W_rp_fc1"], p["b_rp_fc1"], c.rp_logits, 3)
        ops.rp_loss_grad(B, c.rp_logits, c.rp_class, c.grad_scale, None, c.rp_dlogits,
                         c.losses[5:6])
        ops.linear_small_bwd(B, 3 * F, 3, ws.f2, 3 * F, c.rp_dlogits, 3, p["W_rp_fc1"], gws.d_f2, 3 * F, False,
                             g["W_rp_fc1"], g["b_rp_fc1"])
        ops.relu_mask(3 * B, F, gws.d_f2, F, ws.f2, F)
        net.encoder_backward(c.ring, ws.frame_idx[:3 * B], ws.c1, gws.d_f2,
                             c1_max=s_c1)      # (d_f2's maximum: reduced by the wrapper, 127 MB at 4096 actors)

    # ---------------------------------------------------------------------------------------------------
    def compute_gradients(self):
        """Rollout + the four loss branches; leaves the local mean gradient in local_network.grads.flat."""
        net = self.local_network
        net.refresh_shadows()                  # fp16x2 weight planes follow the last optimiser step / load
        net.begin_pass()                       # absmax slots of this pass (fp16x2 GEMM scales)
        self._rollout()
        if self.use_depth_prediction and self.group == 0:
            self.dp_hits.zero_()
        if self.reuse_minibatches > 1:         # the rollout only: its updates are minibatch_gradients()' 
            return
        net.grads.flat.zero_()
        self.losses.zero_()
        self._train_base(self)
        self._train_aux(self)

    def minibatch_gradients(self, m):
        """The gradient of one minibatch update: §7q's reuse pass on block m of the selected group, the actors
        [m Bm, (m + 1) Bm) of the rollout compute_gradients() has just made.  One launch compacts the block's rows into the
        twin's buffers (self.mb); the trunk is re-run on them with the current weights from the block's start state, the
        clipped-surrogate loss reads the rollout's policy, actions, returns and advantages (normalised over the whole
        rollout when normalisation is on), and the auxiliary branches sample the block's own replay with fresh draws for Bm
        actors.  grad_scale is 1 / (Bm world_size).  base_ws, boot_ws, self.pi / v / adv / R and the carried LSTM state are
        only read."""
        M = self.reuse_minibatches
        if M < 2:
            raise ValueError("minibatch_gradients needs Trainer(reuse_minibatches > 1): its buffers are not allocated")
        if isinstance(m, bool) or not isinstance(m, int) or not 0 <= m < M:
            raise ValueError("minibatch_gradients: block %r outside 0..%d" % (m, M - 1))
        net, mb, src = self.local_network, self.mb, self.base_ws
        T, A, Bg, Bm = self.n_step_TD, self.action_size, self.Bg, self.mb.Bg
        mb.ring, b0 = self._block_views[self.group][m]
        mb.base_ring, mb.block = self.ring, m      # the gathered frame indices are relative to the group's ring
        net.refresh_shadows()
        net.begin_pass()
        dst = mb.base_ws
        lstm = dict(side=A + 1 + self.objective_size, xcat=src.xcat, xcat_out=dst.xcat, c0=src.c0, h0=src.h0,
                    c0_out=dst.c0, h0_out=dst.h0) if self.use_lstm else {}
        ops.minibatch_gather(T, Bg, Bm, m * Bm, A, src.frame_idx, self.actions, self.active_log,
                             self.adv_norm if self.normalize_advantages else self.adv, self.R, self.pi, dst.frame_idx,
                             mb.actions, mb.active_log, mb.adv, mb.R, mb.pi, ld=src.xld, **lstm)
        net.trunk_forward(self.ring, dst, T, Bm, lar_from_ring=False, save_c1=True, lar_prefilled=True,
                          objective_prefilled=True)
        net.grads.flat.zero_()
        self.losses.zero_()
        self._train_base(mb, reuse=True)
        self._point_draws(Bm, b0)                  # fresh draws for the block's Bm actors, at their own columns
        self._train_aux(mb)
        self._point_draws(Bg, self._group_views[self.group][3])

    def _train_aux(self, c):
        """The auxiliary branches of one update, each with fresh draws, in the reference's order (pc, vr, rp); `c`: the
        pass state they run on (the trainer itself; the minibatch twin: the block's actors and replay)."""
        for lanes in c.replay_passes:
            self._train_replay(c, lanes)
        if self.use_reward_prediction:
            self._train_rp(c)

    def reuse_gradients(self):
        """One more update's gradient from the rollout compute_gradients() has just made, without an
        environment step: the trunk re-run on the rollout's rows with the current weights -- frame indices, [last action |
        last reward | objective] columns and start state as the rollout left them in base_ws --, the clipped-surrogate loss
        against the behaviour policy self.pi with the rollout's advantages and returns, and the auxiliary branches with
        fresh draws.  The carried LSTM state, boot_ws and self.pi / self.v are not touched."""
        if self.reuse_epochs < 2:
            raise ValueError("reuse_gradients needs Trainer(reuse_epochs > 1): its buffers are not allocated")
        net = self.local_network
        net.refresh_shadows()
        net.begin_pass()                       # the absmax slots belong to a pass: base_ws takes fresh ones
        net.trunk_forward(self.ring, self.base_ws, self.n_step_TD, self.Bg, lar_from_ring=False, save_c1=True,
                          lar_prefilled=True, objective_prefilled=True)
        net.grads.flat.zero_()
        self.losses.zero_()
        self._train_base(self, reuse=True)
        self._train_aux(self)

    def _apply_update(self, lr):
        """Gradient exchange (multi-rank), global-norm clip + the grad_applier's step (RMSProp; Adam: DESIGN §7s) on
        local_network.grads.flat."""
        net = self.local_network
        if self.grad_sync is not None:
            if self.time_grad_sync:                  # HIP events on the launch stream around the exchange
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            self.grad_sync(net.grads.flat)           # RCCL all-reduce (sum of per-rank means / world)
            if self.time_grad_sync:
                e1.record()
                self._sync_events.append((e0, e1))
        self.last_grad_norm = self.grad_applier.step(net.params.flat, net.grads.flat, lr)
        net.mark_params_changed()
        self.updates += 1

    def process(self, sess=None, global_t=0, summary_writer=None, summary_op_dict=None, score_input=None,
                sr_input=None, eval_input=None, entropy_input=None, term_global_t=None, losses_input=None,
                sync_stats=True):
        """-> (env steps taken by this rank's actors inside the call, mean score of episodes finished or None)."""
        if self.environment is None:
            self.prepare()
        if not self._full:
            self._fill_experience(sess)
            return 0, None
        G, E, M = self.groups, self.reuse_epochs, self.reuse_minibatches
        if self.opponent_pool:
            self._refresh_present_self()
        if G > 1 or E > 1 or M > 1:
            self.loss_sum.zero_()
        if E > 1 or M > 1:
            self.reuse_loss_sum.zero_()
            self.reuse_stats_i.zero_()
            self.reuse_stats_f.zero_()
        if self.explore_beta > 0:
            self.explore_stats_i.zero_()
            self.explore_stats_f.zero_()
        if self.normalize_advantages:
            self.adv_stats.zero_()
        # (a group pass is ~300 launches per update: see the dispatch-queue bound below)
        sync_every = max(1, self.GROUP_SYNC_EVERY // (E if M == 1 else E * M))
        for g in range(G):                               # G complete actor-learner passes, one after the other
            self._select_group(g)
            # the reference reads global_t when a worker's process() starts (main.py:114-125)
            lr = self._anneal_learning_rate(global_t + g * self.Bg * self.n_step_TD * self.world_size)
            self.compute_gradients()
            if M > 1:
                self._minibatch_updates(lr, last=g + 1 == G)
            else:
                self._apply_update(lr)
            if E > 1 and M == 1:
                # update 1's losses are the ones last_losses reports under its present keys; the reuse passes overwrite
                # self.losses.  E - 1 more updates on the same rollout, at this group's learning rate
                ops.axpy(1.0 / G, self.losses, self.loss_sum)
                for _ in range(1, E):
                    self.reuse_gradients()
                    self._apply_update(lr)
                    ops.axpy(1.0 / (G * (E - 1)), self.losses, self.reuse_loss_sum)
            ops.rollout_stats(self.Bg, self.n_steps, self.ring.score_valid, self.ring.score_out, self.stats)
            if G > 1:
                if E == 1 and M == 1:
                    ops.axpy(1.0 / G, self.losses, self.loss_sum)
                # bound the un-synchronised dispatch queue like the replay fill does (a group pass is ~300 launches: at
                # G = 64 one call would enqueue ~19 k dispatches before its only host sync; rocprofv3's counter thread
                # did not survive ~24 k in the fill, profiles/r02_pmc_fault.log).  One sync per 16 groups: < 0.1 % of a call.
                if (g + 1) % sync_every == 0 and g + 1 < G:
                    torch.cuda.current_stream().synchronize()
        if G > 1:
            self._select_group(0)
        if self.opponent_pool:
            self._snapshot_opponents()
        if not sync_stats:                               # stats keep accumulating on the device
            return None, None
        steps, episodes, score_sum = self.read_stats()
        self._publish_losses()
        return steps, (score_sum / episodes if episodes > 0 else None)

    def _minibatch_updates(self, lr, last=False):
        """The E * M updates of the selected group's rollout, all at the group's learning rate: epoch e visits
        the blocks in minibatch_order(e, M).  Every update's losses join the call's mean.  The un-synchronised dispatch
        queue keeps process()'s bound: a host sync after every GROUP_SYNC_EVERY updates (`last`: but not after the call's
        final update, which the caller's read of the stats follows)."""
        G, E, M = self.groups, self.reuse_epochs, self.reuse_minibatches
        done = 0
        for e in range(1, E + 1):
            for m in self.minibatch_order(e, M):
                self.minibatch_gradients(m)
                self._apply_update(lr)
                ops.axpy(1.0 / (G * E * M), self.losses, self.loss_sum)
                done += 1
                if done % self.GROUP_SYNC_EVERY == 0 and not (last and done == E * M):
                    torch.cuda.current_stream().synchronize()

    def grad_sync_ms(self):
        """[ms] of every gradient exchange since the last call (time_grad_sync): from the point the launch stream reaches
        the all-reduce (the backward kernels before it have drained) to the point it may continue with clip + RMSProp."""
        torch.cuda.synchronize()
        out = [e0.elapsed_time(e1) for e0, e1 in self._sync_events]
        self._sync_events = []
        return out

    def read_stats(self):
        """(env steps, finished episodes, sum of their scores) since the last read; one host sync."""
        st = self.stats.cpu().numpy()
        self.stats.zero_()
        steps, episodes, score_sum = int(st[0]), int(st[1]), float(st[2])
        self.local_t += steps
        return steps, episodes, score_sum

    def _publish_losses(self):
        # groups: mean over the call's groups; with reuse_epochs > 1 of every group's update 1 (process())
        M = self.reuse_minibatches
        l = (self.loss_sum if self.groups > 1 or self.reuse_epochs > 1 or M > 1 else self.losses).cpu().numpy()
        # the loss kernels scale their sums by grad_scale = 1 / (Bg world_size), the gradient's scale: a rank reports the
        # mean over ITS OWN actors, as a one-rank job does, not its 1 / world_size share of the job's mean
        W = float(self.world_size)
        if W > 1:
            l = l * W
        net = self.local_network
        net.policy_loss, net.value_loss, net.entropy = float(l[0]), float(l[1]), float(l[2])
        net.base_loss = net.policy_loss + net.value_loss
        net.pc_loss, net.vr_loss, net.rp_loss = float(l[3]), float(l[4]), float(l[5])
        net.total_loss = net.base_loss + net.pc_loss + net.vr_loss + net.rp_loss
        if self.use_depth_prediction:
            net.depth_loss = float(l[6])
            net.total_loss += net.depth_loss
        self.last_losses = dict(total_loss=net.total_loss, base_loss=net.base_loss, policy_loss=net.policy_loss,
                                value_loss=net.value_loss, entropy=net.entropy, pc_loss=net.pc_loss,
                                vr_loss=net.vr_loss, rp_loss=net.rp_loss,
                                grad_norm=float(self.last_grad_norm.cpu()[0]))
        if self.use_depth_prediction:
            hits = self.dp_hits.cpu().numpy()
            self.last_losses.update(depth_loss=net.depth_loss, depth_accuracy=float(hits[0]) / max(int(hits[1]), 1))
        if self.reuse_epochs > 1 or M > 1:  # means over the call's reuse updates; the two counts are exact
            # (minibatches, DESIGN §7t: every update of the call is a reuse update, so the means above are theirs)
            r = l if M > 1 else self.reuse_loss_sum.cpu().numpy() * W
            si, sf = self.reuse_stats_i.cpu().numpy(), self.reuse_stats_f.cpu().numpy()
            n = max(int(si[1]), 1)
            self.last_losses.update(reuse_policy_loss=float(r[0]), reuse_value_loss=float(r[1]), reuse_entropy=float(r[2]),
                                    clip_fraction=float(si[0]) / n, approx_kl=float(sf[0]) / n)
            if M > 1:
                self.last_losses["updates"] = self.groups * self.reuse_epochs * M
        if self.explore_beta > 0:         # over the call's groups; the counts are exact
            si, sf = self.explore_stats_i.cpu().numpy(), self.explore_stats_f.cpu().numpy()
            n = max(int(si[0]), 1)
            self.last_losses.update(explore_bonus=float(sf[0]) / n, explore_first=float(si[1]) / n)
        if self.normalize_advantages:     # means over the call's groups of each rollout's mean and std
            st = self.adv_stats.cpu().numpy()
            n = max(float(st[2]), 1.0)
            self.last_losses.update(adv_mean=float(st[0]) / n, adv_std=float(st[1]) / n)
        return self.last_losses

    def _print_log(self, global_t):
        if self.thread_index == 0 and self.local_t - self.prev_local_t >= PERFORMANCE_LOG_INTERVAL:
            self.prev_local_t += PERFORMANCE_LOG_INTERVAL
            el = time.time() - self.start_time
            print("### Performance : {} STEPS in {:.0f} sec. {:.0f} STEPS/sec. {:.2f}M STEPS/hour".format(
                global_t, el, global_t / el, global_t / el * 3600 / 1e6))
