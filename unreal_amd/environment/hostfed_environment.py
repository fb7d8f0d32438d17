"""Host-fed batched environment: CPU simulators -> pinned uint8 staging -> HBM replay ring.

Keeps the contract of /root/reference/environment/lab_environment.py:78-119 for every actor (frame = obs/255,
state unchanged and pixel change 0 on a terminal step, reset by the trainer) while the learner stays the
batched device path: frames are stored as uint8 and the encoder applies frame_scale = 1/255 on load.
`simulator` is any object with reset(mask) -> frames and step(actions, active) -> (frames, rewards, terminals)
(see synthetic_sim.SyntheticBatchSimulator); DeepMind Lab itself is not in the image.

With objective_size > 0 it is the MINOS wrapper contract of /root/reference/environment/indoor_environment.py:63-139
instead: the simulator also returns a measurement vector per actor (reset -> (frames, objectives),
step -> (frames, rewards, terminals, objectives)), stored beside the frame in the ring and concatenated into the LSTM
input; rewards are divided by termination_time (:111) and not clipped.

With raw_frame_shape = (Hs, Ws) it is the gym contract of /root/reference/environment/gym_environment.py:18-96 instead
(gym_environment.GymBatchSimulator): the simulator returns RAW frames [n, Hs, Ws, 3] which are staged as they are and
resized to 84 x 84 on the device (ops.frame_resize); step returns the TERMINAL observation where terminal, the
environment then resets those actors (sim.reset(mask)) and commits with the gym terminal rule (ops.hostfed_step with
terminal_obs: pixel change against the terminal observation, the post-reset observation into the next slot); rewards are
not clipped.

Lock-step (reset / process) and the half-batch schedule (enable_parts) run the same host-step and ingest routines: the
whole batch is one part on the current stream."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops

# The simulators' frames reach the pinned staging by a host memcpy of 21 KB per actor and step -- the largest host
# cost of the path.  It is cut into row blocks copied by a few threads with numpy's copy, which releases the GIL (torch's
# copy_ starts its own intra-op team inside every pool thread: 8 pool threads x that team ran at a third of the rate).
# UNREAL_COPY_THREADS overrides the count (default: up to 8; a GPU's share of the host is 16 cores on the test boxes).
_COPY_THREADS = int(os.environ.get("UNREAL_COPY_THREADS", 0)) or max(1, min(8, (os.cpu_count() or 1) // 2))
_COPY_POOL = ThreadPoolExecutor(_COPY_THREADS) if _COPY_THREADS > 1 else None


def _stage(h, frames, dst):
    """h (pinned uint8 [n, row]) <- frames (uint8 [n, ...]; each frame at the start of its row, rows may be longer, e.g.
    ring.frame_stride), in parallel row blocks; then dst (device bytes) <- h, one H2D copy on the current stream.  (Staging
    and H2D as a pipeline of pieces was measured slower: profiles/r04_hostfed.md.)"""
    n, row = h.shape
    src = np.asarray(frames).reshape(n, -1)
    d = h.numpy()[:, :src.shape[1]]
    if _COPY_POOL is None or n < 4 * _COPY_THREADS:
        np.copyto(d, src)
    else:
        step = (n + _COPY_THREADS - 1) // _COPY_THREADS
        futs = [_COPY_POOL.submit(np.copyto, d[a:a + step], src[a:a + step]) for a in range(0, n, step)]
        for f in futs:
            f.result()
    dst[:n * row].copy_(h.view(-1), non_blocking=True)


class HostFedEnvironment(object):
    def __init__(self, simulator, batch, history_size, device="cuda:0", action_size=6, clip_reward=True,
                 frame_max=255.0, objective_size=0, reward_divisor=1.0, raw_frame_shape=None, frame_shape=None,
                 depth_labels=False):
        if depth_labels:          # the labels come from a device maze's own walls
            raise ValueError("depth_labels is out of scope for host-fed environments: the device does not know their "
                             "geometry (it needs a first-person device maze)")
        self.B, self.sim = batch, simulator
        self.action_size = action_size
        self.clip_reward = clip_reward
        self.objective_size = int(objective_size)
        self.reward_divisor = float(reward_divisor)
        self.pc_denom = 48.0 * frame_max
        self.frame_scale = 1.0 / frame_max          # lab_environment.py:99-102: state = obs / 255
        self.device = torch.device(device)
        # frame_shape (H, W) != (84, 84): the indoor contract at another frame size (frames ring.frame_stride bytes apart,
        # no pixel change)
        self.frame_shape = ops.FRAME_SHAPE if frame_shape is None else (int(frame_shape[0]), int(frame_shape[1]))
        if self.frame_shape != ops.FRAME_SHAPE and (raw_frame_shape is not None or not objective_size):
            raise ValueError("frame_shape %r: other frame sizes are the indoor contract only (objective_size > 0, no "
                             "raw frames)" % (self.frame_shape,))
        self.ring = ops.Ring(batch, history_size, self.device, objective_size=self.objective_size,
                             frame_shape=self.frame_shape)
        self.frame_stride = self.ring.frame_stride
        # gym: raw frames [Hs, Ws, 3] are staged, the resize to 84 x 84 runs on the device; terminal actors' post-reset
        # observations go through a second raw staging (only in steps with a terminal)
        self.raw_shape = None if raw_frame_shape is None else (int(raw_frame_shape[0]), int(raw_frame_shape[1]))
        self.gym = self.raw_shape is not None
        self.row_bytes = self.raw_shape[0] * self.raw_shape[1] * 3 if self.gym else self.frame_stride   # a staged row
        # device staging, [name] = (elements per actor, tensor); a part's are slices
        dev = lambda n, dt=torch.uint8: (n, torch.zeros(batch * n, dtype=dt, device=self.device))
        self._dev = dict(staged=dev(self.frame_stride), rewards=dev(1, torch.float32), terminals=dev(1, torch.int32))
        if self.gym:
            self._dev.update(raw=dev(self.row_bytes), raw_reset=dev(self.row_bytes), reset84=dev(ops.FRAME_BYTES),
                             reset_mask=dev(1, torch.int32))
        if self.objective_size:
            self._dev.update(obj=dev(self.objective_size, torch.float32))
        self._all = self._part(0, batch, None)      # reset() / process(): the whole batch on the current stream
        self.reset()

    def get_action_size(self):
        return self.action_size

    def _part(self, b0, b1, stream):
        """Actors [b0, b1) with their own ring view, pinned staging and slices of the device staging; stream None: the
        current stream of each call."""
        n = b1 - b0
        pin = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt).pin_memory()
        p = {k: t[b0 * m:b1 * m] for k, (m, t) in self._dev.items()}
        p.update(b0=b0, b1=b1, ring=ops.ring_view(self.ring, b0, b1), stream=stream, h2d_done=None,
                 act_ready=torch.cuda.Event(), h_frames=pin(n, self.row_bytes), h_rewards=pin(n, dt=torch.float32),
                 h_terminals=pin(n, dt=torch.int32), h_actions=pin(n, dt=torch.int32), h_active=pin(n, dt=torch.int32))
        if self.gym:
            p.update(h_reset=pin(n, self.row_bytes), h_reset_mask=pin(n, dt=torch.int32), any_reset=False)
        if self.objective_size:
            p.update(h_obj=pin(n, self.objective_size, dt=torch.float32))
        return p

    @staticmethod
    def _wait_staging(p):
        """A part's pinned staging may be rewritten only after the H2D copies that read it have finished."""
        if p["h2d_done"] is not None:
            p["h2d_done"].synchronize()

    @staticmethod
    def _mark_staging(p):
        if p["h2d_done"] is None:
            p["h2d_done"] = torch.cuda.Event()
        p["h2d_done"].record()

    def _stage_obs(self, p, frames, objectives):
        """Part p's rows of the simulators' observations into its pinned staging: the frames on to the device (on p's
        stream), the objectives as far as pinned memory."""
        b0, b1 = p["b0"], p["b1"]
        with torch.cuda.stream(p["stream"]):
            _stage(p["h_frames"], frames[b0:b1], p["raw"] if self.gym else p["staged"])
        if self.objective_size:
            p["h_obj"].copy_(torch.from_numpy(np.ascontiguousarray(objectives[b0:b1], dtype=np.float32)))

    def _resize(self, p, src, dst, mask=None):
        ops.frame_resize(p["b1"] - p["b0"], self.raw_shape[0], self.raw_shape[1], src, dst, mask=mask)

    def _put_objectives(self, p, active):
        if self.objective_size:
            p["obj"].copy_(p["h_obj"].view(-1), non_blocking=True)
            ops.objective_put(p["ring"], p["obj"], active)       # into the slot the frame just went to

    def _gym_resets(self, p, terminals, active):
        """Part p's actors that ended an episode: sim.reset(mask) (the trainer's env.reset(), trainer.py:201-202), their raw
        post-reset observations and the mask staged (H2D on p's stream); the masked resize follows in _ingest.  Call after
        the step's own frames are staged (the simulator reuses its frame array).  -> whether any actor was reset."""
        b0, b1 = p["b0"], p["b1"]
        term = np.zeros(self.B, np.int32)
        term[b0:b1] = np.asarray(terminals[b0:b1]) != 0
        if active is not None:
            term[b0:b1] &= np.asarray(active[b0:b1]) != 0
        if not term.any():
            return False
        frames = self.sim.reset(term)
        with torch.cuda.stream(p["stream"]):
            _stage(p["h_reset"], frames[b0:b1], p["raw_reset"])
            p["h_reset_mask"].copy_(torch.from_numpy(term[b0:b1]))
            p["reset_mask"].copy_(p["h_reset_mask"], non_blocking=True)
        return True

    def _host_step(self, p, actions, active):
        """Host phase of part p: step the simulators (actions / active: whole-batch arrays, passed on as they are), stage
        p's rows of what they return."""
        out = self.sim.step(actions, active)
        frames, rewards, terminals = out[:3]
        b0, b1 = p["b0"], p["b1"]
        self._wait_staging(p)
        self._stage_obs(p, frames, out[3] if self.objective_size else None)
        if self.gym:
            p["any_reset"] = self._gym_resets(p, terminals, active)
        rewards = rewards[b0:b1]
        if self.reward_divisor != 1.0:                  # indoor_environment.py:111
            rewards = (rewards.astype(np.float64) / self.reward_divisor).astype(np.float32)
        p["h_rewards"].copy_(torch.from_numpy(np.ascontiguousarray(rewards, dtype=np.float32)))
        p["h_terminals"].copy_(torch.from_numpy(np.ascontiguousarray(terminals[b0:b1], dtype=np.int32)))

    def _ingest(self, p, actions, active, out_reward, out_terminal, reset_on_terminal, track_score):
        """Device phase of part p on the current stream: H2D of its rewards / terminals, the gym resizes, the ring commit
        kernel and the objectives."""
        p["rewards"].copy_(p["h_rewards"], non_blocking=True)
        p["terminals"].copy_(p["h_terminals"], non_blocking=True)
        if self.gym:
            self._resize(p, p["raw"], p["staged"])
            if p["any_reset"]:
                self._resize(p, p["raw_reset"], p["reset84"], p["reset_mask"])
        ops.hostfed_step(p["ring"], p["staged"], actions, p["rewards"], p["terminals"], active, out_reward, out_terminal,
                         reset_on_terminal, track_score, clip_reward=self.clip_reward and not self.gym,
                         pc_denom=self.pc_denom, reset_staged=p.get("reset84"), terminal_obs=self.gym)
        self._put_objectives(p, active)
        self._mark_staging(p)

    def reset(self, mask=None):
        p = self._all
        out = self.sim.reset(None if mask is None else mask.cpu().numpy())
        frames, objectives = out if self.objective_size else (out, None)
        self._wait_staging(p)
        self._stage_obs(p, frames, objectives)
        if self.gym:
            self._resize(p, p["raw"], p["staged"])
        ops.hostfed_reset(p["ring"], p["staged"], mask)
        self._put_objectives(p, mask)
        self._mark_staging(p)

    def process(self, actions, active=None, out_reward=None, out_terminal=None, reset_on_terminal=True,
                track_score=False):
        a = actions.cpu().numpy()                       # the simulators live on the host: one D2H per step
        self._host_step(self._all, a, None if active is None else active.cpu().numpy())
        self._ingest(self._all, actions, active, out_reward, out_terminal, reset_on_terminal, track_score)

    # ---- half-batch interface: host phase of one part overlaps the device phase of the other ---------
    def enable_parts(self, n_parts=2):
        """Split the actors into `n_parts` contiguous parts, each with its own HIP stream, pinned staging and ring view,
        so that the Trainer can alternate: while the host simulates / stages part k, the device ingests and forwards the
        other part.  Returns the part boundaries [(b0, b1), ...]."""
        if self.B % n_parts:
            raise ValueError("%d actors do not split into %d parts" % (self.B, n_parts))
        Bp = self.B // n_parts
        self.parts = [self._part(k * Bp, (k + 1) * Bp, torch.cuda.Stream(device=self.device)) for k in range(n_parts)]
        self._act_full = np.zeros(self.B, np.int32)
        self._mask_full = np.zeros(self.B, np.int32)
        return [(p["b0"], p["b1"]) for p in self.parts]

    def part_request_actions(self, k, actions, active):
        """On part k's stream: start the D2H copy of its drawn actions (and active flags) into pinned memory."""
        p = self.parts[k]
        p["h_actions"].copy_(actions, non_blocking=True)
        if active is not None:
            p["h_active"].copy_(active, non_blocking=True)
        p["act_ready"].record()

    def part_host_step(self, k, has_active):
        """Host phase of part k: wait for its actions, step ITS simulators only (the others masked out), fill its pinned
        staging."""
        p = self.parts[k]
        p["act_ready"].synchronize()
        b0, b1 = p["b0"], p["b1"]
        self._act_full[b0:b1] = p["h_actions"].numpy()
        self._mask_full[:] = 0
        self._mask_full[b0:b1] = p["h_active"].numpy() if has_active else 1
        self._host_step(p, self._act_full, self._mask_full)

    def part_ingest(self, k, actions, active, out_reward, out_terminal, reset_on_terminal=True, track_score=False):
        """On part k's stream: H2D of the staged part + the ring commit kernel for its actors."""
        self._ingest(self.parts[k], actions, active, out_reward, out_terminal, reset_on_terminal, track_score)

    def stop(self):
        pass
