"""Adam / AdamW with global-norm clipping over flat device buffers: a drop-in for RMSPropApplier as the
`grad_applier` of Trainer.

One deterministic norm reduction (ops.grad_norm, shared with RMSProp) and one fused kernel over the flat parameter buffer
(ops.adam_step) with PyTorch's Adam / AdamW arithmetic.  The step count `t` lives on the host: the bias corrections
1 - beta^t are computed in fp64 and passed as kernel arguments, so a step needs no device counter and no sync."""
import math

import torch

from .. import ops


def _number(name, v, ok, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not ok(v):
        raise ValueError("%s = %r: %s" % (name, v, what))
    return float(v)


def bias_corrections(beta1, beta2, t):
    """(1 - beta1^t, 1 - beta2^t) in fp64 for step t >= 1."""
    return 1.0 - float(beta1) ** int(t), 1.0 - float(beta2) ** int(t)


class AdamApplier(object):
    kind = "adam"

    def __init__(self, learning_rate=None, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.0, clip_norm=40.0,
                 device="cuda:0", name="AdamApplier"):
        self._name = name
        self._learning_rate = learning_rate
        self._beta1 = _number("beta1", beta1, lambda v: 0.0 <= v < 1.0, "a number in [0, 1)")
        self._beta2 = _number("beta2", beta2, lambda v: 0.0 <= v < 1.0, "a number in [0, 1)")
        self._epsilon = _number("epsilon", epsilon, lambda v: v > 0.0, "a finite number > 0")
        self._weight_decay = _number("weight_decay", weight_decay, lambda v: v >= 0.0, "a finite number >= 0")
        self._clip_norm = _number("clip_norm", clip_norm, lambda v: True, "a finite number (<= 0: no clipping)")
        self._device = device
        self._slots = {}
        self.m = self.v = None
        self.t = 0                      # steps taken: every update counts, reuse updates and groups included
        self._scratch = self._norm = None

    def _create_slots(self, flat):
        if self.m is None or self.m.numel() != flat.numel():
            self.m = torch.zeros_like(flat)
            self.v = torch.zeros_like(flat)
            self._scratch = torch.zeros(256, dtype=torch.float32, device=flat.device)
            self._norm = torch.zeros(1, dtype=torch.float32, device=flat.device)
        self._slots = {"m": self.m, "v": self.v}

    def get_slot(self, var, name):
        return self._slots.get(name)

    def step(self, flat_params, flat_grad, lr):
        """clip_by_global_norm + Adam on the flat buffers; returns the (device) pre-clip norm."""
        self._create_slots(flat_params)
        self.t += 1
        bc1, bc2 = bias_corrections(self._beta1, self._beta2, self.t)
        ops.grad_norm(flat_grad, self._scratch, self._norm)
        ops.adam_step(flat_params, self.m, self.v, flat_grad, lr, self._beta1, self._beta2, self._epsilon,
                      self._weight_decay, bc1, bc2, self._clip_norm, self._norm)
        return self._norm

    def minimize_local(self, loss, global_var_list, local_var_list, thread_index=None):
        """The (applier, norm handle) pair shape of RMSPropApplier.minimize_local."""
        return self, self._norm
