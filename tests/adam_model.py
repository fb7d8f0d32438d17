"""fp64 numpy model of DESIGN §7s, written from the contract in include/unreal_hip.h: the clip scale, AdamW's decoupled
decay, the two moments, the bias corrections, the parameter step, the applier's step counting, and the masked normalisation
of a rollout's advantages."""
import numpy as np


def clip_scale(norm, clip_norm):
    """grad is multiplied by clip_norm * min(1 / norm, 1 / clip_norm) when clip_norm > 0 and norm > 0, else by 1."""
    norm, clip_norm = float(norm), float(clip_norm)
    if clip_norm > 0.0 and norm > 0.0:
        return clip_norm * min(1.0 / norm, 1.0 / clip_norm)
    return 1.0


def bias_corrections(beta1, beta2, t):
    return 1.0 - float(beta1) ** int(t), 1.0 - float(beta2) ** int(t)


def adam_step(var, m, v, grad, lr, beta1, beta2, eps, weight_decay, bc1, bc2, clip_norm=0.0, norm=None):
    """One step -> dict(var, m, v, g, decayed, update): g the clipped gradient, decayed the parameters after the decay line,
    update what the last line subtracts.  `norm` None: the gradient's own L2 norm in fp64."""
    var, m, v, grad = (np.asarray(x, dtype=np.float64) for x in (var, m, v, grad))
    if norm is None:
        norm = np.sqrt((grad * grad).sum())
    g = grad * clip_scale(norm, clip_norm)
    decayed = var * (1.0 - lr * weight_decay) if weight_decay != 0 else var.copy()
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    update = (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return dict(var=decayed - update, m=m, v=v, g=g, decayed=decayed, update=update)


class Adam(object):
    """The applier: slots from 0, t counted per step, bias corrections from t."""

    def __init__(self, n, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, clip_norm=40.0):
        self.beta1, self.beta2, self.eps, self.weight_decay, self.clip_norm = beta1, beta2, eps, weight_decay, clip_norm
        self.m, self.v, self.t = np.zeros(n), np.zeros(n), 0

    def step(self, var, grad, lr, norm=None):
        self.t += 1
        bc1, bc2 = bias_corrections(self.beta1, self.beta2, self.t)
        out = adam_step(var, self.m, self.v, grad, lr, self.beta1, self.beta2, self.eps, self.weight_decay, bc1, bc2,
                        self.clip_norm, norm)
        self.m, self.v = out["m"], out["v"]
        return out


def adv_normalize(adv, active, eps):
    """-> (adv_out, mean, std, n) over the rows with active != 0: population variance in two passes; inactive rows 0; with
    fewer than 2 active rows the active rows keep their value (mean = that value or 0, std = 0)."""
    adv = np.asarray(adv, dtype=np.float64)
    on = np.asarray(active) != 0
    n = int(on.sum())
    out = np.zeros_like(adv)
    if n == 0:
        return out, 0.0, 0.0, 0
    x = adv[on]
    mean = x.sum() / n
    std = float(np.sqrt(((x - mean) ** 2).sum() / n))
    out[on] = x if n < 2 else (x - mean) / (std + float(eps))
    return out, float(mean), std, n
