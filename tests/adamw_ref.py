"""float64 NumPy restatement of the optimiser step of detr_tf/optimizers.py with its opt-in extensions, written from the
formulas (tf.keras.optimizers.AdamW, tf.clip_by_norm, tf.clip_by_global_norm):

    G  = sqrt(sum over every TRAINED tensor of sum(g^2))            s = c / max(G, c)         (global_clipnorm = c)
    g  = s * g                       or   g * clipnorm / max(||g||, clipnorm) per tensor      (clipnorm)
    p  = p - lr * weight_decay * p                                                            (decoupled, plain lr)
    m  = b1*m + (1-b1)*g ;  v = b2*v + (1-b2)*g*g
    p  = p - lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)

`lr` and the step count `t` belong to the tensor's GROUP; a group steps when at least one of its tensors is in `grads`.
Everything is float64; nothing here reads a GPU result."""
import math

import numpy as np


def global_norm(grads):
    return math.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads))


class AdamW:
    def __init__(self, lrs, groups, weight_decay=0.0, global_clipnorm=None, clipnorm=None, beta1=0.9, beta2=0.999, eps=1e-7):
        """lrs: group -> learning rate; groups: tensor key -> group."""
        self.lrs, self.groups = dict(lrs), dict(groups)
        self.weight_decay, self.global_clipnorm, self.clipnorm = weight_decay, global_clipnorm, clipnorm
        self.b1, self.b2, self.eps = beta1, beta2, eps
        self.t = {g: 0 for g in self.lrs}
        self.m, self.v = {}, {}
        self.last_norm = None

    def step(self, grads, params):
        """grads: key -> gradient of every tensor trained in this step; params: key -> float64 array, updated in place.
        Returns the clip factor s (1.0 without global_clipnorm)."""
        s = 1.0
        if self.global_clipnorm is not None:
            self.last_norm = global_norm(grads.values())
            s = self.global_clipnorm / max(self.last_norm, self.global_clipnorm)
        for grp in sorted({self.groups[k] for k in grads}):
            self.t[grp] += 1
        for k, g in grads.items():
            grp = self.groups[k]
            lr, t = self.lrs[grp], self.t[grp]
            g = np.asarray(g, np.float64)
            if self.global_clipnorm is not None:
                g = s * g
            elif self.clipnorm is not None:
                g = g * (self.clipnorm / max(math.sqrt(float(np.sum(g * g))), self.clipnorm))
            p = params[k]
            assert p.dtype == np.float64
            p -= lr * self.weight_decay * p
            m = self.m[k] = self.b1 * self.m.get(k, 0.0) + (1.0 - self.b1) * g
            v = self.v[k] = self.b2 * self.v.get(k, 0.0) + (1.0 - self.b2) * g * g
            p -= lr * math.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t) * m / (np.sqrt(v) + self.eps)
        return s
