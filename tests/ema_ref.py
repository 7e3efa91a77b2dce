"""Reference arithmetic of the weight average (csrc/optim.hip ema_kernel, detr_tf/optimizers.py WeightEMA): a NumPy float32
restatement of tf.train.ExponentialMovingAverage's update and of its decay rule.  Nothing here reads a GPU result.

The update is TensorFlow's assign_sub form, three float32 operations that are each rounded on their own:

    t = shadow - param;  t = omd * t;  shadow = shadow - t          omd = float32(1 - decay), the difference taken in double

NumPy's float32 array arithmetic rounds every operation to float32 and never fuses a multiply into an add, so a kernel that
does the same gives the same bits.
"""
import numpy as np


def step_decay(decay, warmup, num_updates):
    """This update's decay (double): `decay`, or with warmup min(decay, (1 + n) / (10 + n)), n = updates done before."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + num_updates) / (10.0 + num_updates))
    return d


def omd_of(decay):
    return np.float32(1.0 - float(decay))


def update(shadow, param, omd):
    """One update; float32 arrays in, a new float32 array out."""
    shadow = np.asarray(shadow, dtype=np.float32)
    param = np.asarray(param, dtype=np.float32)
    omd = np.float32(omd)
    t = shadow - param
    t = omd * t
    out = shadow - t
    assert out.dtype == np.float32
    return out


def closed_form(shadow0, params, decays):
    """float64: s_k = d_k * s_{k-1} + (1 - d_k) * p_k."""
    s = np.asarray(shadow0, dtype=np.float64)
    for p, d in zip(params, decays):
        s = d * s + (1.0 - d) * np.asarray(p, dtype=np.float64)
    return s
