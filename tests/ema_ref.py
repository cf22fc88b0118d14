"""NumPy restatement of the weight-averaging update (include/taco_hip.h taco_param_ema): the three float32 operations of the update,
TF's num_updates warm-up of the decay, and the two sums of the statistics in float64.  Imports without a GPU and without the library."""
import math

import numpy as np


def ema_update(e, p, w):
    """e + w (p - e) as three separately rounded float32 operations -> a new float32 array; e and p float32 arrays, w a float32"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    w = np.float32(w)
    d = (p - e).astype(np.float32)
    t = (w * d).astype(np.float32)
    return (e + t).astype(np.float32)


def ema_update_tf(e, p, decay_w):
    """TF's assign_moving_average form, shadow - (1 - decay) (shadow - var), with 1 - decay given as the float32 w"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    w = np.float32(decay_w)
    return (e - (w * (e - p).astype(np.float32)).astype(np.float32)).astype(np.float32)


def ema_decay(decay, k):
    """tf.train.ExponentialMovingAverage(decay, num_updates=k): min(decay, (1 + k) / (10 + k)) in Python floats"""
    return min(float(decay), (1.0 + k) / (10.0 + k))


def ema_weight(decay, k):
    """w of update k: 1 - ema_decay in Python floats, rounded once to float32"""
    return np.float32(1.0 - ema_decay(decay, k))


def ema_stats(e, p):
    """(sum of (double)d^2 with d the FLOAT32 difference p - e, sum of (double)p^2) by exact summation of the float64 products,
    which are themselves exact"""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    d = (p - e).astype(np.float32).astype(np.float64)
    pd = p.astype(np.float64)
    return math.fsum(d * d), math.fsum(pd * pd)
