"""The host-side argument checks of the entry-point wrappers in lib.py, in one place.

Every checker raises ValueError whose message starts with `who: ` (the wrapper's name) and names the argument.  Nothing here touches
the shared library or a device: a wrapper runs its checks through these, the device check (`on_gpu`) last, and only then calls
`_lib` -- the size functions included.  Imports torch and ctypes only, so it loads without the library."""
from __future__ import annotations

import ctypes as C

import torch


def _names(dtype):
    return ' or '.join(str(d).replace('torch.', '') for d in (dtype if isinstance(dtype, (tuple, list)) else (dtype,)))


def _dims(shape):
    return '(%s%s)' % (', '.join(str(s) for s in shape), ',' if len(shape) == 1 else '')


def tensor_arg(who, name, x, dtype, shape, device=None, optional=False, empty_ok=False):
    """x must be a non-empty contiguous tensor of `dtype` (one, or a tuple of allowed ones) and `shape`: a tuple of ints (exact
    sizes) and strings (free dimensions, each >= 1), on `device` when given -> the sizes of the free dimensions, in order; None for
    the None that `optional` allows.  empty_ok: a free dimension may be 0 (where the library's size function is the judge of sizes)"""
    if x is None and optional:
        return None
    ok = (torch.is_tensor(x) and x.dtype in (dtype if isinstance(dtype, (tuple, list)) else (dtype,)) and x.dim() == len(shape)
          and all(n == s or (isinstance(s, str) and (n >= 1 or empty_ok)) for n, s in zip(x.shape, shape))
          and (device is None or x.device == device) and x.is_contiguous())
    if not ok:
        where = '' if device is None else ' on %s' % (device,)
        got = 'a %s' % type(x).__name__   # (no tensor)
        if torch.is_tensor(x):
            got = '%s %s%s%s' % (_names(x.dtype), tuple(x.shape), where and ' on %s' % (x.device,),
                                 '' if x.is_contiguous() else ' with strides %s' % (tuple(x.stride()),))
        raise ValueError('%s: %s must be a contiguous %s tensor of shape %s%s, got %s' % (who, name, _names(dtype), _dims(shape), where, got))
    return tuple(n for n, s in zip(x.shape, shape) if isinstance(s, str))


def int_arg(who, name, v, lo=None, hi=None) -> int:
    """v as an int: no bool, nothing with a fraction (or that int() cannot take), nothing outside [lo, hi]"""
    try:
        ok = not isinstance(v, bool) and int(v) == v and (lo is None or int(v) >= lo) and (hi is None or int(v) <= hi)
    except (TypeError, ValueError, OverflowError):   # (None, text, NaN, infinity)
        ok = False
    if not ok:
        span = '' if lo is None and hi is None else ' >= %s' % lo if hi is None else ' in [%s, %s]' % ('-inf' if lo is None else lo, hi)
        raise ValueError('%s: %s must be an integer%s, got %r' % (who, name, span, v))
    return int(v)


def float_arg(who, name, v, lo, hi) -> float:
    """v as a float in [lo, hi]: no bool, nothing float() cannot take, no NaN"""
    try:
        x = float(v)
        ok = not isinstance(v, bool) and lo <= x <= hi   # (NaN fails both comparisons)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%s: %s must be a number in [%s, %s], got %r' % (who, name, lo, hi, v))
    return x


def unit_interval(x, what) -> float:
    """x as a float in [0, 1) that is still below 1 as a float32, or ValueError"""
    x = float(x)
    if not 0.0 <= x < 1.0:   # (NaN fails both comparisons)
        raise ValueError('%s must be in [0, 1), got %r' % (what, x))
    if C.c_float(x).value >= 1.0:
        raise ValueError('%s %r rounds to 1 in float32' % (what, x))
    return x


def host_int32(x, n, what):
    """a host sequence of n integers that fit int32 -> a list of ints, or ValueError"""
    if torch.is_tensor(x):
        if x.device.type != 'cpu' or x.dtype.is_floating_point or x.dtype == torch.bool:
            raise ValueError('%s must be integers in host memory, got a %s tensor on %s' % (what, x.dtype, x.device))
        x = x.tolist()
    try:
        x = list(x)
    except TypeError:
        raise ValueError('%s must be a sequence of %d integers, got %r' % (what, n, x)) from None
    if len(x) != n:
        raise ValueError('%s must hold %d integers, got %d' % (what, n, len(x)))
    for v in x:
        try:
            ok = not isinstance(v, bool) and int(v) == v and -(1 << 31) <= int(v) < (1 << 31)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('%s must hold integers that fit int32, got %r' % (what, v))
    return [int(v) for v in x]


def own_or_given(given, shape, dtype, device, what):
    """a fresh torch.empty tensor, or the caller's buffer after a shape / dtype / device check"""
    if given is None:
        return torch.empty(*shape, dtype=dtype, device=device)
    if tuple(given.shape) != tuple(shape) or given.dtype != dtype or given.device != device or not given.is_contiguous():
        raise ValueError('%s: expected a contiguous %s tensor of shape %s on %s' % (what, dtype, tuple(shape), device))
    return given


def no_overlap(who, name_in, t_in, name_out, t_out, span_in=None):
    """the bytes of t_out (None: nothing to check) may not meet those of t_in: span_in of them when given (a strided view), else
    its numel() elements from data_ptr() on"""
    if t_out is None:
        return
    i0, o0 = t_in.data_ptr(), t_out.data_ptr()
    i1 = i0 + (t_in.numel() * t_in.element_size() if span_in is None else span_in)
    if o0 < i1 and i0 < o0 + t_out.numel() * t_out.element_size():
        raise ValueError('%s: %s may not overlap %s' % (who, name_out, name_in))


def on_gpu(who, name, dev):
    """the last check of a wrapper: the ones in front of it are the same for tensors of any device"""
    if dev.type != 'cuda':
        raise ValueError('%s: %s must be on the GPU, got %s (there is no CPU fallback)' % (who, name, dev))


def step_q_arg(who, step_q, B, dev, lo, hi, what, name='step_q'):
    """The step_q of frames_stretch / frames_pitch (`name`: what the wrapper calls it) -> (step_q for the library, the smallest step
    the host knows of):
    None -> (None, None); a (B) int32 tensor on `dev` (a device), shape-checked and never read -> (it, lo); an int (the whole batch)
    or a host sequence of B ints, each checked against [lo, hi] (`what` says what that range means) and uploaded -> (tensor, min)"""
    if step_q is None:
        return None, None
    if torch.is_tensor(step_q) and step_q.device.type != 'cpu':
        tensor_arg(who, name + ' on a device', step_q, torch.int32, (B,), dev)
        return step_q, lo
    one = not torch.is_tensor(step_q) and not hasattr(step_q, '__len__')
    host = host_int32([step_q] * B if one else step_q, B, '%s: %s' % (who, name))
    if min(host) < lo or max(host) > hi:
        raise ValueError('%s: %s must be in [%d, %d] (%s), got %r' % (who, name, lo, hi, what, step_q if one else host))
    return torch.tensor(host, dtype=torch.int32).to(dev), min(host)


def pow2_bins(who, C_bins):
    if not 9 <= C_bins <= 1025 or (C_bins - 1) & (C_bins - 2):
        raise ValueError('%s: C - 1 must be a power of two in [8, 1024], got C = %d' % (who, C_bins))

