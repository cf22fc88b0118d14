"""ctypes binding of libtaco_hip.so (include/taco_hip.h).

PyTorch is used only as the device allocator / stream owner: every call passes raw device pointers
(`tensor.data_ptr()`) and the current HIP stream.  There is NO CPU fallback: if the shared library is missing
the import of this module raises, and every entry point raises `TacoError` on a non-zero return code.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os

# HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  One train step uses the caller's
# stream, the library's side stream, the weight-gradient stream and -- data parallel -- a communication stream plus RCCL's own:
# with 4 queues two of them share a queue and one's kernels sit behind a millisecond of the other's already-enqueued launches
# (measured in round 4: the post-net segment's collective finished 1.47 ms after it became eligible, 30 us with 8 queues).
# The variable is read when the HIP runtime initialises, i.e. at the first device call -- set it before anything touches the GPU.
from . import QUEUES_SET_BY_USER as _QUEUES_SET_BY_USER, TORCH_IMPORTED_FIRST as _TORCH_IMPORTED_FIRST   # (package __init__ applied the default)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from .argcheck import (float_arg, int_arg, no_overlap, on_gpu, pow2_bins, step_q_arg, tensor_arg,   # noqa: E402
                       host_int32 as _host_int32, own_or_given as _own_or_given, unit_interval as _unit_interval)

# If the process may have touched the GPU before importing this package (and did not set the variable itself) the runtime is up
# with its default of 4 queues: the default came too late, and high-priority communication streams would then cost 1.3 ms per
# step instead of saving one (dist._comm_priority asks here).  "May have": the runtime reads the variable at the FIRST HIP API call
# -- hipGetDeviceCount behind torch.cuda.is_available() / device_count() counts, and leaves no trace in torch
# (torch.cuda.is_initialized() stays False) -- so every import of torch ahead of this package is treated as late.
# Launchers that import torch first set the variable themselves before doing so (bench.py, tests/conftest.py, the drivers).
HW_QUEUES_LATE = (not _QUEUES_SET_BY_USER) and (_TORCH_IMPORTED_FIRST or (torch.cuda.is_available() and torch.cuda.is_initialized()))


def effective_hw_queues() -> int:
    """Hardware queues the HIP runtime of this process multiplexes its streams onto, as far as the host can know."""
    if HW_QUEUES_LATE:
        return 4
    try:
        return int(os.environ.get('GPU_MAX_HW_QUEUES', '4'))
    except ValueError:
        return 4

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TACO_LIB') or os.path.join(_HERE, 'libtaco_hip.so')   # TACO_LIB: an alternative build (tuning A/B)


class TacoError(RuntimeError):
    pass


class TacoShape(C.Structure):
    _fields_ = [('B', C.c_int32), ('Tt', C.c_int32), ('Td', C.c_int32), ('r', C.c_int32), ('V', C.c_int32),
                ('S', C.c_int32)]

    def __repr__(self):
        return 'TacoShape(B=%d, Tt=%d, Td=%d, r=%d, V=%d, S=%d)' % (self.B, self.Tt, self.Td, self.r, self.V, self.S)


class TacoTensorInfo(C.Structure):
    _fields_ = [('name', C.c_char * 64), ('offset', C.c_int64), ('size', C.c_int64), ('ndim', C.c_int32),
                ('dims', C.c_int32 * 4)]


class TacoStopRule(C.Structure):
    """Inference end detection (include/taco_hip.h): the row's length is fixed once the alignment argmax has stayed at or past
    character L - 1 - end_offset for `hold` consecutive steps and at least `min_steps` steps have run; rounded up to 4 steps."""
    _fields_ = [('end_offset', C.c_int32), ('hold', C.c_int32), ('min_steps', C.c_int32), ('reserved', C.c_int32)]

    def __init__(self, end_offset=1, hold=4, min_steps=8):
        super().__init__(int(end_offset), int(hold), int(min_steps), 0)

    def __repr__(self):
        return 'TacoStopRule(end_offset=%d, hold=%d, min_steps=%d)' % (self.end_offset, self.hold, self.min_steps)


if not os.path.exists(LIB_PATH):
    raise ImportError(
        'tacotron_amd: %s not found -- build it with `python -c "import __graft_entry__ as g; g.build()"` '
        '(or tacotron_amd/csrc/build.sh).  There is no CPU fallback.' % LIB_PATH)

_lib = C.CDLL(LIB_PATH)

_P = C.c_void_p
_I = C.c_int
_SH = C.POINTER(TacoShape)
_INT_MAX = (1 << 31) - 1   # the largest value an `int` argument of the C ABI holds

EXPORTS = {
    'taco_version': (C.c_int, []),
    'taco_last_error_string': (C.c_char_p, []),
    'taco_param_count': (C.c_int64, [_SH]),
    'taco_param_table': (C.c_int, [_SH, C.POINTER(TacoTensorInfo), _I]),
    'taco_workspace_bytes': (C.c_int64, [_SH, _I]),
    'taco_workspace_table': (C.c_int, [_SH, _I, C.POINTER(TacoTensorInfo), _I]),
    'taco_conv_gemm': (C.c_int, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'taco_debug_gemm2_window': (C.c_int, [_I, _I]),
    'taco_debug_weight_image': (C.c_int64, [_P, _I, _I, _I, _I, _P, C.c_int64, _P]),
    'taco_debug_conv_gemm_nld': (C.c_int, [_P, _I, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    'taco_debug_conv_gemm_ksplit': (C.c_int, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, C.c_int64, _P]),
    'taco_gemm_tn': (C.c_int, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'taco_debug_gemm_naive': (C.c_int, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    'taco_bigru_fwd': (C.c_int, [_P] * 12 + [_I, _I, _P]),
    'taco_debug_bigru_rec_fwd': (C.c_int, [_P] * 8 + [_I, _I, _P]),
    'taco_debug_bigru_bwd': (C.c_int, [_P] * 11 + [_I, _I, _P]),
    'taco_debug_highway_stack_fwd': (C.c_int, [_P] * 10 + [_I, _I, _I, _P]),
    'taco_debug_highway_stack_bwd': (C.c_int, [_P] * 8 + [_I, _I, _P]),
    'taco_debug_prenet_fwd': (C.c_int, [_P] * 9 + [_I, _P]),
    'taco_debug_prenet_bwd': (C.c_int, [_P] * 10 + [_I, _P]),
    'taco_debug_conv_bank_pool_fwd': (C.c_int, [_P, _I, _P, _P, _P, _P, C.c_float, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'taco_debug_conv_gemm_pool_bwd': (C.c_int, [_P, _I, _P, _I, _P, _P, _P, C.c_float, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'taco_debug_bn_maxpool_fwd': (C.c_int, [_P] * 4 + [_I, _I, _I, _P]),
    'taco_debug_bn_maxpool_bwd': (C.c_int, [_P] * 7 + [_I, _I, _I, _P]),
    'taco_debug_bank_gather': (C.c_int, [_P, _I, _P, _P, _I, _P, _I, _P, C.c_int64, _I, _I, _I, _I, _I, _I, _I, _P]),
    'taco_debug_conv_gemm_batch_atomic': (C.c_int, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    'taco_debug_conv_gemm_rowbias': (C.c_int, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    'taco_debug_gemm_tn_group': (C.c_int, [_I] + [_P] * 13 + [_P]),
    'taco_debug_gemm_tn_strided': (C.c_int, [_P, _I, C.c_int64, _P, _I, C.c_int64, _P, _I, C.c_int64, _I, _I, _I, _I, _I, _I, _P]),
    'taco_debug_embedding': (C.c_int, [_P, _P, _P, _I, _I, _I, _P]),
    'taco_debug_embedding_bwd': (C.c_int, [_P, _P, _P, _I, _I, _I, _P]),
    'taco_debug_highway_combine': (C.c_int, [_P, _P, _P, _I, _P]),
    'taco_debug_highway_combine_bwd': (C.c_int, [_P] * 5 + [_I, _P]),
    'taco_debug_act_bwd': (C.c_int, [_P, _P, _P, _P, C.c_int64, _I, _P]),
    'taco_debug_affine_act_bwd': (C.c_int, [_P] * 6 + [_I, _I, _I, _P]),
    'taco_debug_colsum_batched': (C.c_int, [_P, _I, _P, _I, _I, _I, _P]),
    'taco_debug_mask_rows': (C.c_int, [_P, _P, _P, _I, _I, _I, _P]),
    'taco_debug_center_rows': (C.c_int, [_P, _P, _P, _I, _I, _I, _P]),
    'taco_debug_mask_pos': (C.c_int, [_P, _I, _P, _I, _I, _I, C.c_float, _P]),
    'taco_debug_zero_tail_rows': (C.c_int, [_P, _I, _P, _I, _P, _I, _I, _P]),
    'taco_debug_add': (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    'taco_debug_l1_loss': (C.c_int, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    'taco_debug_transpose_batch': (C.c_int, [_I] + [_P] * 7 + [_P]),
    'taco_debug_sumsq': (C.c_int, [_P, C.c_int64, _P, _P]),
    'taco_forward': (C.c_int, [_SH] + [_P] * 17),
    'taco_backward': (C.c_int, [_SH] + [_P] * 14),
    'taco_infer': (C.c_int, [_SH] + [_P] * 9),
    'taco_infer_stop': (C.c_int, [_SH, _P, _P, _P, _P, C.POINTER(TacoStopRule), _P, _P, _P, _P, _P, _P]),
    'taco_alignment_scores': (C.c_int, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    'taco_alignment_path_workspace_bytes': (C.c_int64, [_I, _I, _I]),
    'taco_alignment_path': (C.c_int, [_P, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    'taco_frames_active': (C.c_int, [_P, C.c_float, _P, _I, _I, _I, _P]),
    'taco_frame_dtw_workspace_bytes': (C.c_int64, [_I, _I, _I, _I]),
    'taco_frame_dtw': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'taco_frame_dtw_path_workspace_bytes': (C.c_int64, [_I, _I, _I, _I]),
    'taco_frame_dtw_path': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'taco_path_f0_scores': (C.c_int, [_P, _P, _P, _P, _P, C.c_float, _P, _P, _I, _I, _I, _P]),
    'taco_clip_adam_step': (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_int64, _P, _P, _P]),
    'taco_clip_adam_step_guarded': (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, C.c_int64, _P, _P, _P, _P]),
    'taco_clear_error': (C.c_int, [_SH, _I, _P, _P]),
    'taco_grad_segments': (C.c_int, [_SH, C.POINTER(C.c_int64)]),
    'taco_wait_grad_segment': (C.c_int, [_I, _P]),
    'taco_decoder_mode': (C.c_int, [_I]),
    'taco_debug_spin': (C.c_int, [_I, _I, _I, _I, _P]),
    'taco_debug_clock_probe': (C.c_int, [_P, _I, _P]),
    'taco_debug_fabric_probe': (C.c_int, [_P, _P, _P, C.c_int64, _I, _P]),
    'taco_denorm_unframe': (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'taco_frames_stretch': (C.c_int, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    'taco_frames_pitch': (C.c_int, [_P, _P, _I, _P, _I, _P, _I, _I, _I, _P]),
    'taco_path_curve': (C.c_int, [_P, _P, _I, C.c_int32, _P, _I, _I, _I, _P]),
    'taco_frames_stretch_curve': (C.c_int, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    'taco_frames_pitch_curve': (C.c_int, [_P, _P, _I, _P, _I, _P, _I, _I, _I, _P]),
    'taco_frames_sharpen': (C.c_int, [_P, _P, _I, C.c_float, _I, _P, _I, _I, _I, _P]),
    'taco_frames_formant': (C.c_int, [_P, _P, _I, _P, _I, _P, _I, _I, _I, _P]),
    'taco_frames_cepstats_workspace_bytes': (C.c_int64, [_I, _I, _I, _I]),
    'taco_frames_cepstats': (C.c_int, [_P, _P, _I, _I, _P, _P, _P, _I, _I, _I, _P]),
    'taco_frames_f0': (C.c_int, [_P, _P, _I, _P, _P, _I, _I, C.c_float, C.c_float, _P, _P, _P, _I, _I, _I, _P]),
    'taco_f0_stats': (C.c_int, [_P, _P, _P, _I, _P, _I, _I, _P]),
    'taco_f0_range_curve': (C.c_int, [_P, _P, _I, _P, _P, _I, C.c_float, _P, _P, _I, _I, _P]),
    'taco_f0_viterbi_workspace_bytes': (C.c_int64, [_I, _I, _I, _I]),
    'taco_f0_viterbi': (C.c_int, [_P, _P, _I, _P, _P, _I, _I, _I, C.c_float, C.c_float, C.c_float, _P, _P, _P, _P, _P, _I, _I, _P]),
    'taco_corpus_batch': (C.c_int, [_P, _I, _P, _P, _P, _P, _P, C.c_int64, _I, C.c_int64, _I, _P]),
    'taco_griffinlim_workspace_bytes': (C.c_int64, [_I, _I]),
    'taco_griffinlim': (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _P]),
    'taco_griffinlim_rows_workspace_bytes': (C.c_int64, [_I, _I]),
    'taco_griffinlim_rows': (C.c_int, [_P, _P, C.c_uint64, _P, _I, _P, _P, _I, _I, _I, _P]),
    'taco_griffinlim_fast_workspace_bytes': (C.c_int64, [_I, _I]),
    'taco_griffinlim_fast': (C.c_int, [_P, _P, C.c_uint64, _P, _I, C.c_float, _P, _P, _P, _I, _I, _I, _P]),
    'taco_phase_estimate_workspace_bytes': (C.c_int64, [_I, _I]),
    'taco_phase_estimate': (C.c_int, [_P, _P, _I, _P, _P, _I, _I, _P]),
    'taco_wave_finish_workspace_bytes': (C.c_int64, [_I, _I]),
    'taco_wave_finish': (C.c_int, [_P, _P, C.c_float, C.c_float, _P, _P, _P, _P, _P, _I, _I, _P]),
    'taco_wave_join_workspace_bytes': (C.c_int64, [_I, _I, _I]),
    'taco_wave_join': (C.c_int, [_P, C.c_int64, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I,
                                 _P]),
    'taco_k_weighting': (C.c_int, [_I, C.POINTER(C.c_double)]),
    'taco_wave_loudness_workspace_bytes': (C.c_int64, [_I, _I, _I]),
    'taco_wave_loudness': (C.c_int, [_P, _P, _I, C.c_float, C.c_float, _P, _P, _P, _P, _P, _I, _I, _P]),
    'taco_wave_limit_workspace_bytes': (C.c_int64, [_I, _I, _I]),
    'taco_wave_limit': (C.c_int, [_P, _P, _P, C.c_float, _P, _I, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P]),
    'taco_audio_features_workspace_bytes': (C.c_int64, [_I, _I]),
    'taco_audio_features': (C.c_int, [_P, C.POINTER(C.c_int32), _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'taco_wave_resample': (C.c_int, [_P, C.c_int64, _I, _I, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    'taco_fill_bernoulli': (C.c_int, [_P, C.c_int64, C.c_float, C.c_uint64, _P]),
    'taco_tensor_stats_plan_bytes': (C.c_int64, [C.POINTER(C.c_int64), _I]),
    'taco_tensor_stats_plan': (C.c_int, [C.POINTER(C.c_int64), _I, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int32)]),
    'taco_tensor_stats_workspace_bytes': (C.c_int64, [_I, _I, _I]),
    'taco_tensor_stats': (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    'taco_param_ema_workspace_bytes': (C.c_int64, [C.c_int64]),
    'taco_param_ema': (C.c_int, [_P, _P, C.c_int64, C.c_float, _P, _P, _P, _P]),
    'taco_profile_enable': (C.c_int, [_I]),
    'taco_debug_last_cluster': (C.c_int, [_I]),
    'taco_profile_read': (C.c_int, [_I, C.POINTER(C.c_float), _I]),
    'taco_debug_profile_labels': (C.c_int, [_I, C.c_char_p, _I]),
    'taco_profile_read2': (C.c_int, [_I, C.POINTER(C.c_float), C.POINTER(C.c_double), _I]),
}
for _name, (_res, _args) in EXPORTS.items():
    _fn = getattr(_lib, _name)  # AttributeError here = the library does not export what include/taco_hip.h declares
    _fn.restype = _res
    _fn.argtypes = _args


def last_error() -> str:
    return _lib.taco_last_error_string().decode()


def _check(rc: int, what: str):
    if rc != 0:
        raise TacoError('%s failed (rc=%d): %s' % (what, rc, last_error()))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), 'taco: tensor must be contiguous'
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_shape(B, Tt, Td, r, V, S=1) -> TacoShape:
    """S = num_speakers (<= 1: single-speaker model, no speaker path)."""
    return TacoShape(int(B), int(Tt), int(Td), int(r), int(V), int(S))


def version() -> int:
    return _lib.taco_version()


def _size(fn_name, *args) -> int:
    """What a size function of the library returns (a TacoShape goes by reference), or TacoError when it refuses its arguments."""
    n = getattr(_lib, fn_name)(*[C.byref(a) if isinstance(a, TacoShape) else int(a) for a in args])
    if n < 0:
        raise TacoError('%s(%s): bad arguments (rc=%d)' % (fn_name, ', '.join(repr(a) for a in args), n))
    return n


def param_count(shape: TacoShape) -> int:
    return _size('taco_param_count', shape)


def _table(fn, *args):
    n = fn(*args, None, 0)
    if n < 0:
        raise TacoError(last_error())
    rows = (TacoTensorInfo * n)()
    fn(*args, rows, n)
    return [(r.name.decode(), int(r.offset), int(r.size), tuple(r.dims[i] for i in range(r.ndim))) for r in rows]


def param_table(shape: TacoShape):
    """[(name, offset_floats, size_floats, dims)] in TF variable order."""
    return _table(_lib.taco_param_table, C.byref(shape))


def workspace_bytes(shape: TacoShape, train: bool) -> int:
    return _size('taco_workspace_bytes', shape, train)


def workspace_table(shape: TacoShape, train: bool):
    return _table(_lib.taco_workspace_table, C.byref(shape), int(train))


def conv_gemm(A, W, C_out, M, N, K, taps=1, T=None, pad_l=0, act=0, bias=None, scale=None, shift=None, residual=None,
              keep=None, Cpre=None, lda=None, ldw=None, ldc=None, ldr=None):
    T = M if T is None else T
    _check(_lib.taco_conv_gemm(ptr(A), lda or K, ptr(W), ldw or N, ptr(bias), ptr(scale), ptr(shift), ptr(residual),
                               ldr or N, ptr(keep), ptr(C_out), ldc or N, ptr(Cpre), M, N, K, taps, T, pad_l, act,
                               stream_ptr()), 'taco_conv_gemm')


def debug_gemm2_window(lo, hi):
    return int(_lib.taco_debug_gemm2_window(lo, hi))


def conv_gemm_nld(A, W, C_out, M, N, K, nld, ldw, ldc, act=0, bias=None):
    _check(_lib.taco_debug_conv_gemm_nld(ptr(A), K, ptr(W), ldw, nld, ptr(bias), ptr(C_out), ldc, M, N, K, act, stream_ptr()),
           'taco_debug_conv_gemm_nld')


def conv_gemm_ksplit(A, W, C_out, M, N, K, slabs, taps=1, T=None, pad_l=0, act=0, bias=None):
    T = M if T is None else T
    _check(_lib.taco_debug_conv_gemm_ksplit(ptr(A), K, ptr(W), N, ptr(bias), ptr(C_out), N, M, N, K, taps, T, pad_l, act,
                                            ptr(slabs), slabs.numel(), stream_ptr()), 'taco_debug_conv_gemm_ksplit')


def gemm_tn(A, dY, dW, M, N, K, taps=1, T=None, pad_l=0, accumulate=False, lda=None, ldy=None, ldw=None):
    T = M if T is None else T
    _check(_lib.taco_gemm_tn(ptr(A), lda or K, ptr(dY), ldy or N, ptr(dW), ldw or N, M, N, K, taps, T, pad_l,
                             int(accumulate), stream_ptr()), 'taco_gemm_tn')


def weight_image_bytes(W, taps, K, N, ldw=None):
    need = _lib.taco_debug_weight_image(ptr(W), ldw or N, taps, K, N, None, 0, None)
    if need < 0:
        raise TacoError('taco_debug_weight_image: %d' % need)
    return int(need)


def weight_image(W=None, taps=1, K=0, N=0, ldw=None, img=None):
    """Op-level door to the pre-split weight images (include/taco_hip.h taco_debug_weight_image).  W None: clear this thread's
    table.  Otherwise builds and registers the bf16 plane image of W (taps, K, N) and returns the image tensor (keep it alive).
    img: the caller's own buffer of at least weight_image_bytes(...) bytes (16-byte aligned) instead of a fresh one."""
    if W is None:   # -> launches that ran the image form since the previous clear
        return int(_lib.taco_debug_weight_image(None, 0, 0, 0, 0, None, 0, None))
    ldw = ldw or N
    need = _lib.taco_debug_weight_image(ptr(W), ldw, taps, K, N, None, 0, None)
    if need < 0:
        raise TacoError('taco_debug_weight_image: %d' % need)
    if img is None:
        img = torch.empty(need // 2, dtype=torch.int16, device=W.device)
    assert img.numel() * img.element_size() >= need and img.data_ptr() % 16 == 0, 'taco: weight image buffer too small or misaligned'
    rc = _lib.taco_debug_weight_image(ptr(W), ldw, taps, K, N, ptr(img), need, stream_ptr())
    _check(int(rc), 'taco_debug_weight_image')
    return img


def debug_gemm_naive(A, W, C_out, M, N, K, taps=1, T=None, pad_l=0, act=0, bias=None):
    T = M if T is None else T
    _check(_lib.taco_debug_gemm_naive(ptr(A), K, ptr(W), N, ptr(bias), ptr(C_out), N, M, N, K, taps, T, pad_l, act,
                                      stream_ptr()), 'taco_debug_gemm_naive')


def bigru_fwd(x, w, xg, out, ruc, B, T):
    """w: dict with fw/bw gates/candidate kernels and biases (TF layout)."""
    _check(_lib.taco_bigru_fwd(ptr(x), ptr(w['fw/gates/kernel']), ptr(w['fw/gates/bias']),
                               ptr(w['fw/candidate/kernel']), ptr(w['fw/candidate/bias']),
                               ptr(w['bw/gates/kernel']), ptr(w['bw/gates/bias']),
                               ptr(w['bw/candidate/kernel']), ptr(w['bw/candidate/bias']),
                               ptr(xg), ptr(out), ptr(ruc), B, T, stream_ptr()), 'taco_bigru_fwd')


# ---- op-level debug doors of the CBHG tail (include/taco_hip.h; tests/test_gpu_cbhg_tail.py) ----
DOOR_MAX_ROWS = 1 << 24          # B * T resp. M of the bi-GRU and highway doors
DOOR_MAX_PRENET_ROWS = 1 << 22   # M of the pre-net doors


def _disjoint(who, ins, outs):
    """no output (name, tensor or None) may meet an input or another output"""
    outs = [(n, t) for n, t in outs if t is not None]
    ins = [(n, t) for n, t in ins if t is not None]
    for i, (n_out, t_out) in enumerate(outs):
        for n_in, t_in in ins + outs[i + 1:]:
            no_overlap(who, n_in, t_in, n_out, t_out)


def _layer_table(who, name, ts, nl, shape, dev, dtype=torch.float32):
    """a list of nl tensors of one shape -> ([(name[l], tensor)], the table of 4 pointers the C ABI takes)"""
    if not isinstance(ts, (list, tuple)) or len(ts) != nl:
        raise ValueError('%s: %s must be a list of %d tensors (one per layer), got %s'
                         % (who, name, nl, '%d' % len(ts) if isinstance(ts, (list, tuple)) else 'a %s' % type(ts).__name__))
    named = [('%s[%d]' % (name, l), t) for l, t in enumerate(ts)]
    for n, t in named:
        tensor_arg(who, n, t, dtype, shape, dev)
    return named, (C.c_void_p * 4)(*([t.data_ptr() for t in ts] + [None] * (4 - nl)))


def debug_bigru_rec_fwd(xg, w, out, ruc=None, h0=None):
    """The bi-GRU's forward recurrence alone (taco_debug_bigru_rec_fwd): xg (B, T, 768) the x-side pre-activations with their biases,
    w the GRUCell kernels by the names bigru_fwd uses ('fw/gates/kernel' (256, 256), 'fw/candidate/kernel' (256, 128), 'bw/..'),
    h0 (B, 128) or None -> out (B, T, 256), ruc (B, T, 768) or None, the caller's buffers."""
    who = 'debug_bigru_rec_fwd'
    B, T = tensor_arg(who, 'xg', xg, torch.float32, ('B', 'T', 768))
    dev = xg.device
    if B * T > DOOR_MAX_ROWS:
        raise ValueError('%s: at most %d rows, got B * T = %d' % (who, DOOR_MAX_ROWS, B * T))
    ws = []
    for d in ('fw', 'bw'):
        for part, cols in (('gates', 256), ('candidate', 128)):
            k = '%s/%s/kernel' % (d, part)
            tensor_arg(who, 'w[%r]' % k, w.get(k), torch.float32, (256, cols), dev)
            ws.append(('w[%r]' % k, w[k]))
    tensor_arg(who, 'h0', h0, torch.float32, (B, 128), dev, optional=True)
    tensor_arg(who, 'out', out, torch.float32, (B, T, 256), dev)
    tensor_arg(who, 'ruc', ruc, torch.float32, (B, T, 768), dev, optional=True)
    _disjoint(who, [('xg', xg), ('h0', h0)] + ws, [('out', out), ('ruc', ruc)])
    on_gpu(who, 'xg', dev)
    _check(_lib.taco_debug_bigru_rec_fwd(ptr(xg), ptr(ws[0][1]), ptr(ws[1][1]), ptr(ws[2][1]), ptr(ws[3][1]), ptr(h0), ptr(out), ptr(ruc),
                                         B, T, stream_ptr()), 'taco_debug_bigru_rec_fwd')


def debug_bigru_bwd(dout, out, ruc, wT, dxg, rh, h0=None, dh0=None):
    """The bi-GRU's backward recurrence alone (taco_debug_bigru_bwd): dout, out (B, T, 256), ruc (B, T, 768), wT the transposed h-side
    kernels {'fw/wghT': (256, 128), 'fw/wchT': (128, 128), 'bw/..'}, h0 (B, 128) or None -> dxg (B, T, 768), rh (B, T, 256), dh0
    (2, B, 128) or None, the caller's buffers."""
    who = 'debug_bigru_bwd'
    B, T = tensor_arg(who, 'dout', dout, torch.float32, ('B', 'T', 256))
    dev = dout.device
    if B * T > DOOR_MAX_ROWS:
        raise ValueError('%s: at most %d rows, got B * T = %d' % (who, DOOR_MAX_ROWS, B * T))
    tensor_arg(who, 'out', out, torch.float32, (B, T, 256), dev)
    tensor_arg(who, 'ruc', ruc, torch.float32, (B, T, 768), dev)
    ws = []
    for d in ('fw', 'bw'):
        for part, rows in (('wghT', 256), ('wchT', 128)):
            k = '%s/%s' % (d, part)
            tensor_arg(who, 'wT[%r]' % k, wT.get(k), torch.float32, (rows, 128), dev)
            ws.append(('wT[%r]' % k, wT[k]))
    tensor_arg(who, 'h0', h0, torch.float32, (B, 128), dev, optional=True)
    tensor_arg(who, 'dxg', dxg, torch.float32, (B, T, 768), dev)
    tensor_arg(who, 'rh', rh, torch.float32, (B, T, 256), dev)
    tensor_arg(who, 'dh0', dh0, torch.float32, (2, B, 128), dev, optional=True)
    _disjoint(who, [('dout', dout), ('out', out), ('ruc', ruc), ('h0', h0)] + ws, [('dxg', dxg), ('rh', rh), ('dh0', dh0)])
    on_gpu(who, 'dout', dev)
    _check(_lib.taco_debug_bigru_bwd(ptr(dout), ptr(out), ptr(ruc), ptr(ws[0][1]), ptr(ws[1][1]), ptr(ws[2][1]), ptr(ws[3][1]), ptr(h0),
                                     ptr(dxg), ptr(rh), ptr(dh0), B, T, stream_ptr()), 'taco_debug_bigru_bwd')


def debug_highway_stack_fwd(x, wt, bt, wh, bh, y, th=None, wa=None, rowb=None, hx=None, T=None):
    """The highway stack's forward launch (taco_debug_highway_stack_fwd): x (M, 128); wt, bt, wh, bh, y (and th, or None: no stash)
    lists of nl = len(y) tensors, nl in 1..4.  Adapter form: wa, rowb, hx lists of 4 and T, the rows per sequence."""
    who = 'debug_highway_stack_fwd'
    M, = tensor_arg(who, 'x', x, torch.float32, ('M', 128))
    dev = x.device
    if M > DOOR_MAX_ROWS:
        raise ValueError('%s: at most %d rows, got M = %d' % (who, DOOR_MAX_ROWS, M))
    nl = int_arg(who, 'nl (the length of y)', len(y) if isinstance(y, (list, tuple)) else None, 1, 4)
    ins, outs, tabs = [('x', x)], [], {}
    for name, ts, shape, is_out in (('wt', wt, (128, 128), 0), ('bt', bt, (128,), 0), ('wh', wh, (128, 128), 0), ('bh', bh, (128,), 0),
                                    ('th', th, (M, 256), 1), ('y', y, (M, 128), 1)):
        if ts is None and name == 'th':
            tabs[name] = None
            continue
        named, tabs[name] = _layer_table(who, name, ts, nl, shape, dev)
        (outs if is_out else ins).extend(named)
    ad = wa is not None
    if ad:
        if nl != 4:
            raise ValueError('%s: the adapter form has 4 layers, got nl = %d' % (who, nl))
        T = int_arg(who, 'T', T, 1, M)
        if M % T:
            raise ValueError('%s: T must divide M, got T = %d, M = %d' % (who, T, M))
        for name, ts, shape, is_out in (('wa', wa, (128, 128), 0), ('rowb', rowb, (M // T, 128), 0), ('hx', hx, (M, 128), 1)):
            named, tabs[name] = _layer_table(who, name, ts, 4, shape, dev)
            (outs if is_out else ins).extend(named)
    elif rowb is not None or hx is not None:
        raise ValueError('%s: rowb and hx belong to the adapter form, which wa selects' % who)
    _disjoint(who, ins, outs)
    on_gpu(who, 'x', dev)
    _check(_lib.taco_debug_highway_stack_fwd(ptr(x), tabs['wt'], tabs['bt'], tabs['wh'], tabs['bh'], tabs['th'], tabs['y'], tabs.get('wa'),
                                             tabs.get('rowb'), tabs.get('hx'), M, nl, T if ad else 0, stream_ptr()),
           'taco_debug_highway_stack_fwd')


def debug_highway_stack_bwd(g, wT, th, x, dth, gout, waT=None, dhx=None):
    """The highway stack's backward launch (taco_debug_highway_stack_bwd): g (M, 128); wT (256, 128), th (M, 256), x (M, 128), dth
    (M, 256) lists of nl = len(dth) tensors; gout (M, 128).  Adapter form: waT (128, 128), dhx (M, 128) lists of 4."""
    who = 'debug_highway_stack_bwd'
    M, = tensor_arg(who, 'g', g, torch.float32, ('M', 128))
    dev = g.device
    if M > DOOR_MAX_ROWS:
        raise ValueError('%s: at most %d rows, got M = %d' % (who, DOOR_MAX_ROWS, M))
    nl = int_arg(who, 'nl (the length of dth)', len(dth) if isinstance(dth, (list, tuple)) else None, 1, 4)
    tensor_arg(who, 'gout', gout, torch.float32, (M, 128), dev)
    ins, outs, tabs = [('g', g)], [('gout', gout)], {}
    for name, ts, shape, is_out in (('wT', wT, (256, 128), 0), ('th', th, (M, 256), 0), ('x', x, (M, 128), 0), ('dth', dth, (M, 256), 1)):
        named, tabs[name] = _layer_table(who, name, ts, nl, shape, dev)
        (outs if is_out else ins).extend(named)
    if waT is not None:
        if nl != 4:
            raise ValueError('%s: the adapter form has 4 layers, got nl = %d' % (who, nl))
        for name, ts, shape, is_out in (('waT', waT, (128, 128), 0), ('dhx', dhx, (M, 128), 1)):
            named, tabs[name] = _layer_table(who, name, ts, 4, shape, dev)
            (outs if is_out else ins).extend(named)
    elif dhx is not None:
        raise ValueError('%s: dhx belongs to the adapter form, which waT selects' % who)
    _disjoint(who, ins, outs)
    on_gpu(who, 'g', dev)
    _check(_lib.taco_debug_highway_stack_bwd(ptr(g), tabs['wT'], tabs['th'], tabs['x'], tabs['dth'], ptr(gout), tabs.get('waT'),
                                             tabs.get('dhx'), M, nl, stream_ptr()), 'taco_debug_highway_stack_bwd')


def debug_prenet_fwd(x, w1, b1, w2, b2, y1, y2, keep1=None, keep2=None):
    """The encoder pre-net's forward launch (taco_debug_prenet_fwd): x (M, 256), w1 (256, 256), b1 (256), w2 (256, 128), b2 (128), keep1
    (M, 256) / keep2 (M, 128) uint8 or None -> y1 (M, 256), y2 (M, 128), the caller's buffers."""
    who = 'debug_prenet_fwd'
    M, = tensor_arg(who, 'x', x, torch.float32, ('M', 256))
    dev = x.device
    if M > DOOR_MAX_PRENET_ROWS:
        raise ValueError('%s: at most %d rows, got M = %d' % (who, DOOR_MAX_PRENET_ROWS, M))
    ins = [('x', x), ('w1', w1), ('b1', b1), ('w2', w2), ('b2', b2), ('keep1', keep1), ('keep2', keep2)]
    shapes = {'w1': (256, 256), 'b1': (256,), 'w2': (256, 128), 'b2': (128,), 'keep1': (M, 256), 'keep2': (M, 128)}
    for name, t in ins[1:]:
        tensor_arg(who, name, t, torch.uint8 if name.startswith('keep') else torch.float32, shapes[name], dev, optional=name[0] in 'bk')
    tensor_arg(who, 'y1', y1, torch.float32, (M, 256), dev)
    tensor_arg(who, 'y2', y2, torch.float32, (M, 128), dev)
    _disjoint(who, ins, [('y1', y1), ('y2', y2)])
    on_gpu(who, 'x', dev)
    _check(_lib.taco_debug_prenet_fwd(ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(keep1), ptr(keep2), ptr(y1), ptr(y2), M, stream_ptr()),
           'taco_debug_prenet_fwd')


def debug_prenet_bwd(dy2, w2T, w1T, y1_in, y2_in, dz2, dz1, dx, keep1=None, keep2=None):
    """The encoder pre-net's backward launch (taco_debug_prenet_bwd): dy2 (M, 128), w2T (128, 256), w1T (256, 256), the forward's y1_in
    (M, 256) and y2_in (M, 128), the keep masks or None -> dz2 (M, 128), dz1 (M, 256), dx (M, 256), the caller's buffers."""
    who = 'debug_prenet_bwd'
    M, = tensor_arg(who, 'dy2', dy2, torch.float32, ('M', 128))
    dev = dy2.device
    if M > DOOR_MAX_PRENET_ROWS:
        raise ValueError('%s: at most %d rows, got M = %d' % (who, DOOR_MAX_PRENET_ROWS, M))
    ins = [('dy2', dy2), ('w2T', w2T), ('w1T', w1T), ('y1_in', y1_in), ('y2_in', y2_in), ('keep1', keep1), ('keep2', keep2)]
    shapes = {'w2T': (128, 256), 'w1T': (256, 256), 'y1_in': (M, 256), 'y2_in': (M, 128), 'keep1': (M, 256), 'keep2': (M, 128)}
    for name, t in ins[1:]:
        tensor_arg(who, name, t, torch.uint8 if name.startswith('keep') else torch.float32, shapes[name], dev, optional=name[0] == 'k')
    outs = [('dz2', dz2), ('dz1', dz1), ('dx', dx)]
    for (name, t), cols in zip(outs, (128, 256, 256)):
        tensor_arg(who, name, t, torch.float32, (M, cols), dev)
    _disjoint(who, ins, outs)
    on_gpu(who, 'dy2', dev)
    _check(_lib.taco_debug_prenet_bwd(ptr(dy2), ptr(w2T), ptr(w1T), ptr(keep1), ptr(keep2), ptr(y1_in), ptr(y2_in), ptr(dz2), ptr(dz1),
                                      ptr(dx), M, stream_ptr()), 'taco_debug_prenet_bwd')


# ---- op-level debug doors of the GEMM forms only the model reaches (include/taco_hip.h; tests/test_gpu_gemm_forms.py) ----
# Every tensor is a FLAT contiguous float32 tensor that starts at the operand's element (0, 0) and holds at least
# (rows - 1) * pitch + cols floats; a door returns True when its form ran and False where the library falls back to another
# (TACO_ENOTFOUND: nothing was enqueued).
TACO_ENOTFOUND = -3
DOOR_MAX_GEMM_ROWS = 1 << 22
DOOR_MAX_GEMM_COLS = 1 << 14


def _span(rows, cols, ld):
    return (rows - 1) * ld + cols


def _flat_args(who, ins, outs):
    """ins, outs: [(name, tensor, floats needed, optional)] -> the device of the first input.  Each must be a flat float32 tensor
    of at least that many floats, all on one device; no output's extent may meet another operand's; the device check comes last."""
    dev = ins[0][1].device if torch.is_tensor(ins[0][1]) else None
    for name, t, need, optional in ins + outs:
        if tensor_arg(who, name, t, torch.float32, ('n',), dev, optional) is not None and t.numel() < need:
            raise ValueError('%s: %s must hold at least %d floats, got %d' % (who, name, need, t.numel()))
    live_in = [(n, t, need) for n, t, need, _ in ins if t is not None]
    live_out = [(n, t, need) for n, t, need, _ in outs if t is not None]
    for i, (n_out, t_out, need_out) in enumerate(live_out):
        for n_in, t_in, need_in in live_in + live_out[i + 1:]:
            no_overlap(who, n_in, t_in, n_out, t_out[:need_out], span_in=4 * need_in)
    on_gpu(who, ins[0][0], dev)
    return dev


def _gemm_dims(who, M, T, **cols):
    M = int_arg(who, 'M', M, 1, DOOR_MAX_GEMM_ROWS)
    T = int_arg(who, 'T', T, 1, M)
    if M % T:
        raise ValueError('%s: T must divide M, got M = %d, T = %d' % (who, M, T))
    return (M, T) + tuple(int_arg(who, k, v, 1, DOOR_MAX_GEMM_COLS) for k, v in cols.items())


def _pitch(who, name, ld, least):
    ld = int_arg(who, name, least if ld is None else ld, 1, _INT_MAX)
    if ld < least:
        raise ValueError('%s: %s must be >= %d, got %d' % (who, name, least, ld))
    return ld


def _ptr_table(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _filter_list(who, name, ts, lo=1, hi=16):
    if not isinstance(ts, (list, tuple)) or not lo <= len(ts) <= hi:
        raise ValueError('%s: %s must be a list of %d to %d tensors (one per filter width), got %s'
                         % (who, name, lo, hi, '%d' % len(ts) if isinstance(ts, (list, tuple)) else 'a %s' % type(ts).__name__))
    return len(ts)


def _door(rc, what):
    if rc == TACO_ENOTFOUND:
        return False
    _check(rc, what)
    return True


def debug_conv_bank_pool_fwd(x, W, bias, scale, shift, pool, M, T, N, K, scale_mul=1.0, bank=None, lda=None, ldc=None):
    """The conv bank with the pooled epilogue (taco_debug_conv_bank_pool_fwd): x (M, K; lda), W[f-1] (f, K, N) and bias[f-1] (N) or
    None for f = 1..F = len(W), scale / shift (F N) -> pool and, when given, bank (M, F N; ldc).  False: gemm2.hip did not take it."""
    who = 'debug_conv_bank_pool_fwd'
    F = _filter_list(who, 'W', W)
    if not isinstance(bias, (list, tuple)) or len(bias) != F:
        raise ValueError('%s: bias must be a list of %d tensors or Nones (one per filter width)' % (who, F))
    M, T, N, K = _gemm_dims(who, M, T, N=N, K=K)
    lda, ldc = _pitch(who, 'lda', lda, K), _pitch(who, 'ldc', ldc, F * N)
    ins = [('x', x, _span(M, K, lda), False)]
    ins += [('W[%d]' % f, W[f], (f + 1) * K * N, False) for f in range(F)] + [('bias[%d]' % f, bias[f], N, True) for f in range(F)]
    ins += [('scale', scale, F * N, False), ('shift', shift, F * N, False)]
    _flat_args(who, ins, [('pool', pool, _span(M, F * N, ldc), False), ('bank', bank, _span(M, F * N, ldc), True)])
    return _door(_lib.taco_debug_conv_bank_pool_fwd(ptr(x), lda, _ptr_table(W), _ptr_table(bias), ptr(scale), ptr(shift), float(scale_mul),
                                                    ptr(pool), ptr(bank), ldc, M, T, F, N, K, stream_ptr()), 'taco_debug_conv_bank_pool_fwd')


def debug_conv_gemm_pool_bwd(A, W, pool_x, scale, shift, C_out, dgamma, dbeta, M, T, N, K, taps=3, pad_l=1, scale_mul=1.0, lda=None,
                             ldw=None, ldc=None):
    """One GEMM with the backward pooled epilogue (taco_debug_conv_gemm_pool_bwd): A (M, K; lda), W (taps, K, N; ldw), pool_x (M, N;
    ldc), scale / shift (N) -> C_out (M, N; ldc); dgamma, dbeta (N) are added to.  False: the two-pass form would run."""
    who = 'debug_conv_gemm_pool_bwd'
    M, T, N, K = _gemm_dims(who, M, T, N=N, K=K)
    taps, pad_l = int_arg(who, 'taps', taps, 1, 64), int_arg(who, 'pad_l', pad_l, -64, 64)
    lda, ldw, ldc = _pitch(who, 'lda', lda, K), _pitch(who, 'ldw', ldw, N), _pitch(who, 'ldc', ldc, N)
    _flat_args(who, [('A', A, _span(M, K, lda), False), ('W', W, _span(taps * K, N, ldw), False), ('pool_x', pool_x, _span(M, N, ldc), False),
                     ('scale', scale, N, False), ('shift', shift, N, False)],
               [('C_out', C_out, _span(M, N, ldc), False), ('dgamma', dgamma, N, False), ('dbeta', dbeta, N, False)])
    return _door(_lib.taco_debug_conv_gemm_pool_bwd(ptr(A), lda, ptr(W), ldw, ptr(pool_x), ptr(scale), ptr(shift), float(scale_mul), ptr(C_out),
                                                    ldc, ptr(dgamma), ptr(dbeta), M, N, K, taps, T, pad_l, stream_ptr()),
                 'taco_debug_conv_gemm_pool_bwd')


def _bn_pool_dims(who, B, T, C_cols):
    B, T = int_arg(who, 'B', B, 1, DOOR_MAX_GEMM_ROWS), int_arg(who, 'T', T, 1, DOOR_MAX_GEMM_ROWS)
    if B * T > DOOR_MAX_GEMM_ROWS:
        raise ValueError('%s: B T must be <= %d, got %d' % (who, DOOR_MAX_GEMM_ROWS, B * T))
    C_cols = int_arg(who, 'C', C_cols, 4, DOOR_MAX_GEMM_COLS)
    if C_cols % 4:
        raise ValueError('%s: C must be a multiple of 4, got %d' % (who, C_cols))
    return B, T, C_cols


def debug_bn_maxpool_fwd(x, gamma, beta, y, B, T, C_cols):
    """The two-pass twin of the pooled forward epilogue (taco_debug_bn_maxpool_fwd): x, y dense (B T, C), gamma, beta (C)."""
    who = 'debug_bn_maxpool_fwd'
    B, T, C_cols = _bn_pool_dims(who, B, T, C_cols)
    mc = B * T * C_cols
    _flat_args(who, [('x', x, mc, False), ('gamma', gamma, C_cols, False), ('beta', beta, C_cols, False)], [('y', y, mc, False)])
    _check(_lib.taco_debug_bn_maxpool_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), B, T, C_cols, stream_ptr()), 'taco_debug_bn_maxpool_fwd')


def debug_bn_maxpool_bwd(x, gamma, beta, dy, dx, dgamma, dbeta, B, T, C_cols):
    """The two-pass twin of the pooled backward epilogue (taco_debug_bn_maxpool_bwd): x, dy, dx dense (B T, C); dgamma, dbeta (C) are
    added to."""
    who = 'debug_bn_maxpool_bwd'
    B, T, C_cols = _bn_pool_dims(who, B, T, C_cols)
    mc = B * T * C_cols
    _flat_args(who, [('x', x, mc, False), ('gamma', gamma, C_cols, False), ('beta', beta, C_cols, False), ('dy', dy, mc, False)],
               [('dx', dx, mc, False), ('dgamma', dgamma, C_cols, False), ('dbeta', dbeta, C_cols, False)])
    _check(_lib.taco_debug_bn_maxpool_bwd(ptr(x), ptr(gamma), ptr(beta), ptr(dy), ptr(dx), ptr(dgamma), ptr(dbeta), B, T, C_cols, stream_ptr()),
           'taco_debug_bn_maxpool_bwd')


def debug_bank_gather(dbank, WT, dx_out, slabs, M, T, K, N, S, residual=None, pad_l=None, lda=None, ldc=None, ldr=None):
    """The conv bank's input gradient as one reduction in S chunks + slab sum (taco_debug_bank_gather): dbank (M, F K; lda), WT[f-1]
    (f, K, N) the transposed kernels (contiguous one behind the other for the gather to run), residual (M, N; ldr) or None ->
    dx_out (M, N; ldc) is added to.  pad_l None: (F - 1) - (F - 1) // 2.  False: the library would run the atomic batch."""
    who = 'debug_bank_gather'
    F = _filter_list(who, 'WT', WT)
    M, T, N, K = _gemm_dims(who, M, T, N=N, K=K)
    S = int_arg(who, 'S', S, 1, 16)
    pad_l = int_arg(who, 'pad_l', (F - 1) - (F - 1) // 2 if pad_l is None else pad_l, -64, 64)
    lda, ldc, ldr = _pitch(who, 'lda', lda, F * K), _pitch(who, 'ldc', ldc, N), _pitch(who, 'ldr', ldr, N)
    ins = [('dbank', dbank, _span(M, F * K, lda), False)] + [('WT[%d]' % f, WT[f], (f + 1) * K * N, False) for f in range(F)]
    ins += [('residual', residual, _span(M, N, ldr), True)]
    _flat_args(who, ins, [('dx_out', dx_out, _span(M, N, ldc), False), ('slabs', slabs, slabs.numel() if torch.is_tensor(slabs) else 1, False)])
    return _door(_lib.taco_debug_bank_gather(ptr(dbank), lda, _ptr_table(WT), ptr(residual), ldr, ptr(dx_out), ldc, ptr(slabs), slabs.numel(),
                                             M, T, F, K, N, pad_l, S, stream_ptr()), 'taco_debug_bank_gather')


def debug_conv_gemm_batch_atomic(dbank, WT, dx_out, M, T, K, N, residual=None, lda=None, ldc=None, ldr=None):
    """The atomic K-problem batch, the gather's fall-back (taco_debug_conv_gemm_batch_atomic): operands as debug_bank_gather; dx_out
    is added to with fp32 atomics."""
    who = 'debug_conv_gemm_batch_atomic'
    F = _filter_list(who, 'WT', WT)
    M, T, N, K = _gemm_dims(who, M, T, N=N, K=K)
    lda, ldc, ldr = _pitch(who, 'lda', lda, F * K), _pitch(who, 'ldc', ldc, N), _pitch(who, 'ldr', ldr, N)
    ins = [('dbank', dbank, _span(M, F * K, lda), False)] + [('WT[%d]' % f, WT[f], (f + 1) * K * N, False) for f in range(F)]
    ins += [('residual', residual, _span(M, N, ldr), True)]
    _flat_args(who, ins, [('dx_out', dx_out, _span(M, N, ldc), False)])
    _check(_lib.taco_debug_conv_gemm_batch_atomic(ptr(dbank), lda, _ptr_table(WT), ptr(residual), ldr, ptr(dx_out), ldc, M, T, F, K, N,
                                                  stream_ptr()), 'taco_debug_conv_gemm_batch_atomic')


def debug_conv_gemm_rowbias(A, W, rowb, C_out, M, T, N, K, bias_stride=None, lda=None, ldw=None, ldc=None):
    """A dense layer with a per-sequence bias (taco_debug_conv_gemm_rowbias): C_out (M, N; ldc) = A (M, K; lda) . W (K, N; ldw) +
    rowb[m // T] with rowb (M // T, N; bias_stride)."""
    who = 'debug_conv_gemm_rowbias'
    M, T, N, K = _gemm_dims(who, M, T, N=N, K=K)
    lda, ldw, ldc = _pitch(who, 'lda', lda, K), _pitch(who, 'ldw', ldw, N), _pitch(who, 'ldc', ldc, N)
    bias_stride = _pitch(who, 'bias_stride', bias_stride, N)
    _flat_args(who, [('A', A, _span(M, K, lda), False), ('W', W, _span(K, N, ldw), False), ('rowb', rowb, _span(M // T, N, bias_stride), False)],
               [('C_out', C_out, _span(M, N, ldc), False)])
    _check(_lib.taco_debug_conv_gemm_rowbias(ptr(A), lda, ptr(W), ldw, ptr(rowb), bias_stride, ptr(C_out), ldc, M, T, N, K, stream_ptr()),
           'taco_debug_conv_gemm_rowbias')


def debug_gemm_tn_group(problems):
    """Up to 26 (kMaxTnBatch) weight gradients as one grouped launch (taco_debug_gemm_tn_group).  problems: a list of dicts with A (M, K;
    lda), Y (M, N; ldy), W (taps, K, N; ldw; added to), M, T, N, K, taps, pad_l and optionally dbias ((N), added to), lda, ldy, ldw."""
    who = 'debug_gemm_tn_group'
    if not isinstance(problems, (list, tuple)) or not 1 <= len(problems) <= 26:
        raise ValueError('%s: problems must be a list of 1 to 26 dicts' % who)
    ins, outs, rows = [], [], []
    for i, p in enumerate(problems):
        w = '%s: problems[%d]' % (who, i)
        M, T, N, K = _gemm_dims(w, p['M'], p['T'], N=p['N'], K=p['K'])
        taps, pad_l = int_arg(w, 'taps', p['taps'], 1, 64), int_arg(w, 'pad_l', p['pad_l'], -64, 64)
        lda, ldy, ldw = _pitch(w, 'lda', p.get('lda'), K), _pitch(w, 'ldy', p.get('ldy'), N), _pitch(w, 'ldw', p.get('ldw'), N)
        ins += [('A[%d]' % i, p['A'], _span(M, K, lda), False), ('Y[%d]' % i, p['Y'], _span(M, N, ldy), False)]
        outs += [('W[%d]' % i, p['W'], _span(taps * K, N, ldw), False), ('dbias[%d]' % i, p.get('dbias'), N, True)]
        rows.append((lda, ldy, ldw, M, N, K, taps, T, pad_l))
    _flat_args(who, ins, outs)
    n = len(problems)
    col = lambda j: (C.c_int * n)(*[r[j] for r in rows])
    dbias = [p.get('dbias') for p in problems]
    _check(_lib.taco_debug_gemm_tn_group(n, _ptr_table([p['A'] for p in problems]), col(0), _ptr_table([p['Y'] for p in problems]), col(1),
                                         _ptr_table([p['W'] for p in problems]), col(2), _ptr_table(dbias) if any(d is not None for d in dbias) else None,
                                         col(3), col(4), col(5), col(6), col(7), col(8), stream_ptr()), 'taco_debug_gemm_tn_group')


def debug_gemm_tn_strided(A, Y, W, M, N, K, batch, strideA, strideY, strideW, T=None, pad_l=1, lda=None, ldy=None, ldw=None):
    """`batch` weight gradients of one launch (taco_debug_gemm_tn_strided): member z reads A + z strideA (M, K; lda) and Y + z strideY
    (M, N; ldy) and adds to W + z strideW (K, N; ldw); strides in floats."""
    who = 'debug_gemm_tn_strided'
    M, T, N, K = _gemm_dims(who, M, M if T is None else T, N=N, K=K)
    batch, pad_l = int_arg(who, 'batch', batch, 1, 4096), int_arg(who, 'pad_l', pad_l, -64, 64)
    lda, ldy, ldw = _pitch(who, 'lda', lda, K), _pitch(who, 'ldy', ldy, N), _pitch(who, 'ldw', ldw, N)
    need = (_span(M, K, lda), _span(M, N, ldy), _span(K, N, ldw))
    strides = [_pitch(who, n, s, least) for n, s, least in zip(('strideA', 'strideY', 'strideW'), (strideA, strideY, strideW), need)]
    ext = [(batch - 1) * s + n for s, n in zip(strides, need)]
    _flat_args(who, [('A', A, ext[0], False), ('Y', Y, ext[1], False)], [('W', W, ext[2], False)])
    _check(_lib.taco_debug_gemm_tn_strided(ptr(A), lda, strides[0], ptr(Y), ldy, strides[1], ptr(W), ldw, strides[2], M, N, K, T, pad_l, batch,
                                           stream_ptr()), 'taco_debug_gemm_tn_strided')


# ---- op-level debug doors of the train step's glue kernels (include/taco_hip.h; tests/test_gpu_glue_ops.py) ----
# Flat contiguous tensors again, each of the dtype its operand has (float32, int32 ids and lengths, uint8 keep masks) and of at
# least the operand's element count; TACO_DETERMINISTIC is read by the library on every call.
DOOR_MAX_FLAT = (1 << 31) - 1
LOSS_PARTS = 512           # kLossParts
SUMSQ_PARTS = 256          # kSumsqParts
MAX_TRANSPOSE_BATCH = 96   # kMaxTransposeBatch
_ACTS = {'none': 0, 'relu': 1, 'sigmoid': 2, 'tanh': 3}


def _typed_args(who, ins, outs, alias=()):
    """_flat_args for operands of any dtype: ins, outs = [(name, tensor, dtype, elements needed, optional)].  `alias`: (in, out) name
    pairs that may be the very same tensor (same start: the in-place form); any other meeting of an output with an operand is refused."""
    dev = ins[0][1].device if torch.is_tensor(ins[0][1]) else None
    for name, t, dtype, need, optional in ins + outs:
        if tensor_arg(who, name, t, dtype, ('n',), dev, optional) is not None and t.numel() < need:
            raise ValueError('%s: %s must hold at least %d elements, got %d' % (who, name, need, t.numel()))
    live_in = [(n, t, need) for n, t, _, need, _ in ins if t is not None]
    live_out = [(n, t, need) for n, t, _, need, _ in outs if t is not None]
    for i, (n_out, t_out, need_out) in enumerate(live_out):
        for n_in, t_in, need_in in live_in + live_out[i + 1:]:
            if (n_in, n_out) in alias and t_in.data_ptr() == t_out.data_ptr():
                continue
            no_overlap(who, n_in, t_in, n_out, t_out[:need_out], span_in=t_in.element_size() * need_in)
    on_gpu(who, ins[0][0], dev)
    return dev


def _f(name, t, need, optional=False):
    return (name, t, torch.float32, need, optional)


def _rows_cols(who, **dims):
    """rows-like dimensions (upper-case first letter B, M, T, R) in [1, 2^22], the others columns in [1, 2^14]"""
    return tuple(int_arg(who, k.lower() if k == 'Rows' else k, v, 1, DOOR_MAX_GEMM_ROWS if k[0] in 'BMTR' else DOOR_MAX_GEMM_COLS) for k, v in dims.items())


def _cols4(who, name, v):
    if v % 4:
        raise ValueError('%s: %s must be a multiple of 4, got %d' % (who, name, v))
    return v


def _bt(who, B, T):
    if B * T > DOOR_MAX_GEMM_ROWS:
        raise ValueError('%s: B T must be <= %d, got %d' % (who, DOOR_MAX_GEMM_ROWS, B * T))


def debug_embedding(table, ids, out, rows, V, width):
    """out (rows, width) = table (V, width) [clamp(ids)] (taco_debug_embedding); ids int32 (rows)."""
    who = 'debug_embedding'
    rows, V, width = _rows_cols(who, Rows=rows, V=V, width=width)
    _cols4(who, 'width', width)
    _typed_args(who, [_f('table', table, V * width), ('ids', ids, torch.int32, rows, False)], [_f('out', out, rows * width)])
    _check(_lib.taco_debug_embedding(ptr(table), ptr(ids), ptr(out), rows, V, width, stream_ptr()), 'taco_debug_embedding')


def debug_embedding_bwd(dout, ids, dtable, rows, V, width):
    """dtable (V, width) += the rows of dout (rows, width) by clamped id (taco_debug_embedding_bwd); width <= 1024."""
    who = 'debug_embedding_bwd'
    rows, V = _rows_cols(who, Rows=rows, V=V)
    width = _cols4(who, 'width', int_arg(who, 'width', width, 4, 1024))
    _typed_args(who, [_f('dout', dout, rows * width), ('ids', ids, torch.int32, rows, False)], [_f('dtable', dtable, V * width)])
    _check(_lib.taco_debug_embedding_bwd(ptr(dout), ptr(ids), ptr(dtable), rows, V, width, stream_ptr()), 'taco_debug_embedding_bwd')


def debug_highway_combine(th, x, y, M):
    """y (M, 128) = H T + x (1 - T) with th (M, 256) = [T | H] (taco_debug_highway_combine)."""
    who = 'debug_highway_combine'
    M, = _rows_cols(who, M=M)
    _typed_args(who, [_f('th', th, M * 256), _f('x', x, M * 128)], [_f('y', y, M * 128)])
    _check(_lib.taco_debug_highway_combine(ptr(th), ptr(x), ptr(y), M, stream_ptr()), 'taco_debug_highway_combine')


def debug_highway_combine_bwd(th, x, dy, dth, dx, M):
    """dth (M, 256), dx (M, 128) of the blend above from dy (M, 128) (taco_debug_highway_combine_bwd)."""
    who = 'debug_highway_combine_bwd'
    M, = _rows_cols(who, M=M)
    _typed_args(who, [_f('th', th, M * 256), _f('x', x, M * 128), _f('dy', dy, M * 128)], [_f('dth', dth, M * 256), _f('dx', dx, M * 128)])
    _check(_lib.taco_debug_highway_combine_bwd(ptr(th), ptr(x), ptr(dy), ptr(dth), ptr(dx), M, stream_ptr()), 'taco_debug_highway_combine_bwd')


def debug_act_bwd(y, dy, dz, n, act, keep=None):
    """dz = dy act'(y) [keep ? 2 : 0] over n elements (taco_debug_act_bwd); act 'none' | 'relu' | 'sigmoid' | 'tanh'; keep uint8 (n) or
    None; dz may be dy itself (in place)."""
    who = 'debug_act_bwd'
    n = int_arg(who, 'n', n, 1, DOOR_MAX_FLAT)
    if act not in _ACTS:
        raise ValueError('%s: act must be one of %s, got %r' % (who, sorted(_ACTS), act))
    _typed_args(who, [_f('y', y, n), _f('dy', dy, n), ('keep', keep, torch.uint8, n, True)], [_f('dz', dz, n)], alias=(('dy', 'dz'),))
    _check(_lib.taco_debug_act_bwd(ptr(y), ptr(dy), ptr(keep), ptr(dz), n, _ACTS[act], stream_ptr()), 'taco_debug_act_bwd')


def debug_affine_act_bwd(pre, gamma, dy, dz, dgamma, dbeta, M, N, act):
    """The BN-affine backward (taco_debug_affine_act_bwd): pre, dy, dz (M, N); dgamma, dbeta (N) are added to; act 'none' | 'relu'."""
    who = 'debug_affine_act_bwd'
    M, N = _rows_cols(who, M=M, N=N)
    if act not in ('none', 'relu'):
        raise ValueError("%s: act must be 'none' or 'relu', got %r" % (who, act))
    _typed_args(who, [_f('pre', pre, M * N), _f('gamma', gamma, N), _f('dy', dy, M * N)],
                [_f('dz', dz, M * N), _f('dgamma', dgamma, N), _f('dbeta', dbeta, N)])
    _check(_lib.taco_debug_affine_act_bwd(ptr(pre), ptr(gamma), ptr(dy), ptr(dz), ptr(dgamma), ptr(dbeta), M, N, _ACTS[act], stream_ptr()),
           'taco_debug_affine_act_bwd')


def debug_colsum_batched(x, out, B, T, N, ld=None):
    """out (B, N) = the column sums of each sequence of T rows of x (B T, N; ld) (taco_debug_colsum_batched); overwritten."""
    who = 'debug_colsum_batched'
    B, T, N = _rows_cols(who, B=int_arg(who, 'B', B, 1, 65535), T=T, N=N)
    _bt(who, B, T)
    ld = _pitch(who, 'ld', ld, N)
    _typed_args(who, [_f('x', x, _span(B * T, N, ld))], [_f('out', out, B * N)])
    _check(_lib.taco_debug_colsum_batched(ptr(x), ld, ptr(out), B, T, N, stream_ptr()), 'taco_debug_colsum_batched')


def debug_mask_rows(x, length, y, B, T, C_cols):
    """y (B, T, C) = x where t < length[b], else 0 (taco_debug_mask_rows); length int32 (B)."""
    who = 'debug_mask_rows'
    B, T, C_cols = _rows_cols(who, B=B, T=T, C=C_cols)
    _bt(who, B, T)
    _cols4(who, 'C', C_cols)
    _typed_args(who, [_f('x', x, B * T * C_cols), ('length', length, torch.int32, B, False)], [_f('y', y, B * T * C_cols)])
    _check(_lib.taco_debug_mask_rows(ptr(x), ptr(length), ptr(y), B, T, C_cols, stream_ptr()), 'taco_debug_mask_rows')


def debug_center_rows(x, length, out, B, T, C_cols):
    """out (B, T, C) = x less its column means over the first clamp(length[b], 1, T) rows, 0 behind them (taco_debug_center_rows)."""
    who = 'debug_center_rows'
    B, T, C_cols = _rows_cols(who, B=int_arg(who, 'B', B, 1, 65535), T=T, C=C_cols)
    _bt(who, B, T)
    _cols4(who, 'C', C_cols)
    _typed_args(who, [_f('x', x, B * T * C_cols), ('length', length, torch.int32, B, False)], [_f('out', out, B * T * C_cols)])
    _check(_lib.taco_debug_center_rows(ptr(x), ptr(length), ptr(out), B, T, C_cols, stream_ptr()), 'taco_debug_center_rows')


def debug_mask_pos(g, y, rows, cols, scale, ldg=None, ldy=None):
    """in place g (rows, cols; ldg) = y (rows, cols; ldy) > 0 ? scale g : 0 (taco_debug_mask_pos)."""
    who = 'debug_mask_pos'
    rows, cols = _rows_cols(who, Rows=rows, cols=cols)
    ldg, ldy = _pitch(who, 'ldg', ldg, cols), _pitch(who, 'ldy', ldy, cols)
    _typed_args(who, [_f('y', y, _span(rows, cols, ldy))], [_f('g', g, _span(rows, cols, ldg))])
    _check(_lib.taco_debug_mask_pos(ptr(g), ldg, ptr(y), ldy, rows, cols, float(scale), stream_ptr()), 'taco_debug_mask_pos')


def debug_zero_tail_rows(x0, C0, length, B, Td, x1=None, C1=0):
    """rows t >= length[b] of x0 (B, Td, C0) and, when given, x1 (B, Td, C1) become 0 in place (taco_debug_zero_tail_rows)."""
    who = 'debug_zero_tail_rows'
    B, Td, C0 = _rows_cols(who, B=B, Td=Td, C0=C0)
    _bt(who, B, Td)
    C1 = int_arg(who, 'C1', C1, 1, DOOR_MAX_GEMM_COLS) if x1 is not None else 0
    _typed_args(who, [('length', length, torch.int32, B, False)], [_f('x0', x0, B * Td * C0), _f('x1', x1, B * Td * C1, True)])
    _check(_lib.taco_debug_zero_tail_rows(ptr(x0), C0, ptr(x1), C1, ptr(length), B, Td, stream_ptr()), 'taco_debug_zero_tail_rows')


def debug_add(a, b, y, n):
    """y = a + b over n elements (taco_debug_add)."""
    who = 'debug_add'
    n = int_arg(who, 'n', n, 1, DOOR_MAX_FLAT)
    _typed_args(who, [_f('a', a, n), _f('b', b, n)], [_f('y', y, n)])
    _check(_lib.taco_debug_add(ptr(a), ptr(b), ptr(y), n, stream_ptr()), 'taco_debug_add')


def debug_l1_loss(terms, parts, loss, out=None):
    """The loss as taco_forward forms it (taco_debug_l1_loss).  terms: two entries, each None (the term is 0) or a dict with a, b
    (M, N), M, N and optionally grad (M, N; ldg) and ldg; parts (2 x 512 block partials) and loss (3) are the caller's, out (3) optional."""
    who = 'debug_l1_loss'
    if not isinstance(terms, (list, tuple)) or len(terms) != 2 or all(t is None for t in terms):
        raise ValueError('%s: terms must be a list of two dicts, at most one of them None' % who)
    ins, outs, args = [], [], []
    for i, t in enumerate(terms):
        if t is None:
            args += [None, None, None, 0, 0, 0]
            continue
        M, N = _rows_cols('%s: terms[%d]' % (who, i), M=t['M'], N=t['N'])
        ldg = _pitch('%s: terms[%d]' % (who, i), 'ldg', t.get('ldg'), N)
        ins += [_f('a%d' % i, t['a'], M * N), _f('b%d' % i, t['b'], M * N)]
        outs += [_f('grad%d' % i, t.get('grad'), M * ldg, True)]
        args += [ptr(t['a']), ptr(t['b']), ptr(t.get('grad')), ldg, M, N]
    outs += [_f('parts', parts, 2 * LOSS_PARTS), _f('loss', loss, 3), _f('out', out, 3, True)]
    _typed_args(who, ins, outs)
    _check(_lib.taco_debug_l1_loss(*args, ptr(parts), ptr(loss), ptr(out), stream_ptr()), 'taco_debug_l1_loss')


def debug_transpose_batch(jobs):
    """Up to 96 (kMaxTransposeBatch) transposes of one launch (taco_debug_transpose_batch).  jobs: dicts with src (taps, K, N; ldi), dst
    (taps, N, K; ldo; tap order reversed), taps, K, N and optionally ldi, ldo (0 / missing: dense; a pitched job has taps == 1)."""
    who = 'debug_transpose_batch'
    if not isinstance(jobs, (list, tuple)) or not 1 <= len(jobs) <= MAX_TRANSPOSE_BATCH:
        raise ValueError('%s: jobs must be a list of 1 to %d dicts' % (who, MAX_TRANSPOSE_BATCH))
    ins, outs, rows = [], [], []
    for i, j in enumerate(jobs):
        w = '%s: jobs[%d]' % (who, i)
        taps = int_arg(w, 'taps', j['taps'], 1, 64)
        K, N = _rows_cols(w, K=j['K'], N=j['N'])
        ldi, ldo = int_arg(w, 'ldi', j.get('ldi') or 0, 0, _INT_MAX), int_arg(w, 'ldo', j.get('ldo') or 0, 0, _INT_MAX)
        if (ldi and ldi < N) or (ldo and ldo < K):
            raise ValueError('%s: ldi must be 0 or >= %d and ldo 0 or >= %d, got %d and %d' % (w, N, K, ldi, ldo))
        if (ldi or ldo) and taps != 1:
            raise ValueError('%s: a job with a pitch has taps == 1, got %d' % (w, taps))
        ins.append(_f('src[%d]' % i, j['src'], _span(taps * K, N, ldi or N)))
        outs.append(_f('dst[%d]' % i, j['dst'], _span(taps * N, K, ldo or K)))
        rows.append((taps, K, N, ldi, ldo))
    _typed_args(who, ins, outs)
    n = len(jobs)
    col = lambda k: (C.c_int * n)(*[r[k] for r in rows])
    pitched = any(r[3] or r[4] for r in rows)
    _check(_lib.taco_debug_transpose_batch(n, _ptr_table([j['src'] for j in jobs]), _ptr_table([j['dst'] for j in jobs]), col(0), col(1), col(2),
                                           col(3) if pitched else None, col(4) if pitched else None, stream_ptr()), 'taco_debug_transpose_batch')


def debug_sumsq(x, n, out):
    """out[0 .. 256) = the per-block partial sums of squares of x[0 .. n) that clip+Adam adds up (taco_debug_sumsq); x 16-byte aligned."""
    who = 'debug_sumsq'
    n = int_arg(who, 'n', n, 1, DOOR_MAX_FLAT)
    _typed_args(who, [_f('x', x, n)], [_f('out', out, SUMSQ_PARTS)])
    if x.data_ptr() % 16:
        raise ValueError('%s: x must be 16-byte aligned' % who)
    _check(_lib.taco_debug_sumsq(ptr(x), n, ptr(out), stream_ptr()), 'taco_debug_sumsq')


def forward(shape, params, text, text_length, mel, stft, masks, s2s, out, align, loss, workspace, speaker=None):
    m = masks or {}
    _check(_lib.taco_forward(C.byref(shape), ptr(params), ptr(text), ptr(text_length), ptr(speaker), ptr(mel), ptr(stft),
                             ptr(m.get('enc_keep1')), ptr(m.get('enc_keep2')), ptr(m.get('dec_keep1')),
                             ptr(m.get('dec_keep2')), ptr(m.get('sample')), ptr(s2s), ptr(out), ptr(align), ptr(loss),
                             ptr(workspace), stream_ptr()), 'taco_forward')


def backward(shape, params, text, text_length, s2s, align, masks, grads, workspace, speaker=None):
    m = masks or {}
    _check(_lib.taco_backward(C.byref(shape), ptr(params), ptr(text), ptr(text_length), ptr(speaker), ptr(s2s), ptr(align),
                              ptr(m.get('enc_keep1')), ptr(m.get('enc_keep2')), ptr(m.get('dec_keep1')),
                              ptr(m.get('dec_keep2')), ptr(m.get('sample')), ptr(grads), ptr(workspace), stream_ptr()),
           'taco_backward')


def infer(shape, params, text, text_length, s2s, out, align, workspace, speaker=None):
    _check(_lib.taco_infer(C.byref(shape), ptr(params), ptr(text), ptr(text_length), ptr(speaker), ptr(s2s), ptr(out), ptr(align),
                           ptr(workspace), stream_ptr()), 'taco_infer')


def infer_stop(shape, params, text, text_length, rule, s2s, out, align, lengths, workspace, speaker=None):
    """taco_infer with end detection: `rule` a TacoStopRule, `lengths` (B) int32 on the device receives len_b; rows t >= len_b of
    s2s / out / align are 0."""
    _check(_lib.taco_infer_stop(C.byref(shape), ptr(params), ptr(text), ptr(text_length), ptr(speaker), C.byref(rule) if rule is not None else None,
                                ptr(s2s), ptr(out), ptr(align), ptr(lengths), ptr(workspace), stream_ptr()), 'taco_infer_stop')


ALIGN_COUNTS = ('n', 'end', 'pad_steps', 'back', 'skip', 'covered')   # columns of counts (include/taco_hip.h taco_alignment_scores)
ALIGN_MEANS = ('focus', 'pad_mass')                                   # columns of means
MAX_JUMP = 3                       # `skip` counts argmax moves of more than this many characters in one decoder step; a choice
ALIGN_MAX_TD = ALIGN_MAX_TT = 16384   # TACO_ALIGNMENT_MAX_TD / _TT


def alignment_scores(alignments, text_length, steps=None, max_jump=MAX_JUMP, counts=None, means=None):
    """Per-utterance attention scores (include/taco_hip.h taco_alignment_scores): alignments (B, Td, Tt) fp32, text_length (B) int32,
    steps (B) int32 or None -- the lengths of infer_stop; None scores all Td steps -- all on the device -> (counts (B, 6) int32 in the
    order ALIGN_COUNTS, means (B, 2) fp32 in the order ALIGN_MEANS), device tensors.  Enqueued on the current stream; nothing is
    copied and nothing waits.  counts / means: the caller's own buffers; default: fresh ones."""
    who = 'alignment_scores'
    B, Td, Tt = tensor_arg(who, 'alignments', alignments, torch.float32, ('B', 'Td', 'Tt'))
    dev = alignments.device
    if Td > ALIGN_MAX_TD or Tt > ALIGN_MAX_TT:
        raise ValueError('%s: at most %d steps and %d characters, got Td = %d, Tt = %d' % (who, ALIGN_MAX_TD, ALIGN_MAX_TT, Td, Tt))
    tensor_arg(who, 'text_length', text_length, torch.int32, (B,), dev)
    tensor_arg(who, 'steps', steps, torch.int32, (B,), dev, optional=True)
    max_jump = int_arg(who, 'max_jump', max_jump, 0, _INT_MAX)
    counts = _own_or_given(counts, (B, len(ALIGN_COUNTS)), torch.int32, dev, who + ': counts')
    means = _own_or_given(means, (B, len(ALIGN_MEANS)), torch.float32, dev, who + ': means')
    on_gpu(who, 'alignments', dev)
    _check(_lib.taco_alignment_scores(ptr(alignments), ptr(text_length), ptr(steps), max_jump, ptr(counts), ptr(means), B, Td, Tt,
                                      stream_ptr()), 'taco_alignment_scores')
    return counts, means


PATH_COUNTS = ('n', 'end', 'skipped')   # columns of counts (include/taco_hip.h taco_alignment_path)
PATH_JUMP = 4                      # characters a decoder step may advance on the path; untuned -- at r = 5 a step covers more than
                                   # one character of ordinary speech, so 1 is not usable
PATH_MAX_TD, PATH_MAX_TT, PATH_MAX_JUMP = 16384, 4096, 15   # TACO_ALIGN_PATH_MAX_TD / _TT / _JUMP


def _path_shape(who, B, Td, Tt):
    if Td > PATH_MAX_TD or Tt > PATH_MAX_TT:
        raise ValueError('%s: at most %d steps and %d characters, got Td = %d, Tt = %d' % (who, PATH_MAX_TD, PATH_MAX_TT, Td, Tt))
    return int_arg(who, 'B', B, 1, _INT_MAX), int_arg(who, 'Td', Td, 1), int_arg(who, 'Tt', Tt, 1)


def alignment_path_workspace_bytes(B, Td, Tt) -> int:
    return _size('taco_alignment_path_workspace_bytes', *_path_shape('alignment_path_workspace_bytes', B, Td, Tt))


def alignment_path(alignments, text_length, steps=None, max_jump=PATH_JUMP, path=None, dur=None, counts=None, mass=None, workspace=None):
    """The best monotone path through each attention matrix (include/taco_hip.h taco_alignment_path): alignments (B, Td, Tt) fp32,
    text_length (B) int32, steps (B) int32 or None -- the lengths of infer_stop; None walks all Td steps -- all on the device, max_jump
    in 1 .. 15 the characters a step may advance -> (path (B, Td) int32: the character of every step, -1 from the row's length on;
    dur (B, Tt) int32: the steps of every character; counts (B, 3) int32 in the order PATH_COUNTS; mass (B) fp32: the attention mass
    on the path), device tensors.  workspace: uint8, alignment_path_workspace_bytes(B, Td, Tt) bytes (0 for the product's shapes).
    Enqueued on the current stream; nothing is copied and nothing waits.  The outputs and workspace: the caller's own buffers;
    default: fresh ones."""
    who = 'alignment_path'
    B, Td, Tt = tensor_arg(who, 'alignments', alignments, torch.float32, ('B', 'Td', 'Tt'))
    dev = alignments.device
    _path_shape(who, B, Td, Tt)
    tensor_arg(who, 'text_length', text_length, torch.int32, (B,), dev)
    tensor_arg(who, 'steps', steps, torch.int32, (B,), dev, optional=True)
    max_jump = int_arg(who, 'max_jump', max_jump, 1, PATH_MAX_JUMP)
    path = _own_or_given(path, (B, Td), torch.int32, dev, who + ': path')
    dur = _own_or_given(dur, (B, Tt), torch.int32, dev, who + ': dur')
    counts = _own_or_given(counts, (B, len(PATH_COUNTS)), torch.int32, dev, who + ': counts')
    mass = _own_or_given(mass, (B,), torch.float32, dev, who + ': mass')
    if workspace is not None:
        tensor_arg(who, 'workspace', workspace, torch.uint8, ('bytes',), dev, empty_ok=True)
    on_gpu(who, 'alignments', dev)
    workspace = _own_or_given(workspace, (alignment_path_workspace_bytes(B, Td, Tt),), torch.uint8, dev, who + ': workspace')
    _check(_lib.taco_alignment_path(ptr(alignments), ptr(text_length), ptr(steps), max_jump, ptr(path), ptr(dur), ptr(counts), ptr(mass),
                                    ptr(workspace) if workspace.numel() else None, B, Td, Tt, stream_ptr()), 'taco_alignment_path')
    return path, dur, counts, mass


def clip_adam_step(params, grads, m, v, lr, cap, step, scratch, gnorm_out, err_words=None):
    """err_words: int32 view of the workspace's `dec.err` tensor (first two words) or None (unguarded)."""
    assert scratch.numel() >= 256, 'taco: clip_adam scratch must hold 256 floats'
    _check(_lib.taco_clip_adam_step_guarded(ptr(params), ptr(grads), ptr(m), ptr(v), params.numel(), float(lr), float(cap),
                                            int(step), ptr(scratch), ptr(gnorm_out), ptr(err_words), stream_ptr()),
           'taco_clip_adam_step_guarded')


def clear_error(shape, train, workspace):
    _check(_lib.taco_clear_error(C.byref(shape), int(train), ptr(workspace), stream_ptr()), 'taco_clear_error')


def grad_segments(shape):
    """Float offsets [b0 .. b5] of the five gradient segments (0 embedding + encoder pre_net, 1 encoder conv bank, 2 rest of the
    encoder, 3 decoder, 4 post-net); they become final in the order 4, 3, 2, 1, 0 during taco_backward."""
    b = (C.c_int64 * 8)()
    n = _lib.taco_grad_segments(C.byref(shape), b)
    if n < 1 or n > 7:
        raise TacoError('taco_grad_segments: ' + last_error())
    return [int(x) for x in b[:n + 1]]


def wait_grad_segment(seg, stream):
    """Device-side wait of `stream` (a torch.cuda.Stream) for segment `seg` of this thread's last taco_backward."""
    _check(_lib.taco_wait_grad_segment(int(seg), C.c_void_p(stream.cuda_stream)), 'taco_wait_grad_segment')


def decoder_mode(mode=-1) -> int:
    """Process-wide decoder mode (include/taco_hip.h): 0 decoder3 fast exchange, 1 decoder3 agent-scope exchange, 2 decoder.hip.
    Sets it when mode >= 0; returns the PREVIOUS mode."""
    return _lib.taco_decoder_mode(int(mode))


def clock_probe(iters=1 << 20):
    """GHz the chip sustains under a chip-wide latency-bound load (every CU: 8 waves of dependent FMAs); host synchronisation."""
    out = torch.zeros(3, dtype=torch.int64, device='cuda')
    for _ in range(2):   # (first call: clocks ramping up)
        _check(_lib.taco_debug_clock_probe(ptr(out), int(iters), stream_ptr()), 'taco_debug_clock_probe')
    torch.cuda.synchronize()
    cyc, ticks = out[0].item(), out[1].item()
    return cyc / (ticks * 10.0) if ticks > 0 else 0.0


def fabric_probe(iters=2000, scratch_mb=768):
    """Latencies of this box that the latency-bound kernels wait on (include/taco_hip.h taco_debug_fabric_probe); host
    synchronisation.  Returns ns per granule hop (one way) in the three exchange forms, ns per dependent load (plain, L2 hit / agent scope
    on cold lines), the bandwidth one workgroup streams at, and which XCDs the probing workgroups ran on."""
    out = torch.zeros(32, dtype=torch.int64, device='cuda')
    gran = torch.zeros(512, dtype=torch.int64, device='cuda')
    scratch = torch.zeros(scratch_mb << 18, dtype=torch.int32, device='cuda')
    res = None
    for _ in range(2):   # (first call: clocks ramping up, cold TLBs)
        out.zero_(); gran.zero_()
        _check(_lib.taco_debug_fabric_probe(ptr(out), ptr(gran), ptr(scratch), int(scratch.numel() * 4), int(iters), stream_ptr()),
               'taco_debug_fabric_probe')
        torch.cuda.synchronize()
        res = out.tolist()
    n = max(1, res[6])
    ok = res[7]
    xcc = res[8:32]
    hop = lambda t: t * 10.0 / n / 2.0   # noqa: E731  (a round trip is two hops)
    return {'hop_ns_same_xcd_l2_local': hop(res[0]) if ok & 1 else None,
            'hop_ns_same_xcd_agent_scope': hop(res[1]) if ok & 2 else None,
            'hop_ns_cross_xcd': hop(res[2]) if ok & 4 else None,
            'load_ns_l2_hit': res[3] * 10.0 / n, 'load_ns_agent_scope_cold': res[4] * 10.0 / n,
            'one_cu_stream_gb_s': (8 << 20) / (res[5] * 10e-9) / 1e9 if res[5] > 0 else None,
            'xcc_of_pairs': {'l2_local': [xcc[0], xcc[8]], 'agent': [xcc[1], xcc[9]], 'cross': [xcc[2], xcc[3]]},
            'scratch_mb': scratch_mb}


def debug_spin(blocks, threads, lds_bytes, usec, stream=None):
    """Communication-kernel stand-in (co-residency tests): spins `usec` microseconds on `stream` (default: current)."""
    sp = stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _check(_lib.taco_debug_spin(int(blocks), int(threads), int(lds_bytes), int(usec), sp), 'taco_debug_spin')


def denorm_unframe(output, stft_mean, stft_std, r, want_spec=True, want_mag_t=False, spec=None, mag_t=None):
    """(B, Td, r*C) normalised r-frame layout -> chronological de-normalised (B, F, C) [and / or exp() transposed (B, C, F)].
    spec / mag_t: the caller's own output buffers (default: fresh ones)."""
    B, Td, RC = output.shape
    Cw = RC // r
    F = (Td // 4) * 4 * r
    spec = _own_or_given(spec, (B, F, Cw), torch.float32, output.device, 'denorm_unframe: spec') if want_spec else None
    mag_t = _own_or_given(mag_t, (B, Cw, F), torch.float32, output.device, 'denorm_unframe: mag_t') if want_mag_t else None
    _check(_lib.taco_denorm_unframe(ptr(output), ptr(stft_mean), ptr(stft_std), ptr(spec), ptr(mag_t), B, Td, r, Cw,
                                    stream_ptr()), 'taco_denorm_unframe')
    if want_spec and want_mag_t:
        return spec, mag_t
    return spec if want_spec else mag_t


STRETCH_ONE, STRETCH_MIN_STEP, STRETCH_MAX_STEP, STRETCH_MAX_FRAMES = 65536, 16384, 262144, 8192   # include/taco_hip.h


def stretch_step(rate) -> int:
    """A speaking rate (1.0: the model's own, 0.8 slower, 1.25 faster) -> step_q of taco_frames_stretch = round(65536 * rate), the
    source frames advanced per output frame in units of 2^-16; ValueError outside [0.25, 4] or for NaN"""
    try:
        rate = float(rate)
    except (TypeError, ValueError):
        raise ValueError('rate must be a number in [0.25, 4], got %r' % (rate,)) from None
    if not 0.25 <= rate <= 4.0:   # (NaN fails both comparisons)
        raise ValueError('rate must be in [0.25, 4], got %r' % (rate,))
    return int(round(65536.0 * rate))


def _stretch_clamp(step_q) -> int:
    return min(max(int(step_q), STRETCH_MIN_STEP), STRETCH_MAX_STEP)


def stretch_frames(F_b, step_q, cap=None) -> int:
    """Fo_b of taco_frames_stretch on the host: 0 for F_b <= 0, else ((F_b - 1) << 16) // s + 1 with s = step_q clamped as the device
    clamps it, and at most `cap` (the Fo of the call) when given"""
    F_b = int(F_b)
    if F_b <= 0:
        return 0
    n = ((F_b - 1) << 16) // _stretch_clamp(step_q) + 1
    return n if cap is None else min(int(cap), n)


def stretch_capacity(F, step_q_min) -> int:
    """The Fo no row of a (B, C, F) call can exceed when no row's step is below step_q_min (the slowest rate of the batch)"""
    return stretch_frames(F, step_q_min)


def _frames_cap(who, F):
    if F > STRETCH_MAX_FRAMES:
        raise ValueError('%s: at most %d frames, got F = %d' % (who, STRETCH_MAX_FRAMES, F))


def _row_frames_arg(who, frames, frames_per_unit, B, dev) -> int:
    """the per-row frame counts of the frames_* calls: frames None or (B) int32 on dev, in units of frames_per_unit >= 1 (returned)"""
    tensor_arg(who, 'frames', frames, torch.int32, (B,), dev, optional=True)
    return int_arg(who, 'frames_per_unit', frames_per_unit, 1)


def frames_stretch(mag_t, frames=None, step_q=None, frames_per_unit=1, Fo=None, out=None, frames_out=None):
    """Speaking rate on the magnitude frames (include/taco_hip.h taco_frames_stretch): mag_t (B, C, F) fp32 on the device ->
    (out (B, C, Fo) fp32, frames_out (B) int32): row b's first F_b = clamp(frames[b] * frames_per_unit, 0, F) frames resampled
    linearly at step_q[b] / 65536 source frames per output frame, Fo_b = stretch_frames(F_b, step_q[b], Fo) of them, zeros behind.
    frames: (B) int32 on the device, or None (all F frames).  step_q: None (65536: a copy), an int (the whole batch), a host sequence
    of B ints (checked against [16384, 262144], then uploaded) or a (B) int32 tensor on the device (clamped there, never read here).
    Fo: default the capacity at the slowest step the host knows of (16384 for a device tensor).  out / frames_out: the caller's own
    buffers; default: fresh ones.  Enqueued on the current stream; nothing is read back and nothing waits."""
    who = 'frames_stretch'
    B, Cw, F = tensor_arg(who, 'mag_t', mag_t, torch.float32, ('B', 'C', 'F'))
    dev = mag_t.device
    _frames_cap(who, F)
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    step_q, slowest = step_q_arg(who, step_q, B, dev, STRETCH_MIN_STEP, STRETCH_MAX_STEP, 'rates 0.25 to 4')
    if Fo is None:
        Fo = stretch_capacity(F, STRETCH_ONE if slowest is None else slowest)
        if out is None and Fo > STRETCH_MAX_FRAMES:
            raise ValueError('%s: F = %d frames at step %d may need %d output frames, more than %d: give Fo'
                             % (who, F, slowest, Fo, STRETCH_MAX_FRAMES))
        if out is not None and torch.is_tensor(out) and out.dim() == 3:
            Fo = out.shape[2]
    Fo = int_arg(who, 'Fo', Fo, 1, STRETCH_MAX_FRAMES)
    out = _own_or_given(out, (B, Cw, Fo), torch.float32, dev, who + ': out')
    no_overlap(who, 'mag_t', mag_t, 'out', out)
    frames_out = _own_or_given(frames_out, (B,), torch.int32, dev, who + ': frames_out')
    on_gpu(who, 'mag_t', dev)
    _check(_lib.taco_frames_stretch(ptr(mag_t), ptr(frames), frames_per_unit, ptr(step_q), ptr(out), ptr(frames_out), B, Cw, F, Fo,
                                    stream_ptr()), 'taco_frames_stretch')
    return out, frames_out


PITCH_ONE, PITCH_MIN_STEP, PITCH_MAX_STEP, PITCH_MAX_LIFTER = 65536, 32768, 131072, 64   # include/taco_hip.h


def pitch_step(semitones) -> int:
    """A pitch shift in semitones (0: the model's own, +12 an octave up) -> step_q of taco_frames_pitch =
    round(65536 * 2^(-semitones / 12)), the source bins advanced per output bin in units of 2^-16; ValueError outside [-12, 12] or for
    a non-finite value"""
    try:
        semitones = float(semitones)
    except (TypeError, ValueError):
        raise ValueError('pitch must be a number of semitones in [-12, 12], got %r' % (semitones,)) from None
    if not -12.0 <= semitones <= 12.0:   # (NaN fails both comparisons)
        raise ValueError('pitch must be in [-12, 12] semitones, got %r' % (semitones,))
    return int(round(65536.0 * 2.0 ** (-semitones / 12.0)))


def steps_of(values, to_step, n=None):
    """Rates or pitches -> step_q values by to_step (stretch_step / pitch_step): None -> None; a number -> an int; a host sequence or
    host tensor -> a list of ints (ValueError unless it holds n of them, when n is given); a tensor on a device holds step_q values
    already and is passed through, never read"""
    if values is None or (torch.is_tensor(values) and values.device.type != 'cpu'):
        return values
    values = values.tolist() if torch.is_tensor(values) else values
    if not hasattr(values, '__len__'):
        return to_step(values)
    if n is not None and len(values) != n:
        raise ValueError('%d values for %d rows' % (len(values), n))
    return [to_step(x) for x in values]


def frames_pitch(mag_t, frames=None, step_q=None, frames_per_unit=1, lifter=32, out=None):
    """Pitch on the magnitude frames (include/taco_hip.h taco_frames_pitch): mag_t (B, C, F) fp32 on the device, C - 1 a power of two
    in [8, 1024] -> out (B, C, F) fp32: in the first F_b = clamp(frames[b] * frames_per_unit, 0, F) frames of row b the log-excitation
    is warped along the bin axis at step_q[b] / 65536 source bins per output bin under the frame's own log-envelope (the cepstrum's
    quefrencies 0 .. lifter), zeros behind.
    frames: (B) int32 on the device, or None (all F frames).  step_q: None (65536: a copy), an int (the whole batch), a host sequence
    of B ints (checked against [32768, 131072], then uploaded) or a (B) int32 tensor on the device (clamped there, never read here).
    lifter: 1 .. min(64, (C - 1) / 2); the default 32 (quefrencies up to 2 ms at 16 kHz) is untuned.  out: the caller's own buffer;
    default: a fresh one.  Enqueued on the current stream; nothing is read back and nothing waits."""
    who = 'frames_pitch'
    B, Cw, F, dev, frames_per_unit, lifter = _cepstrum_args(who, mag_t, lifter, frames, frames_per_unit, first=1)
    step_q, _ = step_q_arg(who, step_q, B, dev, PITCH_MIN_STEP, PITCH_MAX_STEP, '+12 to -12 semitones')
    out = _own_or_given(out, (B, Cw, F), torch.float32, dev, who + ': out')
    no_overlap(who, 'mag_t', mag_t, 'out', out)
    on_gpu(who, 'mag_t', dev)
    _check(_lib.taco_frames_pitch(ptr(mag_t), ptr(frames), frames_per_unit, ptr(step_q), lifter, ptr(out), B, Cw, F, stream_ptr()),
           'taco_frames_pitch')
    return out


def stretch_dur(rate) -> int:
    """A speaking rate -> dur_q of taco_frames_stretch_curve = round(65536 / rate), the output frames a source frame lasts in units
    of 2^-16 (the inverse sense of stretch_step: durations add); ValueError outside [0.25, 4] or for NaN"""
    try:
        rate = float(rate)
    except (TypeError, ValueError):
        raise ValueError('rate must be a number in [0.25, 4], got %r' % (rate,)) from None
    if not 0.25 <= rate <= 4.0:   # (NaN fails both comparisons)
        raise ValueError('rate must be in [0.25, 4], got %r' % (rate,))
    return int(round(65536.0 / rate))


def stretch_curve_capacity(F, dur_q_max) -> int:
    """The Fo no row of a (B, C, F) taco_frames_stretch_curve call can exceed when no duration is above dur_q_max (clamped as the
    device clamps it): min(8192, ((F - 1) * dur_q_max >> 16) + 1)"""
    F = int(F)
    if F <= 0:
        return 0
    return min(STRETCH_MAX_FRAMES, (((F - 1) * _stretch_clamp(dur_q_max)) >> 16) + 1)


def path_curve(path, values, frames_per_step=1, fill=0, curve=None):
    """Per-character values to a per-frame curve along the path of alignment_path (include/taco_hip.h taco_path_curve): path (B, Td)
    int32 and values (B, Tt) int32 on the device -> curve (B, Td * frames_per_step) int32 with
    curve[b, t * frames_per_step + u] = values[b, path[b, t]], and `fill` where the path names no character (-1 behind the row's
    steps, an index >= Tt).  Exact, nothing clamped.  curve: the caller's own buffer; default: a fresh one.  Enqueued on the current
    stream; nothing is read back and nothing waits."""
    who = 'path_curve'
    B, Td = tensor_arg(who, 'path', path, torch.int32, ('B', 'Td'))
    dev = path.device
    (Tt,) = tensor_arg(who, 'values', values, torch.int32, (B, 'Tt'), dev)
    frames_per_step = int_arg(who, 'frames_per_step', frames_per_step, 1, STRETCH_MAX_FRAMES)
    if Td * frames_per_step > STRETCH_MAX_FRAMES:
        raise ValueError('%s: at most %d frames, got Td = %d x frames_per_step = %d' % (who, STRETCH_MAX_FRAMES, Td, frames_per_step))
    fill = int_arg(who, 'fill', fill, -(1 << 31), _INT_MAX)
    curve = _own_or_given(curve, (B, Td * frames_per_step), torch.int32, dev, who + ': curve')
    on_gpu(who, 'path', dev)
    _check(_lib.taco_path_curve(ptr(path), ptr(values), frames_per_step, fill, ptr(curve), B, Td, Tt, stream_ptr()), 'taco_path_curve')
    return curve


def frames_stretch_curve(mag_t, frames=None, dur_q=None, frames_per_unit=1, Fo=None, dur_q_max=STRETCH_MAX_STEP, out=None,
                         frames_out=None, src=None):
    """A speaking rate that varies along the utterance (include/taco_hip.h taco_frames_stretch_curve): mag_t (B, C, F) fp32 on the
    device -> (out (B, C, Fo) fp32, frames_out (B) int32, src (B, Fo) int32).  dur_q: (B, F) int32 on the device -- the output frames
    source frame i lasts in units of 2^-16 (stretch_dur(rate)), clamped there to [16384, 262144] and never read here -- or None
    (65536 everywhere: a copy).  src is the time map: (i << 16) | wq per output frame, -1 behind Fo_b.  frames: (B) int32 on the
    device, or None.  Fo: default stretch_curve_capacity(F, dur_q_max), dur_q_max being the caller's statement of the slowest
    duration in dur_q (F for None).  out / frames_out / src: the caller's own buffers; default: fresh ones.  Enqueued on the
    current stream; nothing is read back and nothing waits."""
    who = 'frames_stretch_curve'
    B, Cw, F = tensor_arg(who, 'mag_t', mag_t, torch.float32, ('B', 'C', 'F'))
    dev = mag_t.device
    _frames_cap(who, F)
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    tensor_arg(who, 'dur_q', dur_q, torch.int32, (B, F), dev, optional=True)
    if Fo is None:
        if out is not None and torch.is_tensor(out) and out.dim() == 3:
            Fo = out.shape[2]
        else:
            Fo = F if dur_q is None else stretch_curve_capacity(F, int_arg(who, 'dur_q_max', dur_q_max, STRETCH_MIN_STEP, STRETCH_MAX_STEP))
    Fo = int_arg(who, 'Fo', Fo, 1, STRETCH_MAX_FRAMES)
    out = _own_or_given(out, (B, Cw, Fo), torch.float32, dev, who + ': out')
    no_overlap(who, 'mag_t', mag_t, 'out', out)
    frames_out = _own_or_given(frames_out, (B,), torch.int32, dev, who + ': frames_out')
    src = _own_or_given(src, (B, Fo), torch.int32, dev, who + ': src')
    on_gpu(who, 'mag_t', dev)
    _check(_lib.taco_frames_stretch_curve(ptr(mag_t), ptr(frames), frames_per_unit, ptr(dur_q), ptr(out), ptr(frames_out), ptr(src), B, Cw,
                                          F, Fo, stream_ptr()), 'taco_frames_stretch_curve')
    return out, frames_out, src


def frames_pitch_curve(mag_t, frames=None, step_q=None, frames_per_unit=1, lifter=32, out=None):
    """A pitch contour (include/taco_hip.h taco_frames_pitch_curve): frames_pitch with a step per frame.  step_q: (B, F) int32 on the
    device (pitch_step(semitones) per frame; clamped there to [32768, 131072], never read here) or None (65536: a copy).  Frame f has
    the bits frames_pitch gives it at the row step step_q[b, f]; a frame at 65536 is its input bit for bit.  Everything else as
    frames_pitch."""
    who = 'frames_pitch_curve'
    B, Cw, F, dev, frames_per_unit, lifter = _cepstrum_args(who, mag_t, lifter, frames, frames_per_unit, first=1)
    tensor_arg(who, 'step_q', step_q, torch.int32, (B, F), dev, optional=True)
    out = _own_or_given(out, (B, Cw, F), torch.float32, dev, who + ': out')
    no_overlap(who, 'mag_t', mag_t, 'out', out)
    on_gpu(who, 'mag_t', dev)
    _check(_lib.taco_frames_pitch_curve(ptr(mag_t), ptr(frames), frames_per_unit, ptr(step_q), lifter, ptr(out), B, Cw, F, stream_ptr()),
           'taco_frames_pitch_curve')
    return out


SHARPEN_FIRST, SHARPEN_MIN_BETA, SHARPEN_MAX_BETA = 2, -1.0, 1.0   # include/taco_hip.h
SHARPEN_LIFTER = 32   # UNTUNED, like every beta: nobody has listened


def _cepstrum_args(who, mag_t, lifter, frames, frames_per_unit, first=SHARPEN_FIRST):
    """the argument checks the cepstral wrappers share (first: the smallest lifter) -> (B, C, F, device, frames_per_unit, lifter)"""
    B, Cw, F = tensor_arg(who, 'mag_t', mag_t, torch.float32, ('B', 'C', 'F'))
    dev = mag_t.device
    pow2_bins(who, Cw)
    _frames_cap(who, F)
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    lifter = int_arg(who, 'lifter (at C = %d)' % Cw, lifter, first, min(PITCH_MAX_LIFTER, (Cw - 1) // 2))
    return B, Cw, F, dev, frames_per_unit, lifter


def frames_sharpen(mag_t, beta, lifter=SHARPEN_LIFTER, frames=None, frames_per_unit=1, out=None):
    """The cepstral post-filter (include/taco_hip.h taco_frames_sharpen): mag_t (B, C, F) fp32 on the device, C - 1 a power of two in
    [8, 1024] -> out (B, C, F) fp32: in the first F_b = clamp(frames[b] * frames_per_unit, 0, F) frames of row b the quefrencies
    2 .. lifter of the frame's cepstrum are scaled by 1 + beta at unchanged frame energy, zeros behind.  beta: a number in [-1, 1]
    for the whole batch; 0 is a bit copy.  lifter: 2 .. min(64, (C - 1) / 2); the default 32 is untuned.  frames: (B) int32 on the
    device, or None (all F frames).  out: the caller's own buffer; default: a fresh one.  Enqueued on the current stream; nothing
    is read back and nothing waits."""
    who = 'frames_sharpen'
    B, Cw, F, dev, frames_per_unit, lifter = _cepstrum_args(who, mag_t, lifter, frames, frames_per_unit)
    beta = float_arg(who, 'beta', beta, SHARPEN_MIN_BETA, SHARPEN_MAX_BETA)
    out = _own_or_given(out, (B, Cw, F), torch.float32, dev, who + ': out')
    no_overlap(who, 'mag_t', mag_t, 'out', out)
    on_gpu(who, 'mag_t', dev)
    _check(_lib.taco_frames_sharpen(ptr(mag_t), ptr(frames), frames_per_unit, beta, lifter, ptr(out), B, Cw, F, stream_ptr()),
           'taco_frames_sharpen')
    return out


def formant_step(semitones) -> int:
    """A formant shift in semitones (0: the model's own, +12 moves the envelope an octave up) -> step_q of taco_frames_formant =
    round(65536 * 2^(-semitones / 12)): the arithmetic of pitch_step; ValueError outside [-12, 12] or for a non-finite value"""
    try:
        semitones = float(semitones)
    except (TypeError, ValueError):
        raise ValueError('formant must be a number of semitones in [-12, 12], got %r' % (semitones,)) from None
    if not -12.0 <= semitones <= 12.0:   # (NaN fails both comparisons)
        raise ValueError('formant must be in [-12, 12] semitones, got %r' % (semitones,))
    return int(round(65536.0 * 2.0 ** (-semitones / 12.0)))


def frames_formant(mag_t, frames=None, step_q=None, frames_per_unit=1, lifter=32, out=None):
    """Timbre on the magnitude frames (include/taco_hip.h taco_frames_formant), the dual of frames_pitch: mag_t (B, C, F) fp32 on the
    device, C - 1 a power of two in [8, 1024] -> out (B, C, F) fp32: in the first F_b = clamp(frames[b] * frames_per_unit, 0, F)
    frames of row b the frame's own log-envelope (the cepstrum's quefrencies 0 .. lifter) is read at step_q[b] / 65536 source bins
    per output bin under the unmoved log-excitation, at unchanged frame energy; zeros behind.
    frames: (B) int32 on the device, or None (all F frames).  step_q: None (65536: a copy), an int (the whole batch), a host sequence
    of B ints (checked against [32768, 131072], then uploaded) or a (B) int32 tensor on the device (clamped there, never read here);
    formant_step(semitones) makes one.  lifter: 1 .. min(64, (C - 1) / 2); the default 32 is untuned.  out: the caller's own buffer;
    default: a fresh one.  Enqueued on the current stream; nothing is read back and nothing waits."""
    who = 'frames_formant'
    B, Cw, F, dev, frames_per_unit, lifter = _cepstrum_args(who, mag_t, lifter, frames, frames_per_unit, first=1)
    step_q, _ = step_q_arg(who, step_q, B, dev, PITCH_MIN_STEP, PITCH_MAX_STEP, '+12 to -12 semitones')
    out = _own_or_given(out, (B, Cw, F), torch.float32, dev, who + ': out')
    no_overlap(who, 'mag_t', mag_t, 'out', out)
    on_gpu(who, 'mag_t', dev)
    _check(_lib.taco_frames_formant(ptr(mag_t), ptr(frames), frames_per_unit, ptr(step_q), lifter, ptr(out), B, Cw, F, stream_ptr()),
           'taco_frames_formant')
    return out


def frames_cepstats_workspace_bytes(B, C_bins, F, lifter=SHARPEN_LIFTER) -> int:
    return _size('taco_frames_cepstats_workspace_bytes', B, C_bins, F, lifter)


def frames_cepstats(mag_t, lifter=SHARPEN_LIFTER, frames=None, frames_per_unit=1, out=None, workspace=None):
    """The raw material of the global variance (include/taco_hip.h taco_frames_cepstats): mag_t (B, C, F) fp32 on the device ->
    (sums (B, lifter + 1, 2) fp64, count (B) int32), device tensors: per row the sums over its first F_b frames of each cepstral
    coefficient c[n], n = 0 .. lifter, and of its square, and F_b.  gv_variance() makes variances of them on the host.  frames: (B)
    int32 on the device, or None.  out: the caller's own (sums, count); workspace: uint8, frames_cepstats_workspace_bytes(B, C, F,
    lifter) bytes; default: fresh ones.  Enqueued on the current stream; nothing is read back and nothing waits."""
    who = 'frames_cepstats'
    B, Cw, F, dev, frames_per_unit, lifter = _cepstrum_args(who, mag_t, lifter, frames, frames_per_unit)
    if out is not None and len(out) != 2:
        raise ValueError('%s: out must be (sums, count)' % who)
    sums = _own_or_given(None if out is None else out[0], (B, lifter + 1, 2), torch.float64, dev, who + ': sums')
    count = _own_or_given(None if out is None else out[1], (B,), torch.int32, dev, who + ': count')
    if workspace is not None:
        tensor_arg(who, 'workspace', workspace, torch.uint8, ('bytes',), dev)
    on_gpu(who, 'mag_t', dev)
    workspace = _own_or_given(workspace, (frames_cepstats_workspace_bytes(B, Cw, F, lifter),), torch.uint8, dev, who + ': workspace')
    _check(_lib.taco_frames_cepstats(ptr(mag_t), ptr(frames), frames_per_unit, lifter, ptr(sums), ptr(count), ptr(workspace), B, Cw, F,
                                     stream_ptr()), 'taco_frames_cepstats')
    return sums, count


def gv_variance(sums, count):
    """sums (..., Q + 1, 2) and count (...) as frames_cepstats returns them, on the HOST (NumPy) -> var (..., Q + 1) float64:
    sums[n, 1] / count - (sums[n, 0] / count)^2; NaN where count < 2"""
    sums, count = np.asarray(sums, dtype=np.float64), np.asarray(count, dtype=np.float64)[..., None]
    with np.errstate(divide='ignore', invalid='ignore'):
        var = sums[..., 1] / count - (sums[..., 0] / count) ** 2
    return np.where(count >= 2, var, np.nan)


def gv_ratio(sums_pred, n_pred, sums_rec, n_rec):
    """The global-variance ratio per utterance, on the HOST: exp(mean over n = 1 .. Q of log(var_pred[n] / var_rec[n])) of this
    model's linear-frequency cepstra -- below 1: the prediction is over-smoothed.  NaN for an utterance with fewer than 2 frames
    on either side (or a variance that is not positive)."""
    vp, vr = gv_variance(sums_pred, n_pred)[..., 1:], gv_variance(sums_rec, n_rec)[..., 1:]
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.exp(np.log(vp / vr).mean(axis=-1))


F0_MAX_LAGS = 512          # TACO_F0_MAX_LAGS
F0_RATIO, F0_THRESHOLD = 0.9, 0.3   # UNTUNED defaults of the pick: nobody has compared them with a labelled pitch track


def f0_lags(sr=16000, fmin=60.0, fmax=400.0):
    """(lag_min, lag_max) of a pitch range in Hz at sample rate sr: floor(sr / fmax) .. floor(sr / fmin); 40 .. 266 by default"""
    sr, fmin, fmax = float(sr), float(fmin), float(fmax)
    if not 0.0 < fmin < fmax < sr:
        raise ValueError('f0_lags: need 0 < fmin < fmax < sr, got fmin = %r, fmax = %r, sr = %r' % (fmin, fmax, sr))
    return int(math.floor(sr / fmax)), int(math.floor(sr / fmin))


def f0_tables(sr=16000, fmin=60.0, fmax=400.0, deemphasis=0.97, C=1025, win_length=1200):
    """The tables of taco_frames_f0 for features made with pre-emphasis `deemphasis` and a periodic Hann window of win_length samples
    -> (weight (C) float32, gain (L) float32, lag_min, lag_max), host NumPy (computed in float64):
      weight[k] = 1 / |1 - a e^{-i pi k / (C - 1)}|^2, which undoes the pre-emphasis on the power spectrum (all ones for a = 0);
      gain[j] = wa[0] / wa[lag_min - 1 + j], wa the autocorrelation of the window zero-padded to N = 2 (C - 1): the window's own
      autocorrelation divided out of the frame's (Boersma's correction).
    ValueError when the lags do not fit C or the cap of 512, or the window does not cover lag_max + 1."""
    lag_min, lag_max = f0_lags(sr, fmin, fmax)
    C, win_length, a = int(C), int(win_length), float(deemphasis)
    pow2_bins('f0_tables', C)
    if not 0.0 <= a < 1.0:
        raise ValueError('f0_tables: deemphasis must be in [0, 1), got %r' % (deemphasis,))
    L = lag_max - lag_min + 3
    if not 2 <= lag_min <= lag_max <= C - 2 or L > F0_MAX_LAGS:
        raise ValueError('f0_tables: %g .. %g Hz at %g Hz are lags %d .. %d: need 2 <= lag_min <= lag_max <= %d and at most %d lags '
                         'with their neighbours' % (fmin, fmax, sr, lag_min, lag_max, C - 2, F0_MAX_LAGS))
    N = 2 * (C - 1)
    if not lag_max + 1 < win_length <= N:
        raise ValueError('f0_tables: win_length must be in (lag_max + 1, N] = (%d, %d], got %d' % (lag_max + 1, N, win_length))
    k = np.arange(C, dtype=np.float64)
    weight = 1.0 / (1.0 - 2.0 * a * np.cos(np.pi * k / (C - 1)) + a * a)
    w = np.zeros(N)
    w[:win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    wa = np.fft.irfft(np.abs(np.fft.rfft(w, 2 * N)) ** 2)   # (2 N points: no lag wraps around)
    lags = np.arange(lag_min - 1, lag_max + 2)
    return weight.astype(np.float32), (wa[0] / wa[lags]).astype(np.float32), lag_min, lag_max


def _f0_table(who, name, x, n, dev):
    """None, a (n) float32 tensor on `dev`, or host numbers (uploaded) -> None or the device tensor; ValueError"""
    if x is None or (torch.is_tensor(x) and x.device.type != 'cpu'):
        tensor_arg(who, name + ' on a device', x, torch.float32, (n,), dev, optional=True)
        return x
    host = np.asarray(x.numpy() if torch.is_tensor(x) else x, dtype=np.float32)
    if host.shape != (n,):
        raise ValueError('%s: %s must hold %d numbers, got shape %s' % (who, name, n, host.shape))
    return torch.from_numpy(np.ascontiguousarray(host)).to(dev)


def frames_f0(mag_t, frames=None, frames_per_unit=1, weight=None, gain=None, lag_min=40, lag_max=266, ratio=F0_RATIO,
              threshold=F0_THRESHOLD, want_acf=False, out=None):
    """The pitch of magnitude frames (include/taco_hip.h taco_frames_f0): mag_t (B, C, F) fp32 on the device, C - 1 a power of two in
    [8, 1024] -> (period (B, F), strength (B, F)) fp32, and acf (B, L, F) behind them with want_acf, L = lag_max - lag_min + 3: per
    frame the normalised autocorrelation over lags lag_min - 1 .. lag_max + 1 (the cosine transform of the weighted power spectrum,
    times gain), the first local maximum at or above ratio times the largest one, refined by a parabola: period in samples (F0 =
    sr / period), strength its height; both 0 for an unvoiced frame (no maximum, or strength below threshold) and behind F_b =
    clamp(frames[b] * frames_per_unit, 0, F).
    frames: (B) int32 on the device, or None (all F frames).  weight (C) / gain (L): None (ones), float32 device tensors, or host
    numbers (uploaded); f0_tables() makes them, with lag_min and lag_max (the defaults 40 .. 266 are 400 .. 60 Hz at 16 kHz).
    ratio 0.9 and threshold 0.3 are UNTUNED defaults.  out: the caller's own (period, strength) or (period, strength, acf); default:
    fresh ones.  Enqueued on the current stream; nothing is read back and nothing waits."""
    who = 'frames_f0'
    B, Cw, F = tensor_arg(who, 'mag_t', mag_t, torch.float32, ('B', 'C', 'F'))
    dev = mag_t.device
    pow2_bins(who, Cw)
    _frames_cap(who, F)
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    lag_min, lag_max = int_arg(who, 'lag_min', lag_min), int_arg(who, 'lag_max', lag_max)
    L = lag_max - lag_min + 3
    if not 2 <= lag_min <= lag_max <= Cw - 2 or L > F0_MAX_LAGS:
        raise ValueError('%s: need 2 <= lag_min <= lag_max <= %d at C = %d and at most %d lags with their neighbours, got lag_min = %d, '
                         'lag_max = %d' % (who, Cw - 2, Cw, F0_MAX_LAGS, lag_min, lag_max))
    ratio, threshold = float(ratio), float(threshold)
    if not 0.0 < ratio <= 1.0:   # (NaN fails)
        raise ValueError('%s: ratio must be in (0, 1], got %r' % (who, ratio))
    if threshold != threshold:
        raise ValueError('%s: threshold is NaN' % who)
    weight = _f0_table(who, 'weight', weight, Cw, dev)
    gain = _f0_table(who, 'gain', gain, L, dev)
    if out is not None and len(out) != (3 if want_acf else 2):
        raise ValueError('%s: out must be (period, strength%s)' % (who, ', acf' if want_acf else ''))
    period = _own_or_given(None if out is None else out[0], (B, F), torch.float32, dev, who + ': period')
    strength = _own_or_given(None if out is None else out[1], (B, F), torch.float32, dev, who + ': strength')
    acf = _own_or_given(None if out is None else out[2], (B, L, F), torch.float32, dev, who + ': acf') if want_acf else None
    for name, t in (('period', period), ('strength', strength), ('acf', acf)):
        no_overlap(who, 'mag_t', mag_t, name, t)
    on_gpu(who, 'mag_t', dev)
    _check(_lib.taco_frames_f0(ptr(mag_t), ptr(frames), frames_per_unit, ptr(weight), ptr(gain), lag_min, lag_max, ratio, threshold,
                               ptr(period), ptr(strength), ptr(acf), B, Cw, F, stream_ptr()), 'taco_frames_f0')
    return (period, strength, acf) if want_acf else (period, strength)


def f0_stats(period, other=None, frames=None, frames_per_unit=1, out=None):
    """Statistics of a pitch track (include/taco_hip.h taco_f0_stats): period (B, F) fp32 on the device, as frames_f0 returns it ->
    stats (B, 3) fp32 = (count, mean, population standard deviation) of log2(period) over the frames with period > 0 among the first
    F_b.  other (B, F): the statistics of log2(other) - log2(period) over the frames voiced in both: the octaves by which `period`
    is higher in pitch than `other` (12 x the mean: semitones).  Nothing is read back."""
    who = 'f0_stats'
    B, F = tensor_arg(who, 'period', period, torch.float32, ('B', 'F'))
    dev = period.device
    _frames_cap(who, F)
    tensor_arg(who, 'other', other, torch.float32, (B, F), dev, optional=True)
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    out = _own_or_given(out, (B, 3), torch.float32, dev, who + ': out')
    on_gpu(who, 'period', dev)
    _check(_lib.taco_f0_stats(ptr(period), ptr(other), ptr(frames), frames_per_unit, ptr(out), B, F, stream_ptr()), 'taco_f0_stats')
    return out


F0_RANGE_MAX_SCALE, F0_RANGE_MAX_SMOOTH = 4.0, 8   # include/taco_hip.h: scale_q up to 4 x 65536, TACO_F0_RANGE_MAX_SMOOTH
F0_RANGE_SMOOTH, F0_RANGE_LIMIT = 2, 0.5           # f0_range_curve's smooth and limit (octaves): UNTUNED, nobody has listened


def range_scale(k) -> int:
    """An intonation range factor (1: the contour as tracked, 0 flat, 1.5 every excursion half as wide again) -> scale_q of
    taco_f0_range_curve = round(65536 * k), the companion of pitch_step; ValueError outside [0, 4] or for a non-finite value"""
    try:
        if isinstance(k, bool):
            raise TypeError
        k = float(k)
    except (TypeError, ValueError):
        raise ValueError('the intonation range must be a factor in [0, 4], got %r' % (k,)) from None
    if not 0.0 <= k <= F0_RANGE_MAX_SCALE:   # (NaN fails both comparisons)
        raise ValueError('the intonation range must be in [0, 4], got %r' % (k,))
    return int(round(65536.0 * k))


def f0_range_curve(period, frames=None, frames_per_unit=1, scale_q=None, base_q=None, smooth=F0_RANGE_SMOOTH, limit=F0_RANGE_LIMIT,
                   out=None, want_stats=False):
    """The intonation range as a pitch curve (include/taco_hip.h taco_f0_range_curve): period (B, F) fp32 on the device, as frames_f0
    or f0_viterbi return it -> step_q (B, F) int32 for frames_pitch_curve, and with want_stats (step_q, stats (B, 3)), stats being
    f0_stats(period, None, frames, frames_per_unit) bit for bit: every frame's distance from the row's own level (the mean of
    log2(period) over its voiced frames) is multiplied by k = scale_q / 65536; unvoiced frames lie on the line between their voiced
    neighbours, the deviations are smoothed by a triangle of half-width `smooth` frames, and one frame's excursion changes by at
    most `limit` octaves.
    frames: (B) int32 on the device, or None (all F frames).  scale_q: None (65536: neutral, base_q or 65536 copied), an int
    (range_scale(k), the whole batch), a host sequence of B ints (checked against [0, 262144], then uploaded) or a (B) int32
    tensor on the device (clamped there, never read here).  base_q: None or (B, F) int32 on the device, a step curve to compose
    with (clamped there to [32768, 131072]).  smooth in 0 .. 8 and limit in (0, 1]: the defaults 2 and 0.5 are UNTUNED.  out: the
    caller's own step_q, or (step_q, stats) with want_stats; default: fresh ones.  Enqueued on the current stream; nothing is read
    back and nothing waits."""
    who = 'f0_range_curve'
    B, F = tensor_arg(who, 'period', period, torch.float32, ('B', 'F'))
    dev = period.device
    _frames_cap(who, F)
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    scale_q, _ = step_q_arg(who, scale_q, B, dev, 0, int(F0_RANGE_MAX_SCALE * 65536), 'range factors 0 to 4', name='scale_q')
    tensor_arg(who, 'base_q', base_q, torch.int32, (B, F), dev, optional=True)
    smooth = int_arg(who, 'smooth', smooth, 0, F0_RANGE_MAX_SMOOTH)
    limit = float_arg(who, 'limit', limit, 0.0, 1.0)
    if limit == 0.0:
        raise ValueError('%s: limit must be a number of octaves in (0, 1], got %r' % (who, limit))
    if want_stats and out is not None and (torch.is_tensor(out) or len(out) != 2):
        raise ValueError('%s: out must be (step_q, stats)' % who)
    step_q = _own_or_given(out[0] if want_stats and out is not None else out, (B, F), torch.int32, dev, who + ': step_q')
    stats = _own_or_given(None if out is None else out[1], (B, 3), torch.float32, dev, who + ': stats') if want_stats else None
    no_overlap(who, 'period', period, 'step_q', step_q)
    if base_q is not None:
        no_overlap(who, 'base_q', base_q, 'step_q', step_q)
    on_gpu(who, 'period', dev)
    _check(_lib.taco_f0_range_curve(ptr(period), ptr(frames), frames_per_unit, ptr(scale_q), ptr(base_q), smooth, limit, ptr(step_q),
                                    ptr(stats), B, F, stream_ptr()), 'taco_f0_range_curve')
    return (step_q, stats) if want_stats else step_q


F0_MAX_CAND = 15           # TACO_F0_MAX_CAND
F0_CANDIDATES = 4          # candidates kept per frame by default: UNTUNED
F0_VITERBI_COUNTS = ('frames', 'voiced', 'moved', 'switches')   # the columns of f0_viterbi's counts
F0_OCTAVE_COST, F0_JUMP_COST, F0_SWITCH_COST = 0.01, 0.35, 0.14   # Praat's defaults (Boersma 1993), per 0.01 s of frame period: UNTUNED


def f0_viterbi_lag_tables(lag_min, lag_max, octave_cost=F0_OCTAVE_COST):
    """(bias (L) float32, lg (L) float32) of f0_viterbi for the lags lag_min - 1 .. lag_max + 1 (f0_viterbi_tables has the formulas);
    float64 on the host, rounded once"""
    who = 'f0_viterbi_lag_tables'
    lag_min, lag_max = int_arg(who, 'lag_min', lag_min, 2), int_arg(who, 'lag_max', lag_max)
    if lag_max < lag_min or lag_max - lag_min + 3 > F0_MAX_LAGS:
        raise ValueError('%s: need lag_min <= lag_max and at most %d lags with their neighbours, got lag_min = %d, lag_max = %d'
                         % (who, F0_MAX_LAGS, lag_min, lag_max))
    octave_cost = float(octave_cost)
    if not (0.0 <= octave_cost < math.inf):   # (NaN fails)
        raise ValueError('%s: octave_cost must be finite and not negative, got %r' % (who, octave_cost))
    lags = np.arange(lag_min - 1, lag_max + 2, dtype=np.float64)
    return (octave_cost * np.log2(lags / lag_max)).astype(np.float32), np.log2(lags).astype(np.float32)


def f0_viterbi_tables(sr=16000, fmin=60.0, fmax=400.0, octave_cost=F0_OCTAVE_COST, hop=300):
    """The tables and costs of f0_viterbi for frames `hop` samples apart -> (bias (L) float32, lg (L) float32, jump_cost, switch_cost),
    host NumPy computed in float64 and rounded once; row j is the lag lag_min - 1 + j of f0_lags(sr, fmin, fmax):
      lg[j] = log2(lag_j);
      bias[j] = octave_cost * log2(lag_j / lag_max): <= 0 up to lag_max and zero at the lowest pitch, so that a shorter lag of the same
      height scores higher (Praat's octave cost);
      jump_cost, switch_cost = Praat's 0.35 and 0.14 times 0.01 s / (hop / sr), its own correction for the frame period.
    All of them are UNTUNED: nobody has compared them with a labelled pitch track."""
    lag_min, lag_max = f0_lags(sr, fmin, fmax)
    L = lag_max - lag_min + 3
    if lag_min < 2 or L > F0_MAX_LAGS:
        raise ValueError('f0_viterbi_tables: %g .. %g Hz at %g Hz are lags %d .. %d: need lag_min >= 2 and at most %d lags with their '
                         'neighbours' % (fmin, fmax, sr, lag_min, lag_max, F0_MAX_LAGS))
    octave_cost, hop = float(octave_cost), float(hop)
    if not (0.0 <= octave_cost < math.inf):   # (NaN fails)
        raise ValueError('f0_viterbi_tables: octave_cost must be finite and not negative, got %r' % (octave_cost,))
    if not (0.0 < hop < math.inf):
        raise ValueError('f0_viterbi_tables: hop must be a positive number of samples, got %r' % (hop,))
    bias, lg = f0_viterbi_lag_tables(lag_min, lag_max, octave_cost)
    scale = 0.01 / (hop / float(sr))
    return bias, lg, F0_JUMP_COST * scale, F0_SWITCH_COST * scale


def _f0_viterbi_shape(who, B, L, F, K):
    B, L, F = int_arg(who, 'B', B, 1, _INT_MAX), int_arg(who, 'L', L, 3, F0_MAX_LAGS), int_arg(who, 'F', F, 1)
    _frames_cap(who, F)
    return B, L, F, int_arg(who, 'candidates', K, 1, F0_MAX_CAND)


def f0_viterbi_workspace_bytes(B, L, F, K) -> int:
    return _size('taco_f0_viterbi_workspace_bytes', *_f0_viterbi_shape('f0_viterbi_workspace_bytes', B, L, F, K))


def _cost_arg(who, name, x) -> float:
    x = float(x)
    if not (0.0 <= x < math.inf) or not (C.c_float(x).value < math.inf):   # (NaN fails; so does what rounds to infinity in float32)
        raise ValueError('%s: %s must be finite and not negative, got %r' % (who, name, x))
    return x


def f0_viterbi(acf, frames=None, frames_per_unit=1, lag_min=40, lag_max=266, bias=None, lg=None, candidates=F0_CANDIDATES,
               threshold=F0_THRESHOLD, jump_cost=None, switch_cost=None, out=None, workspace=None):
    """A pitch track smoothed across frames (include/taco_hip.h taco_f0_viterbi): acf (B, L, F) fp32 on the device as
    frames_f0(..., want_acf=True) returns it, L = lag_max - lag_min + 3 -> (period (B, F) fp32, strength (B, F) fp32 with the meaning
    of frames_f0's, counts (B, 4) int32 in the order F0_VITERBI_COUNTS, score (B) fp32), device tensors.  Per frame the `candidates`
    highest local maxima of acf minus bias are kept, and one of them or "unvoiced" (which scores `threshold`) is chosen per frame by
    the best path under jump_cost per octave between consecutive voiced frames and switch_cost per voiced / unvoiced switch.
    frames: (B) int32 on the device, or None.  bias (L): None (zeros), a float32 device tensor or host numbers; lg (L): the log2 of
    every row's lag, likewise -- None: the table of f0_viterbi_tables for these lags.  jump_cost / switch_cost None: those of
    f0_viterbi_tables() (16 kHz, hop 300).  All defaults are UNTUNED.  With both costs 0 and no bias the result is frames_f0's at
    ratio = 1.  out: the caller's own (period, strength, counts, score); workspace: uint8, f0_viterbi_workspace_bytes(B, L, F,
    candidates) bytes; default: fresh ones.  Enqueued on the current stream; nothing is read back and nothing waits."""
    who = 'f0_viterbi'
    B, L, F = tensor_arg(who, 'acf', acf, torch.float32, ('B', 'L', 'F'))
    dev = acf.device
    _frames_cap(who, F)
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    lag_min, lag_max = int_arg(who, 'lag_min', lag_min), int_arg(who, 'lag_max', lag_max)
    if not 2 <= lag_min <= lag_max or lag_max - lag_min + 3 > F0_MAX_LAGS:
        raise ValueError('%s: need 2 <= lag_min <= lag_max and at most %d lags with their neighbours, got lag_min = %d, lag_max = %d'
                         % (who, F0_MAX_LAGS, lag_min, lag_max))
    if L != lag_max - lag_min + 3:
        raise ValueError('%s: acf must have lag_max - lag_min + 3 = %d rows, got %d' % (who, lag_max - lag_min + 3, L))
    K = int_arg(who, 'candidates', candidates, 1, F0_MAX_CAND)
    threshold = float(threshold)
    if not (-math.inf < threshold < math.inf) or not (abs(C.c_float(threshold).value) < math.inf):
        raise ValueError('%s: threshold must be finite, got %r' % (who, threshold))
    if jump_cost is None or switch_cost is None:
        _, _, jump_d, switch_d = f0_viterbi_tables()
        jump_cost, switch_cost = jump_d if jump_cost is None else jump_cost, switch_d if switch_cost is None else switch_cost
    jump_cost, switch_cost = _cost_arg(who, 'jump_cost', jump_cost), _cost_arg(who, 'switch_cost', switch_cost)
    if lg is None:
        lg = f0_viterbi_lag_tables(lag_min, lag_max)[1]
    bias = _f0_table(who, 'bias', bias, L, dev)
    lg = _f0_table(who, 'lg', lg, L, dev)
    if out is not None and len(out) != 4:
        raise ValueError('%s: out must be (period, strength, counts, score)' % who)
    period = _own_or_given(None if out is None else out[0], (B, F), torch.float32, dev, who + ': period')
    strength = _own_or_given(None if out is None else out[1], (B, F), torch.float32, dev, who + ': strength')
    counts = _own_or_given(None if out is None else out[2], (B, len(F0_VITERBI_COUNTS)), torch.int32, dev, who + ': counts')
    score = _own_or_given(None if out is None else out[3], (B,), torch.float32, dev, who + ': score')
    for name, t in (('period', period), ('strength', strength), ('counts', counts), ('score', score)):
        no_overlap(who, 'acf', acf, name, t)
    if workspace is not None:
        tensor_arg(who, 'workspace', workspace, torch.uint8, ('bytes',), dev)
    on_gpu(who, 'acf', dev)
    workspace = _own_or_given(workspace, (f0_viterbi_workspace_bytes(B, L, F, K),), torch.uint8, dev, who + ': workspace')
    _check(_lib.taco_f0_viterbi(ptr(acf), ptr(frames), frames_per_unit, ptr(bias), ptr(lg), lag_min, lag_max, K, threshold, jump_cost,
                                switch_cost, ptr(period), ptr(strength), ptr(counts), ptr(score), ptr(workspace), B, F, stream_ptr()),
           'taco_f0_viterbi')
    return period, strength, counts, score


DTW_MAX_FRAMES, DTW_MAX_K, DTW_MAX_C = 1024, 32, 128   # TACO_DTW_MAX_FRAMES / _K / _C
MCD_DB = 10.0 * math.sqrt(2.0) / math.log(10.0)        # mel-cepstral distortion in dB per unit of Euclidean cepstral distance


def dct_basis(C=80, first=1, count=13):
    """Rows first .. first + count - 1 of the orthonormal DCT-II over C points, (count, C) float32 on the host, computed in float64
    and rounded once: row k is sqrt(2 / C) cos(pi (c + 1/2) k / C), row 0 is sqrt(1 / C).  The default leaves out c0 (the frame's
    mean log energy) and keeps the 13 cepstral coefficients MCD is usually taken over."""
    C, first, count = int(C), int(first), int(count)
    if C < 1 or first < 0 or count < 1 or first + count > C:
        raise ValueError('dct_basis: need C >= 1, first >= 0, count >= 1 and first + count <= C, got C = %d, first = %d, count = %d'
                         % (C, first, count))
    k = np.arange(first, first + count, dtype=np.float64)[:, None]
    c = np.arange(C, dtype=np.float64)[None, :]
    rows = np.sqrt(2.0 / C) * np.cos(np.pi * (c + 0.5) * k / C)
    rows[k[:, 0] == 0] = np.sqrt(1.0 / C)
    return rows.astype(np.float32)


def _frames_arg(who, name, x):
    """chronological frames (B, F, C) fp32 -> (B, F, C)"""
    return tensor_arg(who, name, x, torch.float32, ('B', 'F', 'C'))


def frames_active(x, floor, n=None):
    """Frames in use per row (include/taco_hip.h taco_frames_active): x (B, F, C) fp32 chronological frames on the device ->
    n (B) int32 on the device, 1 + the last frame with an element above `floor` (0: none; a NaN is not above anything).  Enqueued on
    the current stream; nothing is copied and nothing waits.  n: the caller's own buffer; default: a fresh one."""
    who = 'frames_active'
    B, F, Cw = _frames_arg(who, 'x', x)
    floor = float(floor)
    if floor != floor:
        raise ValueError('%s: floor is NaN' % who)
    n = _own_or_given(n, (B,), torch.int32, x.device, who + ': n')
    on_gpu(who, 'x', x.device)
    _check(_lib.taco_frames_active(ptr(x), floor, ptr(n), B, F, Cw, stream_ptr()), 'taco_frames_active')
    return n


def _dtw_args(who, a, b, na, nb, basis, cost, steps):
    """the argument checks frame_dtw and frame_dtw_path share -> (B, Fa, Fb, C, K, device, cost, steps)"""
    B, Fa, Cw = _frames_arg(who, 'a', a)
    dev = a.device
    Fb, = tensor_arg(who, 'b', b, torch.float32, (B, 'Fb', Cw), dev)
    if max(Fa, Fb) > DTW_MAX_FRAMES or Cw > DTW_MAX_C:
        raise ValueError('%s: at most %d frames of %d channels, got Fa = %d, Fb = %d, C = %d' % (who, DTW_MAX_FRAMES, DTW_MAX_C, Fa, Fb, Cw))
    tensor_arg(who, 'na', na, torch.int32, (B,), dev, optional=True)
    tensor_arg(who, 'nb', nb, torch.int32, (B,), dev, optional=True)
    K = Cw if basis is None else tensor_arg(who, 'basis', basis, torch.float32, ('K', Cw), dev)[0]
    if K > DTW_MAX_K:
        raise ValueError('%s: at most %d coefficients per frame, got %d%s'
                         % (who, DTW_MAX_K, K, ' (no basis: the channels themselves)' if basis is None else ''))
    cost = _own_or_given(cost, (B,), torch.float32, dev, who + ': cost')
    steps = _own_or_given(steps, (B,), torch.int32, dev, who + ': steps')
    return B, Fa, Fb, Cw, K, dev, cost, steps


def frame_dtw_workspace_bytes(B, Fa, Fb, K) -> int:
    return _size('taco_frame_dtw_workspace_bytes', B, Fa, Fb, K)


def frame_dtw(a, b, na=None, nb=None, basis=None, cost=None, steps=None, work=None):
    """Dynamic time warping per batch row (include/taco_hip.h taco_frame_dtw): a (B, Fa, C), b (B, Fb, C) fp32 chronological frames,
    na / nb (B) int32 or None (all Fa / Fb frames), basis (K, C) fp32 or None (the channels themselves), all on the device ->
    (cost (B) fp32, steps (B) int32), device tensors: the summed Euclidean distance of the coefficient vectors along the cheapest
    warping path and the number of cells on it; cost / steps is the mean distance per step, MCD_DB times that the distortion in dB.
    Enqueued on the current stream; nothing is copied and nothing waits.  cost / steps / work: the caller's own buffers (work: uint8,
    frame_dtw_workspace_bytes(B, Fa, Fb, K) bytes); default: fresh ones."""
    who = 'frame_dtw'
    B, Fa, Fb, Cw, K, dev, cost, steps = _dtw_args(who, a, b, na, nb, basis, cost, steps)
    on_gpu(who, 'a', dev)
    nbytes = frame_dtw_workspace_bytes(B, Fa, Fb, K)
    work = _own_or_given(work, (nbytes,), torch.uint8, dev, who + ': work')
    _check(_lib.taco_frame_dtw(ptr(a), ptr(na), ptr(b), ptr(nb), ptr(basis), ptr(cost), ptr(steps), ptr(work) if nbytes else None,
                               B, Fa, Fb, Cw, K, stream_ptr()), 'taco_frame_dtw')
    return cost, steps


def frame_dtw_path_workspace_bytes(B, Fa, Fb, K) -> int:
    return _size('taco_frame_dtw_path_workspace_bytes', B, Fa, Fb, K)


def frame_dtw_path(a, b, na=None, nb=None, basis=None, cost=None, steps=None, path_a=None, path_b=None, work=None):
    """frame_dtw with the warping path (include/taco_hip.h taco_frame_dtw_path): the same arguments, the same cost and steps bit for
    bit -> (cost, steps, path_a, path_b); path_a / path_b (B, Fa + Fb - 1) int32: entries t < steps[b] are the cells (i_t, j_t) of the
    path from (0, 0) to (na - 1, nb - 1), the rest -1.  work: uint8, frame_dtw_path_workspace_bytes(B, Fa, Fb, K) bytes (never 0: the
    direction table, a byte per cell of Fa + Fb - 1 diagonals of Fa).  Enqueued on the current stream; nothing is copied and nothing
    waits.  The outputs and work: the caller's own buffers; default: fresh ones."""
    who = 'frame_dtw_path'
    B, Fa, Fb, Cw, K, dev, cost, steps = _dtw_args(who, a, b, na, nb, basis, cost, steps)
    P = Fa + Fb - 1
    path_a = _own_or_given(path_a, (B, P), torch.int32, dev, who + ': path_a')
    path_b = _own_or_given(path_b, (B, P), torch.int32, dev, who + ': path_b')
    on_gpu(who, 'a', dev)
    work = _own_or_given(work, (frame_dtw_path_workspace_bytes(B, Fa, Fb, K),), torch.uint8, dev, who + ': work')
    _check(_lib.taco_frame_dtw_path(ptr(a), ptr(na), ptr(b), ptr(nb), ptr(basis), ptr(cost), ptr(steps), ptr(path_a), ptr(path_b),
                                    ptr(work), B, Fa, Fb, Cw, K, stream_ptr()), 'taco_frame_dtw_path')
    return cost, steps, path_a, path_b


PATH_SCORE_COUNTS = ('cells', 'both_voiced', 'a_only', 'b_only', 'gross')   # the columns of path_f0_scores' counts


def path_f0_scores(period_a, period_b, path_a, path_b, steps, gross=1.2, counts=None, means=None):
    """Two pitch tracks compared along a warping path (include/taco_hip.h taco_path_f0_scores): period_a (B, Fa), period_b (B, Fb)
    fp32 as frames_f0 returns them, path_a / path_b (B, Fa + Fb - 1) int32 and steps (B) int32 as frame_dtw_path returns them, all on
    the device -> (counts (B, 5) int32 in the order PATH_SCORE_COUNTS, means (B, 2) fp32: the mean and the root mean square of
    log2(period_b) - log2(period_a) over the cells voiced in both -- the octaves by which a lies above b; x 1200: cents).  A cell is a
    gross error when one period is more than `gross` times the other.  Nothing is read back."""
    who = 'path_f0_scores'
    B, Fa = tensor_arg(who, 'period_a', period_a, torch.float32, ('B', 'Fa'))
    dev = period_a.device
    Fb, = tensor_arg(who, 'period_b', period_b, torch.float32, (B, 'Fb'), dev)
    if max(Fa, Fb) > DTW_MAX_FRAMES:
        raise ValueError('%s: at most %d frames, got Fa = %d, Fb = %d' % (who, DTW_MAX_FRAMES, Fa, Fb))
    P = Fa + Fb - 1
    for name, t, shape in (('path_a', path_a, (B, P)), ('path_b', path_b, (B, P)), ('steps', steps, (B,))):
        tensor_arg(who, name, t, torch.int32, shape, dev)
    gross = float(gross)
    if not gross > 1.0 or not C.c_float(gross).value > 1.0:   # (NaN fails)
        raise ValueError('%s: gross must be above 1 (as a float32 too), got %r' % (who, gross))
    counts = _own_or_given(counts, (B, 5), torch.int32, dev, who + ': counts')
    means = _own_or_given(means, (B, 2), torch.float32, dev, who + ': means')
    on_gpu(who, 'period_a', dev)
    _check(_lib.taco_path_f0_scores(ptr(period_a), ptr(period_b), ptr(path_a), ptr(path_b), ptr(steps), gross, ptr(counts), ptr(means),
                                    B, Fa, Fb, stream_ptr()), 'taco_path_f0_scores')
    return counts, means


def corpus_batch_width(src_addr, out_addr, row, fp16) -> int:
    """Elements per thread and access taco_corpus_batch picks (include/taco_hip.h): the largest V in {8 (fp16 only), 4, 2, 1}
    with row % V == 0, the source address a multiple of V elements and the output address a multiple of min(V, 4) floats.
    Pure host arithmetic, the restatement of the library's rule; V = 8 is the 16-byte vector path, V = 1 the scalar one."""
    esz = 2 if fp16 else 4
    v = 8 if fp16 else 4
    while v > 1:
        if row % v == 0 and src_addr % (v * esz) == 0 and out_addr % (min(v, 4) * 4) == 0:
            return v
        v >>= 1
    return 1


def _corpus_batch_args(src, mean, std, index, n_bad):
    """The argument check of corpus_batch -> (N, row, C, B, device); ValueError before any library call."""
    who = 'corpus_batch'
    N, Td, Cw = tensor_arg(who, 'src', src, (torch.float16, torch.float32), ('N', 'Td', 'C'))
    dev = src.device
    if (mean is None) != (std is None):
        raise ValueError('%s: mean and std must both be given or both be None' % who)
    tensor_arg(who, 'mean', mean, torch.float32, (Cw,), dev, optional=True)
    tensor_arg(who, 'std', std, torch.float32, (Cw,), dev, optional=True)
    B = N if index is None else tensor_arg(who, 'index', index, torch.int64, ('B',), dev)[0]
    if n_bad is not None and (not torch.is_tensor(n_bad) or n_bad.numel() != 1 or n_bad.dtype != torch.int32 or n_bad.device != dev):
        raise ValueError('%s: n_bad must be one int32 on %s' % (who, dev))   # (of any shape: (), (1,), (1, 1))
    on_gpu(who, 'src', dev)
    return N, Td * Cw, Cw, B, dev


def corpus_batch(src, mean, std, index=None, out=None, n_bad=None):
    """Batch gather with the corpus standardisation fused in (include/taco_hip.h taco_corpus_batch): src (N, Td, C) fp16 or fp32,
    mean / std (C) fp32 or both None (pure gather / widening), index (B) int64 on the device or None (identity, B = N) ->
    out (B, Td, C) fp32 = (float(src[index]) - mean) / std, NumPy's fp32 result bit for bit.  A row whose index is outside
    [0, N) comes out as zeros and is counted in n_bad (one int32 on the device, zeroed by the call) when given.  out: the
    caller's own buffer; default: a fresh one."""
    N, row, Cw, B, dev = _corpus_batch_args(src, mean, std, index, n_bad)
    out = _own_or_given(out, (B, row // Cw, Cw), torch.float32, dev, 'corpus_batch: out')
    _check(_lib.taco_corpus_batch(ptr(src), int(src.dtype == torch.float16), ptr(index), ptr(mean), ptr(std), ptr(out), ptr(n_bad),
                                  N, B, row, Cw, stream_ptr()), 'taco_corpus_batch')
    return out


def _griffinlim_args(who, mag_t, frames, phase0, frames_per_unit, n_iter, need_frames=False, need_phase0=False):
    """The argument check of the three Griffin-Lim wrappers -> (B, F, device, frames_per_unit, n_iter); ValueError names `who`."""
    B, F = tensor_arg(who, 'mag_t', mag_t, torch.float32, ('B', 1025, 'F'), empty_ok=True)   # (B >= 1, F >= 5: the size functions refuse)
    dev = mag_t.device
    tensor_arg(who, 'frames', frames, torch.int32, (B,), dev, optional=not need_frames)
    tensor_arg(who, 'phase0', phase0, torch.float32, (B, 1025, F), dev, optional=not need_phase0)
    if int(frames_per_unit) < 1 or int(n_iter) < 0:
        raise ValueError('%s: frames_per_unit >= 1 and n_iter >= 0, got %d and %d' % (who, frames_per_unit, n_iter))
    return B, F, dev, int(frames_per_unit), int(n_iter)


def griffinlim_workspace_floats(B, F) -> int:
    return _size('taco_griffinlim_workspace_bytes', B, F) // 4


def griffinlim(mag_t, phase0, n_iter=50, out=None, work=None):
    """mag_t, phase0 (B, 1025, F) -> waveform (B, 300 (F - 1)); audio.griffinlim on the GPU.  out / work: the caller's own
    waveform buffer and workspace (griffinlim_workspace_floats(B, F) floats); default: fresh ones."""
    B, F, dev, _, n_iter = _griffinlim_args('griffinlim', mag_t, None, phase0, 1, n_iter, need_phase0=True)
    work = _own_or_given(work, (griffinlim_workspace_floats(B, F),), torch.float32, dev, 'griffinlim: work')
    wave = _own_or_given(out, (B, 300 * (F - 1)), torch.float32, dev, 'griffinlim: out')
    _check(_lib.taco_griffinlim(ptr(mag_t), ptr(phase0), ptr(wave), ptr(work), B, F, n_iter, stream_ptr()), 'taco_griffinlim')
    return wave


def griffinlim_rows_workspace_floats(B, F) -> int:
    return _size('taco_griffinlim_rows_workspace_bytes', B, F) // 4


def griffinlim_rows(mag_t, frames, phase0=None, seed=0, n_iter=50, frames_per_unit=1, out=None, work=None):
    """Griffin-Lim per utterance (include/taco_hip.h taco_griffinlim_rows): mag_t (B, 1025, F), frames (B) int32 on the device ->
    waveform (B, 300 (F - 1)); row b is the Griffin-Lim of its first F_b = min(F, frames[b] * frames_per_unit) frames, 0 from
    sample 300 (F_b - 1) on.  phase0 (B, 1025, F) initial angles, or None: seeded phases drawn on the device.  out / work: the
    caller's own waveform buffer and workspace (griffinlim_rows_workspace_floats(B, F) floats); default: fresh ones."""
    B, F, dev, frames_per_unit, n_iter = _griffinlim_args('griffinlim_rows', mag_t, frames, phase0, frames_per_unit, n_iter,
                                                          need_frames=True)
    work = _own_or_given(work, (griffinlim_rows_workspace_floats(B, F),), torch.float32, dev, 'griffinlim_rows: work')
    wave = _own_or_given(out, (B, 300 * (F - 1)), torch.float32, dev, 'griffinlim_rows: out')
    _check(_lib.taco_griffinlim_rows(ptr(mag_t), ptr(phase0), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(frames), frames_per_unit,
                                     ptr(wave), ptr(work), B, F, n_iter, stream_ptr()), 'taco_griffinlim_rows')
    return wave


def griffinlim_fast_workspace_floats(B, F) -> int:
    return _size('taco_griffinlim_fast_workspace_bytes', B, F) // 4


def griffinlim_fast(mag_t, frames=None, phase0=None, seed=0, n_iter=50, momentum=0.99, frames_per_unit=1, want_conv=False,
                    out=None, conv=None, work=None):
    """Fast Griffin-Lim (include/taco_hip.h taco_griffinlim_fast): mag_t (B, 1025, F) -> waveform (B, 300 (F - 1)), or with
    want_conv (waveform, conv (B, n_iter + 1)): the spectral convergence in front of every round and, last, of the waveform
    returned.  momentum in [0, 1): 0 is the plain algorithm.  frames (B) int32 on the device, or None: every row has F frames.
    phase0 (B, 1025, F) initial angles, or None: seeded phases drawn on the device.  out / conv / work: the caller's own buffers
    (work: griffinlim_fast_workspace_floats(B, F) floats); default: fresh ones.  A conv buffer implies want_conv."""
    B, F, dev, frames_per_unit, n_iter = _griffinlim_args('griffinlim_fast', mag_t, frames, phase0, frames_per_unit, n_iter)
    momentum = _unit_interval(momentum, 'griffinlim_fast: momentum')
    want_conv = bool(want_conv) or conv is not None
    work = _own_or_given(work, (griffinlim_fast_workspace_floats(B, F),), torch.float32, dev, 'griffinlim_fast: work')
    wave = _own_or_given(out, (B, 300 * (F - 1)), torch.float32, dev, 'griffinlim_fast: out')
    conv = _own_or_given(conv, (B, n_iter + 1), torch.float32, dev, 'griffinlim_fast: conv') if want_conv else None
    _check(_lib.taco_griffinlim_fast(ptr(mag_t), ptr(phase0), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(frames), frames_per_unit,
                                     momentum, ptr(wave), ptr(conv), ptr(work), B, F, n_iter, stream_ptr()), 'taco_griffinlim_fast')
    return (wave, conv) if want_conv else wave


def phase_estimate_workspace_bytes(B, F) -> int:
    who = 'phase_estimate_workspace_bytes'
    return _size('taco_phase_estimate_workspace_bytes', int_arg(who, 'B', B, 1, _INT_MAX), int_arg(who, 'F', F, 1, _INT_MAX))


def phase_estimate(mag_t, frames=None, frames_per_unit=1, out=None, workspace=None):
    """Initial phases for Griffin-Lim read off the magnitudes (include/taco_hip.h taco_phase_estimate; single-pass spectrogram
    inversion): mag_t (B, 1025, F) fp32 on the device -> phase0 (B, 1025, F) fp32 radians, the `phase0` of griffinlim /
    griffinlim_rows / griffinlim_fast.  Row b is estimated over its first F_b = clamp(frames[b] * frames_per_unit, 0, F) frames,
    zeros behind.  frames: (B) int32 on the device, or None (all F frames).  out: the caller's own phase0; workspace: uint8,
    phase_estimate_workspace_bytes(B, F) bytes; default: fresh ones.  Enqueued on the current stream; nothing is read back and
    nothing waits."""
    who = 'phase_estimate'
    B, F = tensor_arg(who, 'mag_t', mag_t, torch.float32, ('B', 1025, 'F'))
    dev = mag_t.device
    frames_per_unit = _row_frames_arg(who, frames, frames_per_unit, B, dev)
    out = _own_or_given(out, (B, 1025, F), torch.float32, dev, who + ': out')
    no_overlap(who, 'mag_t', mag_t, 'out', out)
    if workspace is not None:
        tensor_arg(who, 'workspace', workspace, torch.uint8, ('bytes',), dev)
    on_gpu(who, 'mag_t', dev)
    workspace = _own_or_given(workspace, (phase_estimate_workspace_bytes(B, F),), torch.uint8, dev, who + ': workspace')
    _check(_lib.taco_phase_estimate(ptr(mag_t), ptr(frames), frames_per_unit, ptr(out), ptr(workspace), B, F, stream_ptr()),
           'taco_phase_estimate')
    return out


def wave_finish_workspace_floats(B, L) -> int:
    return _size('taco_wave_finish_workspace_bytes', B, L) // 4


def wave_finish(wave, samples=None, deemphasis=0.97, trim_top_db=0.0, want_out=True, want_pcm=True, out=None, pcm=None, bounds=None,
                peak=None, work=None):
    """Waveform finishing (include/taco_hip.h taco_wave_finish): wave (B, L) fp32 -> (out (B, L) fp32 or None, pcm (B, L) int16 or
    None, bounds (B, 2) int32, peak (B) fp32).  Per row: de-emphasis y[n] = x[n] + deemphasis * y[n-1] over its first n_b samples,
    the energy trim [s_b, e_b) at trim_top_db below the loudest frame (0: none), peak = max |y| inside it, then out = y[s_b : e_b]
    and pcm = write_wav's PCM16 of it, zeros behind.  samples (B) int32 on the device, or None: every row has L samples.
    deemphasis in [0, 1); trim_top_db >= 0.  out / pcm / bounds / peak / work: the caller's own buffers (work:
    wave_finish_workspace_floats(B, L) floats); default: fresh ones.  An out / pcm buffer implies want_out / want_pcm."""
    B, L = tensor_arg('wave_finish', 'wave', wave, torch.float32, ('B', 'L'))
    dev = wave.device
    tensor_arg('wave_finish', 'samples', samples, torch.int32, (B,), dev, optional=True)
    deemphasis, trim_top_db = _unit_interval(deemphasis, 'wave_finish: deemphasis'), float(trim_top_db)
    if not trim_top_db >= 0.0:
        raise ValueError('wave_finish: trim_top_db must be >= 0, got %r' % trim_top_db)
    want_out = bool(want_out) or out is not None
    want_pcm = bool(want_pcm) or pcm is not None
    if not (want_out or want_pcm):
        raise ValueError('wave_finish: at least one of out and pcm is needed')
    out = _own_or_given(out, (B, L), torch.float32, dev, 'wave_finish: out') if want_out else None
    if out is not None and out.data_ptr() == wave.data_ptr():
        raise ValueError('wave_finish: out may not alias wave')
    pcm = _own_or_given(pcm, (B, L), torch.int16, dev, 'wave_finish: pcm') if want_pcm else None
    bounds = _own_or_given(bounds, (B, 2), torch.int32, dev, 'wave_finish: bounds')
    peak = _own_or_given(peak, (B,), torch.float32, dev, 'wave_finish: peak')
    work = _own_or_given(work, (wave_finish_workspace_floats(B, L),), torch.float32, dev, 'wave_finish: work')
    _check(_lib.taco_wave_finish(ptr(wave), ptr(samples), deemphasis, trim_top_db, ptr(out), ptr(pcm), ptr(bounds), ptr(peak),
                                 ptr(work), B, L, stream_ptr()), 'taco_wave_finish')
    return out, pcm, bounds, peak


def wave_join_workspace_bytes(N, P, Lj) -> int:
    return _size('taco_wave_join_workspace_bytes', N, P, Lj)


def wave_join(pieces, bounds, first, gap, fade=0, Lj=None, want_out=True, want_pcm=True, out=None, pcm=None, offsets=None, total=None,
              peak=None, work=None):
    """Joins the finished pieces of long prompts (include/taco_hip.h taco_wave_join): pieces (N, L) fp32 on the device -- the `out` of
    wave_finish, or rows `pitch` >= L floats apart (a view with stride (pitch, 1)) -- and bounds (N, 2) int32 on the device, the
    `bounds` of wave_finish -> (out (P, Lj) fp32 or None, pcm (P, Lj) int16 or None, offsets (N) int32, total (P) int32, peak (P)
    fp32).  first: P + 1 host integers, the pieces of prompt p are rows first[p] .. first[p+1] - 1; gap: N host integers >= 0, the
    samples of silence behind each piece (ignored behind a prompt's last one); fade >= 0: samples of the linear ramp at every interior
    edge.  Prompt p's row holds its pieces at offsets[i], total[p] samples in all, zeros behind; pcm is scaled by the prompt's peak.
    Lj: the row length; default: the worst case max_p (K_p L + the prompt's gaps) rounded up to a multiple of 8, with which nothing is
    ever cut and the host needs no length from the device.  out / pcm / offsets / total / peak / work: the caller's own buffers (work:
    uint8, wave_join_workspace_bytes(N, P, Lj) bytes); default: fresh ones.  An out / pcm buffer implies want_out / want_pcm."""
    who = 'wave_join'
    if not torch.is_tensor(pieces) or pieces.dim() != 2 or pieces.dtype != torch.float32 or pieces.shape[0] < 1 or pieces.shape[1] < 1:
        raise ValueError('%s: pieces must be a float32 tensor of shape (N, L), got %s %s'
                         % (who, getattr(pieces, 'dtype', type(pieces)), tuple(getattr(pieces, 'shape', ()))))
    N, L = pieces.shape
    dev = pieces.device
    if L > 1 and pieces.stride(1) != 1:
        raise ValueError('%s: the samples of a piece must be contiguous, got strides %s' % (who, tuple(pieces.stride())))
    pitch = pieces.stride(0) if N > 1 else max(pieces.stride(0), L)
    if pitch < L:
        raise ValueError('%s: the rows of pieces are %d floats apart, fewer than L = %d' % (who, pitch, L))
    tensor_arg(who, 'bounds', bounds, torch.int32, (N, 2), dev)
    try:
        P = len(first) - 1
    except TypeError:
        raise ValueError('%s: first must be a sequence of P + 1 integers' % who) from None
    if P < 1:
        raise ValueError('%s: first must hold P + 1 >= 2 integers, got %d' % (who, P + 1))
    first = _host_int32(first, P + 1, who + ': first')
    gap = _host_int32(gap, N, who + ': gap')
    if first[0] != 0 or first[P] != N:
        raise ValueError('%s: first must start at 0 and end at N = %d, got %d and %d' % (who, N, first[0], first[P]))
    if any(first[p] > first[p + 1] for p in range(P)):
        raise ValueError('%s: first must not decrease, got %r' % (who, first))
    if min(gap) < 0:
        raise ValueError('%s: gap must be >= 0, got %d' % (who, min(gap)))
    fade = int_arg(who, 'fade', fade, 0)
    want_out = bool(want_out) or out is not None
    want_pcm = bool(want_pcm) or pcm is not None
    if not (want_out or want_pcm):
        raise ValueError('%s: at least one of out and pcm is needed' % who)
    if Lj is None:
        worst = max((first[p + 1] - first[p]) * L + sum(gap[first[p]:first[p + 1] - 1]) for p in range(P))
        Lj = max(8, -(-worst // 8) * 8)
    Lj = int_arg(who, 'Lj', Lj, 1, _INT_MAX)
    out = _own_or_given(out, (P, Lj), torch.float32, dev, who + ': out') if want_out else None
    no_overlap(who, 'pieces', pieces, 'out', out, span_in=((N - 1) * pitch + L) * 4)
    pcm = _own_or_given(pcm, (P, Lj), torch.int16, dev, who + ': pcm') if want_pcm else None
    offsets = _own_or_given(offsets, (N,), torch.int32, dev, who + ': offsets')
    total = _own_or_given(total, (P,), torch.int32, dev, who + ': total')
    peak = _own_or_given(peak, (P,), torch.float32, dev, who + ': peak')
    work = _own_or_given(work, (wave_join_workspace_bytes(N, P, Lj),), torch.uint8, dev, who + ': work')
    on_gpu(who, 'pieces', dev)
    _check(_lib.taco_wave_join(C.c_void_p(pieces.data_ptr()), pitch, ptr(bounds), (C.c_int32 * (P + 1))(*first), (C.c_int32 * N)(*gap),
                               fade, ptr(out), ptr(pcm), ptr(offsets), ptr(total), ptr(peak), ptr(work), N, P, L, Lj, stream_ptr()),
           'taco_wave_join')
    return out, pcm, offsets, total, peak

LOUD_CHUNK = 2048   # TACO_LOUD_CHUNK: the samples of a row that one workgroup of taco_wave_loudness filters


def _loud_sr(who, sr) -> int:
    sr = int_arg(who, 'sr', sr, 8000, 48000)
    if sr % 10:
        raise ValueError('%s: sr must be a multiple of 10 (a hop is sr / 10 samples), got %d' % (who, sr))
    return sr


def k_weighting(sr):
    """The K-weighting of ITU-R BS.1770 at sample rate sr (include/taco_hip.h taco_k_weighting; a host function): ten floats,
    b0 b1 b2 a1 a2 of the shelf, then of the high-pass.  sr: a multiple of 10 in [8000, 48000]."""
    sr = _loud_sr('k_weighting', sr)
    coef = (C.c_double * 10)()
    _check(_lib.taco_k_weighting(sr, coef), 'taco_k_weighting')
    return [float(c) for c in coef]


def wave_loudness_workspace_floats(B, L, sr) -> int:
    return _size('taco_wave_loudness_workspace_bytes', B, L, sr) // 4


def wave_loudness(wave, samples=None, sr=16000, target=None, ceiling=1.0, want_out=None, want_pcm=None, out=None, pcm=None, loud=None,
                  blocks=None, work=None):
    """Integrated loudness and a target level (include/taco_hip.h taco_wave_loudness): wave (B, L) fp32 -> (out (B, L) fp32 or None,
    pcm (B, L) int16 or None, loud (B, 4) fp32 = (I, M, g, peak_out), blocks (B, 4) int32 = (nb, past the absolute gate, past both
    gates, limited)).  Per row: the K-weighted mean squares of 400 ms blocks at 75 % overlap over its first n_b samples, gated at
    -70 LUFS and at 10 LU below the mean of what is left, give I (LUFS) and the maximum momentary loudness M; a row shorter than
    400 ms is one block.  target None: measure only (g = 1; out and pcm stay None).  target in [-70, 0] LUFS: out = wave * g with
    g = 10^((target - I) / 20), or ceiling / max |wave| where that would carry the peak above ceiling, in (0, 1]; pcm = PCM16 of
    out, zeros behind n_b.  samples (B) int32 on the device, or None: every row has L samples.  want_out / want_pcm default to
    whether there is a target.  out / pcm / loud / blocks / work: the caller's own buffers (work:
    wave_loudness_workspace_floats(B, L, sr) floats); default: fresh ones.  An out / pcm buffer implies want_out / want_pcm; out may
    be wave itself."""
    who = 'wave_loudness'
    B, L = tensor_arg(who, 'wave', wave, torch.float32, ('B', 'L'))
    dev = wave.device
    tensor_arg(who, 'samples', samples, torch.int32, (B,), dev, optional=True)
    sr = _loud_sr(who, sr)
    want_out = (target is not None if want_out is None else bool(want_out)) or out is not None
    want_pcm = (target is not None if want_pcm is None else bool(want_pcm)) or pcm is not None
    if target is None:
        if want_out or want_pcm:
            raise ValueError('%s: out and pcm need a target (target=None measures only)' % who)
        target, ceiling = 0.0, 1.0
    else:
        target, ceiling = float(target), float(ceiling)
        if not -70.0 <= target <= 0.0:   # (NaN fails)
            raise ValueError('%s: target must be in [-70, 0] LUFS, got %r' % (who, target))
        if not 0.0 < ceiling <= 1.0 or C.c_float(ceiling).value <= 0.0:
            raise ValueError('%s: ceiling must be in (0, 1], got %r' % (who, ceiling))
        if not (want_out or want_pcm):
            raise ValueError('%s: a target needs at least one of out and pcm' % who)
    out = _own_or_given(out, (B, L), torch.float32, dev, who + ': out') if want_out else None
    pcm = _own_or_given(pcm, (B, L), torch.int16, dev, who + ': pcm') if want_pcm else None
    loud = _own_or_given(loud, (B, 4), torch.float32, dev, who + ': loud')
    blocks = _own_or_given(blocks, (B, 4), torch.int32, dev, who + ': blocks')
    if work is not None:
        tensor_arg(who, 'work', work, torch.float32, ('floats',), dev)
    on_gpu(who, 'wave', dev)
    work = _own_or_given(work, (wave_loudness_workspace_floats(B, L, sr),), torch.float32, dev, who + ': work')
    _check(_lib.taco_wave_loudness(ptr(wave), ptr(samples), sr, target, ceiling, ptr(out), ptr(pcm), ptr(loud), ptr(blocks), ptr(work),
                                   B, L, stream_ptr()), 'taco_wave_loudness')
    return out, pcm, loud, blocks


LIMIT_CHUNK = 2048   # TACO_LIMIT_CHUNK: the samples of a row that one workgroup of taco_wave_limit handles
LIMIT_MAX_W = 512    # the longest look-ahead of taco_wave_limit, in samples
# The defaults of the true-peak limiter: 4 x oversampling, 12 taps per phase, Kaiser beta 6 (and 1.5 ms of look-ahead in
# griffinlim.level_waveform).  They are UNTUNED: chosen so that the meter reads tones within EBU Tech 3341's +0.2 / -0.4 dB
# (tests/test_wave_limit_host.py); nobody has listened to a limited file.
LIMIT_P, LIMIT_T, LIMIT_BETA = 4, 12, 6.0


def true_peak_taps(P=LIMIT_P, T=LIMIT_T, beta=LIMIT_BETA):
    """The interpolator of taco_wave_limit: a (P - 1, T) float32 array, phases 1 .. P - 1 of a Kaiser-windowed sinc.  Tap j of phase p
    sits at t = j - (T/2 - 1) - p/P samples: h = sinc(t) I0(beta sqrt(1 - (t / (T/2))^2)) / I0(beta), 0 where the root's argument is
    negative; each phase is divided by its own sum, in fp64, and rounded once.  P in 1..8 (P = 1: an empty table), T even in 2..32."""
    who = 'true_peak_taps'
    P, T = int_arg(who, 'P', P, 1, 8), int_arg(who, 'T', T, 2, 32)
    if T % 2:
        raise ValueError('%s: T must be even, got %d' % (who, T))
    beta = float(beta)
    if not 0.0 <= beta < math.inf:
        raise ValueError('%s: beta must be a finite number >= 0, got %r' % (who, beta))
    half = T // 2
    t = np.arange(T, dtype=np.float64)[None, :] - (half - 1) - np.arange(1, P, dtype=np.float64)[:, None] / P
    u = 1.0 - (t / half) ** 2
    h = np.where(u >= 0.0, np.sinc(t) * np.i0(beta * np.sqrt(np.maximum(u, 0.0))) / np.i0(beta), 0.0)
    return (h / h.sum(axis=1, keepdims=True)).astype(np.float32)


def limit_window(W):
    """The smoothing weights of taco_wave_limit: a (2 W + 1) float32 array, 0.5 - 0.5 cos(2 pi (k + 1) / (2 W + 2)) (a Hann window
    without its zero ends) divided by its sum in fp64 and rounded once.  W in 0..512 is the look-ahead in samples."""
    W = int_arg('limit_window', 'W', W, 0, LIMIT_MAX_W)
    k = np.arange(2 * W + 1, dtype=np.float64)
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1.0) / (2 * W + 2))
    return (h / h.sum()).astype(np.float32)


def wave_limit_workspace_floats(B, L, W) -> int:
    return _size('taco_wave_limit_workspace_bytes', B, L, W) // 4


_default_taps = {}   # device -> the default interpolator, uploaded once


def _limit_table(who, name, x, shape, dev, empty_ok=False):
    """a float32 table on `dev`: the caller's device tensor (checked, never read), or a host array / tensor (checked and uploaded)"""
    if not torch.is_tensor(x):
        try:
            x = torch.from_numpy(np.ascontiguousarray(x))
        except TypeError:
            raise ValueError('%s: %s must be a float32 array or tensor, got a %s' % (who, name, type(x).__name__)) from None
    free = tensor_arg(who, name, x, torch.float32, shape, None if x.device.type == 'cpu' else dev, empty_ok=empty_ok)
    return x, free


def wave_limit(wave, samples=None, gain=None, ceiling=1.0, taps=None, window=None, want_out=None, want_pcm=None, out=None, pcm=None,
               peaks=None, counts=None, work=None):
    """True-peak meter and look-ahead limiter (include/taco_hip.h taco_wave_limit): wave (B, L) fp32 -> (out (B, L) fp32 or None,
    pcm (B, L) int16 or None, peaks (B, 4) fp32 = (tp_in, G, g_min, peak_out), counts (B, 2) int32 = (n_b, samples limited)).  Per row
    over its first n_b samples: the envelope e = the largest of |x| and of the P - 1 interpolated phases of `taps`; the gain
    r = ceiling / (G e) where G e passes the ceiling, else 1; its minimum over W samples either side, smoothed by `window`, and never
    above r: out = (G x) s, pcm its PCM16, zeros behind n_b.  tp_in is the true peak of the input, peak_out the sample peak of out.
    samples (B) int32 on the device, or None: every row has L samples.  gain (B) fp32 on the device, or None: G = 1.  ceiling in
    (0, 1], on the true peak.  taps: a (P - 1, T) float32 table (a device tensor, or a host array that is uploaded); None: the
    default true_peak_taps(), uploaded once per device; a (0, T) table is P = 1, a sample-peak limiter.  window: (2 W + 1) float32
    likewise, limit_window(W); None: MEASURE ONLY -- the dBTP meter: peaks = (tp_in, 1, 1, max |x|), out and pcm stay None and gain
    and ceiling are not looked at.  want_out / want_pcm default to whether there is a window.  out / pcm / peaks / counts / work: the
    caller's own buffers (work: wave_limit_workspace_floats(B, L, W) floats); default: fresh ones.  An out / pcm buffer implies
    want_out / want_pcm; out may be wave itself."""
    who = 'wave_limit'
    B, L = tensor_arg(who, 'wave', wave, torch.float32, ('B', 'L'))
    dev = wave.device
    if B > 65535:
        raise ValueError('%s: at most 65535 rows per call, got %d' % (who, B))
    tensor_arg(who, 'samples', samples, torch.int32, (B,), dev, optional=True)
    tensor_arg(who, 'gain', gain, torch.float32, (B,), dev, optional=True)
    if taps is None:
        P, T = LIMIT_P, LIMIT_T
    else:
        taps, (P, T) = _limit_table(who, 'taps', taps, ('P - 1', 'T'), dev, empty_ok=True)
        P += 1
        if not 1 <= P <= 8 or not 2 <= T <= 32 or T % 2:
            raise ValueError('%s: taps must hold P - 1 in [0, 7] phases of an even number T in [2, 32] of taps, got %s'
                             % (who, tuple(taps.shape)))
    want_out = (window is not None if want_out is None else bool(want_out)) or out is not None
    want_pcm = (window is not None if want_pcm is None else bool(want_pcm)) or pcm is not None
    if window is None:
        if want_out or want_pcm:
            raise ValueError('%s: out and pcm need a window (window=None measures only)' % who)
        W, ceiling = 0, 1.0
    else:
        window, (n_w,) = _limit_table(who, 'window', window, ('2 W + 1',), dev)
        if n_w % 2 == 0 or n_w // 2 > LIMIT_MAX_W:
            raise ValueError('%s: window must hold 2 W + 1 weights with W in [0, %d], got %d' % (who, LIMIT_MAX_W, n_w))
        W = n_w // 2
        ceiling = float(ceiling)
        if not 0.0 < ceiling <= 1.0 or C.c_float(ceiling).value <= 0.0:   # (NaN fails)
            raise ValueError('%s: ceiling must be in (0, 1], got %r' % (who, ceiling))
        if not (want_out or want_pcm):
            raise ValueError('%s: a window needs at least one of out and pcm' % who)
    out = _own_or_given(out, (B, L), torch.float32, dev, who + ': out') if want_out else None
    if out is not None and out.data_ptr() != wave.data_ptr():
        no_overlap(who, 'wave', wave, 'out', out)
    pcm = _own_or_given(pcm, (B, L), torch.int16, dev, who + ': pcm') if want_pcm else None
    peaks = _own_or_given(peaks, (B, 4), torch.float32, dev, who + ': peaks')
    counts = _own_or_given(counts, (B, 2), torch.int32, dev, who + ': counts')
    if work is not None:
        tensor_arg(who, 'work', work, torch.float32, ('floats',), dev)
    on_gpu(who, 'wave', dev)
    if taps is None:
        if dev not in _default_taps:
            _default_taps[dev] = torch.from_numpy(true_peak_taps()).to(dev)
        taps = _default_taps[dev]
    elif taps.device != dev:
        taps = taps.to(dev)
    if window is not None and window.device != dev:
        window = window.to(dev)
    work = _own_or_given(work, (wave_limit_workspace_floats(B, L, W),), torch.float32, dev, who + ': work')
    _check(_lib.taco_wave_limit(ptr(wave), ptr(samples), ptr(gain), ceiling, ptr(taps) if P > 1 else None, P, T, ptr(window), W,
                                ptr(out), ptr(pcm), ptr(peaks), ptr(counts), ptr(work), B, L, stream_ptr()), 'taco_wave_limit')
    return out, pcm, peaks, counts


def audio_features_workspace_bytes(B, L) -> int:
    return _size('taco_audio_features_workspace_bytes', B, L)


def audio_features(wave, wave_len, mel_basis, r, max_len=108000, out_dtype=torch.float16, out=None, work=None):
    """audio.process_audio for a batch (include/taco_hip.h taco_audio_features).  wave (B, L) fp32 on the device, wave_len (B) host
    ints, mel_basis (80, 1025) fp32 on the device -> (mel (B, Td, 80 r), stft (B, Td, 1025 r), kept (B) int32, bounds (B, 2) int32),
    device tensors; out_dtype float16 or float32.  out: the caller's own (mel, stft, kept, bounds) buffers, work: the caller's
    own workspace (uint8, audio_features_workspace_bytes(B, L) bytes); default: fresh ones."""
    if not torch.is_tensor(wave):
        raise ValueError('audio_features: wave must be a tensor of shape (B, L), got %s' % type(wave))
    B, L = wave.shape
    if len(wave_len) != B:
        raise ValueError('audio_features: %d lengths for %d waves' % (len(wave_len), B))
    lens = (C.c_int32 * B)(*[int(x) for x in wave_len])
    assert out_dtype in (torch.float16, torch.float32)
    nbytes = audio_features_workspace_bytes(B, L)
    F = 1 + int(max_len) // 300
    Td = (F // (4 * r)) * 4 if r > 0 else 0
    dev = wave.device
    o = out if out is not None else (None, None, None, None)
    work = _own_or_given(work, (nbytes,), torch.uint8, dev, 'audio_features: work')
    mel = _own_or_given(o[0], (B, max(Td, 0), 80 * max(r, 0)), out_dtype, dev, 'audio_features: mel')
    stft = _own_or_given(o[1], (B, max(Td, 0), 1025 * max(r, 0)), out_dtype, dev, 'audio_features: stft')
    kept = _own_or_given(o[2], (B,), torch.int32, dev, 'audio_features: kept')
    bounds = _own_or_given(o[3], (B, 2), torch.int32, dev, 'audio_features: bounds')
    _check(_lib.taco_audio_features(ptr(wave), lens, ptr(mel_basis), ptr(mel), ptr(stft), ptr(bounds), ptr(kept), ptr(work), B, L,
                                    int(max_len), int(r), int(out_dtype == torch.float16), stream_ptr()), 'taco_audio_features')
    return mel, stft, kept, bounds


WAVE_RESAMPLE_TILE = 1024   # outputs per workgroup of taco_wave_resample (include/taco_hip.h TACO_WAVE_RESAMPLE_TILE)


def wave_resample(pcm, rows, taps, width, channels, P, Q, n_left, n_right, L=None, out=None):
    """PCM decode and kaiser_best resampling (include/taco_hip.h taco_wave_resample): pcm (B, row_bytes) uint8, the interleaved
    little-endian frames of B files of one format (width 1..4 bytes per sample, channels 1..8); rows (B, 2) int32 on the device,
    (n_orig_b, n_calc_b); taps (Q, n_left + n_right) float32, the polyphase table of audio.resample_filter (None allowed when
    P == Q: decode-only) -> wave (B, L) float32: row b holds its n_calc_b resampled samples (P == Q: its decoded frames), zeros behind.
    L: the width of a fresh result; out: the caller's own (B, L) buffer instead."""
    who = 'wave_resample'
    B, row_bytes = tensor_arg(who, 'pcm', pcm, torch.uint8, ('B', 'row_bytes'))
    dev = pcm.device
    if B > 65535:
        raise ValueError('%s: at most 65535 rows per call, got %d' % (who, B))
    width, channels = int_arg(who, 'width', width, 1, 4), int_arg(who, 'channels', channels, 1, 8)
    P, Q = int_arg(who, 'P', P, 1), int_arg(who, 'Q', Q, 1)
    n_left, n_right = int_arg(who, 'n_left', n_left, 1), int_arg(who, 'n_right', n_right, 1)
    if row_bytes % (width * channels):
        raise ValueError('%s: row_bytes %d is not a multiple of width * channels = %d' % (who, row_bytes, width * channels))
    tensor_arg(who, 'rows', rows, torch.int32, (B, 2), dev)
    if taps is None and P != Q:
        raise ValueError('%s: taps may be None only when P == Q (decode-only), got P = %d, Q = %d' % (who, P, Q))
    tensor_arg(who, 'taps', taps, torch.float32, (Q, n_left + n_right), dev, optional=True)
    if P != Q:   # the library's own rule: the frames one tile reads must fit 64 KiB of LDS
        span = (WAVE_RESAMPLE_TILE - 1) * P // Q + 1 + n_left + n_right
        if (-(-span // P) * P + n_left + n_right if Q == 1 else span) * 4 > 64 * 1024:
            raise ValueError('%s: P / Q = %d / %d with %d taps reads %d frames per tile, more than 64 KiB of LDS hold'
                             % (who, P, Q, n_left + n_right, span))
    if (L is None) == (out is None):
        raise ValueError('%s: give exactly one of L and out' % who)
    L = int_arg(who, 'L', L, 1) if out is None else tensor_arg(who, 'out', out, torch.float32, (B, 'L'), dev)[0]
    on_gpu(who, 'pcm', dev)
    wave = _own_or_given(out, (B, L), torch.float32, dev, who + ': out')
    _check(_lib.taco_wave_resample(ptr(pcm), row_bytes, width, channels, ptr(rows), ptr(taps), P, Q, n_left, n_right, ptr(wave), B, L,
                                   stream_ptr()), 'taco_wave_resample')
    return wave


def fill_bernoulli(out, p_one, seed):
    _check(_lib.taco_fill_bernoulli(ptr(out), out.numel(), float(p_one), int(seed) & 0xFFFFFFFFFFFFFFFF, stream_ptr()),
           'taco_fill_bernoulli')


STATS_CHUNK = 8192          # TACO_STATS_CHUNK: the positions of a segment that one wave of taco_tensor_stats reads
STATS_MAX_SEGMENTS = 4096   # TACO_STATS_MAX_SEGMENTS
STATS_COUNTS = ('size', 'finite', 'nan', 'pinf', 'ninf', 'zeros')   # columns of counts (include/taco_hip.h taco_tensor_stats)
STATS_MOMENTS = ('sum', 'sumsq', 'min', 'max', 'absmax')            # columns of moments
STATS_E_LO, STATS_E_HI, STATS_SUB_BITS = -24, 15, 2                 # the default buckets: 2^-24 .. 2^16, four per octave, NB = 321


class TensorStats(collections.namedtuple('TensorStats', 'counts moments hist')):
    """What tensor_stats returns: counts (n, 6) int64, moments (n, 5) fp64, hist (n, NB) int64, device tensors."""
    __slots__ = ()


class TensorStatsPlan(object):
    """The work list of tensor_stats for one list of segments of one buffer: `dev` the blob on the device (int64 words), `header` its
    first 32 bytes on the host (the only thing a call reads there), n segments, n_items work items, base_floats the floats the
    buffer must hold, `segments` the (offset, size) pairs."""

    def __init__(self, dev, header, n, n_items, base_floats, segments):
        self.dev, self.header, self.n, self.n_items, self.base_floats, self.segments = dev, header, n, n_items, base_floats, segments


def _stats_buckets(who, e_lo, e_hi, sub_bits):
    e_lo = int_arg(who, 'e_lo', e_lo, -126, 127)
    e_hi = int_arg(who, 'e_hi', e_hi, e_lo, 127)
    sub_bits = int_arg(who, 'sub_bits', sub_bits, 0, 3)
    return e_lo, e_hi, sub_bits, 2 * ((e_hi - e_lo + 1) << sub_bits) + 1


def tensor_stats_plan(segments, base_floats, device='cuda') -> TensorStatsPlan:
    """The plan of tensor_stats (include/taco_hip.h taco_tensor_stats_plan) for `segments`, a host sequence of (offset, size) pairs in
    floats of a buffer of base_floats floats: built on the host, uploaded once.  1 .. STATS_MAX_SEGMENTS segments, each inside
    [0, base_floats); they may overlap and may be empty."""
    who = 'tensor_stats_plan'
    try:
        segs = [(int_arg(who, 'a segment offset', o, 0), int_arg(who, 'a segment size', s, 0)) for o, s in segments]
    except (TypeError, ValueError) as e:
        if isinstance(e, ValueError) and str(e).startswith(who):
            raise
        raise ValueError('%s: segments must be a sequence of (offset, size) pairs, got %r' % (who, segments)) from None
    n = int_arg(who, 'the number of segments', len(segs), 1, STATS_MAX_SEGMENTS)
    base_floats = int_arg(who, 'base_floats', base_floats, 0)
    for i, (o, s) in enumerate(segs):
        if o + s > base_floats:
            raise ValueError('%s: segment %d = (offset %d, size %d) is outside [0, %d)' % (who, i, o, s, base_floats))
    dev = torch.device(device)   # (tensor_stats is the judge of the device: the plan goes where its buffer is)
    flat =(C.c_int64 * (2 * n))(*[v for seg in segs for v in seg])
    nbytes = _lib.taco_tensor_stats_plan_bytes(flat, n)
    if nbytes < 0:
        raise TacoError('taco_tensor_stats_plan_bytes: bad arguments (rc=%d)' % nbytes)
    blob = np.zeros(nbytes // 8, dtype=np.int64)   # (every part of the blob is whole 8-byte words)
    n_items = C.c_int32(0)
    _check(_lib.taco_tensor_stats_plan(flat, n, base_floats, C.c_void_p(blob.ctypes.data), nbytes, C.byref(n_items)), 'taco_tensor_stats_plan')
    return TensorStatsPlan(torch.from_numpy(blob).to(dev), blob[:4].copy(), n, int(n_items.value), base_floats, segs)


def tensor_stats_workspace_bytes(n, n_items, NB) -> int:
    return _size('taco_tensor_stats_workspace_bytes', n, n_items, NB)


def tensor_stats_edges(e_lo=STATS_E_LO, e_hi=STATS_E_HI, sub_bits=STATS_SUB_BITS):
    """The NB + 1 edges of tensor_stats' buckets as float64, ascending: bin b holds the finite x with edges[b] <= x < edges[b + 1] for
    the positive bins, edges[b] < x <= edges[b + 1] for the negative ones, and the centre bin is the open interval between its two
    edges -2^e_lo and 2^e_lo; the outermost edges are -inf and +inf (the top buckets are open-ended).  A positive bucket m opens at
    the fp32 value with the bits (lo + m - 1) << (23 - sub_bits): 2^e (1 + f / 2^sub_bits)."""
    e_lo, e_hi, s, NB = _stats_buckets('tensor_stats_edges', e_lo, e_hi, sub_bits)
    Nm = (NB - 1) // 2
    pos = np.array([math.ldexp(1.0 + (m % (1 << s)) / float(1 << s), e_lo + (m >> s)) for m in range(Nm)], dtype=np.float64)
    return np.concatenate([[-np.inf], -pos[::-1], pos, [np.inf]])


def tensor_stats(base, plan, e_lo=STATS_E_LO, e_hi=STATS_E_HI, sub_bits=STATS_SUB_BITS, counts=None, moments=None, hist=None, work=None):
    """Statistics and histograms of the plan's segments of `base` in one call (include/taco_hip.h taco_tensor_stats): base a
    flat (1-d) fp32 tensor of at least plan.base_floats floats, 16-byte aligned, plan a TensorStatsPlan (tensor_stats_plan) ->
    TensorStats(counts (n, 6) int64 in the order STATS_COUNTS, moments (n, 5) fp64 in the order STATS_MOMENTS over the finite
    elements, hist (n, NB) int64 in sign-symmetric log buckets from 2^e_lo to 2^(e_hi + 1), 2^sub_bits per octave,
    NB = 2 ((e_hi - e_lo + 1) << sub_bits) + 1; tensor_stats_edges gives their edges).  Two launches on the current stream, no copy,
    no synchronisation.  counts / moments / hist / work: the caller's own buffers (work: uint8,
    tensor_stats_workspace_bytes(plan.n, plan.n_items, NB) bytes); default: fresh ones."""
    who = 'tensor_stats'
    if not isinstance(plan, TensorStatsPlan):
        raise ValueError('%s: plan must be a TensorStatsPlan (tensor_stats_plan), got a %s' % (who, type(plan).__name__))
    floats, = tensor_arg(who, 'base', base, torch.float32, ('floats',))
    if floats < plan.base_floats:
        raise ValueError('%s: base holds %d floats, the plan was built for %d' % (who, floats, plan.base_floats))
    dev = base.device
    e_lo, e_hi, sub_bits, NB = _stats_buckets(who, e_lo, e_hi, sub_bits)
    if plan.dev.device != dev:
        raise ValueError('%s: the plan is on %s, base on %s' % (who, plan.dev.device, dev))
    counts = _own_or_given(counts, (plan.n, len(STATS_COUNTS)), torch.int64, dev, who + ': counts')
    moments = _own_or_given(moments, (plan.n, len(STATS_MOMENTS)), torch.float64, dev, who + ': moments')
    hist = _own_or_given(hist, (plan.n, NB), torch.int64, dev, who + ': hist')
    if work is not None:
        tensor_arg(who, 'work', work, torch.uint8, ('bytes',), dev)
    on_gpu(who, 'base', dev)
    if base.data_ptr() % 16:
        raise ValueError('%s: base must be 16-byte aligned' % who)
    need = tensor_stats_workspace_bytes(plan.n, plan.n_items, NB)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    elif work.numel() < need or work.data_ptr() % 8:
        raise ValueError('%s: work must hold %d bytes and be 8-byte aligned, got %d' % (who, need, work.numel()))
    _check(_lib.taco_tensor_stats(ptr(base), ptr(plan.dev), C.c_void_p(plan.header.ctypes.data), plan.n, plan.n_items, e_lo, e_hi,
                                  sub_bits, ptr(counts), ptr(moments), ptr(hist), ptr(work), stream_ptr()), 'taco_tensor_stats')
    return TensorStats(counts, moments, hist)


EMA_WARMUP = (1.0, 10.0)   # tf.train.ExponentialMovingAverage(num_updates=k): decay_k = min(decay, (1 + k) / (10 + k))


def ema_decay(decay, k) -> float:
    """The decay of weight-averaging update number k (k = 0 the first: the EMA updates attempted before this one), TF's num_updates
    warm-up min(decay, (1 + k) / (10 + k)) in Python floats: 0.1, 0.18, ... until the configured decay takes over."""
    decay = float_arg('ema_decay', 'decay', decay, 0.0, 1.0)
    k = int_arg('ema_decay', 'k', k, 0)
    return min(decay, (EMA_WARMUP[0] + k) / (EMA_WARMUP[1] + k))


def ema_weight(decay, k):
    """w of param_ema for update number k: 1 - ema_decay(decay, k) in Python floats, rounded once to float32"""
    return np.float32(1.0 - ema_decay(decay, k))


def param_ema_workspace_bytes(n) -> int:
    return _size('taco_param_ema_workspace_bytes', n)


def param_ema(ema, params, w, err_words=None, stats=None, workspace=None):
    """One weight-averaging update in place (include/taco_hip.h taco_param_ema): ema[i] += w (params[i] - ema[i]) as three rounded
    fp32 operations, ema and params flat fp32 tensors of one length on the GPU that do not overlap (any float alignment), w in [0, 1]
    (ema_weight).  err_words: the two int32 error words of clip_adam_step, or None (unguarded): with either set, ema stays as it is.
    stats: None, or 3 float64 on the device that receive (sum of the squared differences before the update, sum of params^2, 1), or
    (-1, -1, 0) for a skipped update; workspace then is param_ema_workspace_bytes(n) bytes of uint8 (default: a fresh one).  One
    launch, two with stats, on the current stream; no copy and no synchronisation.  Returns stats."""
    who = 'param_ema'
    n, = tensor_arg(who, 'ema', ema, torch.float32, ('floats',))
    dev = ema.device
    tensor_arg(who, 'params', params, torch.float32, (n,), dev)
    w = float_arg(who, 'w', w, 0.0, 1.0)
    tensor_arg(who, 'err_words', err_words, torch.int32, (2,), dev, optional=True)
    tensor_arg(who, 'stats', stats, torch.float64, (3,), dev, optional=True)
    tensor_arg(who, 'workspace', workspace, torch.uint8, ('bytes',), dev, optional=True)
    no_overlap(who, 'params', params, 'ema', ema)
    on_gpu(who, 'ema', dev)
    if stats is not None:
        need = param_ema_workspace_bytes(n)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        elif workspace.numel() < need or workspace.data_ptr() % 8:
            raise ValueError('%s: workspace must hold %d bytes and be 8-byte aligned, got %d' % (who, need, workspace.numel()))
    _check(_lib.taco_param_ema(ptr(ema), ptr(params), n, w, ptr(err_words), ptr(stats), ptr(workspace) if stats is not None else None,
                               stream_ptr()), 'taco_param_ema')
    return stats


def last_cluster(which: int) -> int:
    return _lib.taco_debug_last_cluster(int(which))


def profile_enable(mask):
    """mask: bit c = category c (0 decoder fwd, 1 decoder bwd, 2 GEMM family, 3 bi-GRU); True = both decoder kernels."""
    _check(_lib.taco_profile_enable(3 if mask is True else int(mask)), 'taco_profile_enable')


def profile_labels(which: int):
    """What each launch currently in ring `which` was (kernel family + shape); call before profile_read."""
    cap = 1 << 19
    buf = C.create_string_buffer(cap)
    n = _lib.taco_debug_profile_labels(int(which), buf, cap)
    if n < 0:
        raise TacoError('taco_debug_profile_labels: ' + last_error())
    return buf.value.decode().split('\n')[:n]


def profile_read(which: int, with_flops=False):
    """Elapsed milliseconds (and algorithmic FLOPs) of every recorded launch of category `which` since the last read."""
    cap = 4096
    buf = (C.c_float * cap)()
    fl = (C.c_double * cap)()
    n = _lib.taco_profile_read2(which, buf, fl, cap)
    if n < 0:
        raise TacoError('taco_profile_read: ' + last_error())
    n = min(n, cap)
    ms = [buf[i] for i in range(n)]
    return (ms, [fl[i] for i in range(n)]) if with_flops else ms
