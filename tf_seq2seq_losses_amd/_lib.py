"""ctypes binding of libctc_amd.so (C ABI declared in include/ctc_amd.h).

The product path has NO fallback: if the shared library is missing or does not load, importing the
symbols raises, loudly.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (hipcc,
--offload-arch=gfx950); the .so lives in-tree next to this file.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTC_AMD_LIB", os.path.join(_HERE, "libctc_amd.so"))  # override: kernel experiments only

ABI_VERSION = 6
CLASSIC, SIMPLIFIED = 0, 1
WRT_LOGITS, WRT_LOGPROBS = 0, 1
WS_LOSS_GRAD, WS_ALPHA_BETA, WS_HESSIAN, WS_HVP, WS_LOSS_GRAD_LOGITS = 0, 1, 2, 3, 4
OK, EINVAL, EWORKSPACE, EHIP, ELABEL = 0, -1, -2, -3, -4
F32, BF16, F16 = 0, 1, 2
WILDCARD = -2  # CTC_AMD_WILDCARD: the label value of a wildcard position (ctc_amd_wildcard_best_path)
OPTIONAL_CLASSIC_MAX_U = 512  # CTC_AMD_OPTIONAL_CLASSIC_MAX_U: the classic optional-wildcard alignment's U
OPTIONAL_WILDCARD = -3  # CTC_AMD_OPTIONAL_WILDCARD: a wildcard position that may be empty (ctc_amd_optional_wildcard_loss_grad)
LONG_MAX_U, LONG_FRAMES_MULTIPLE, LONG_FRAMES_DEFAULT = 65536, 4, 128  # CTC_AMD_LONG_*: ctc_amd_long_best_path
PREFIX_MAX, PREFIX_GROUP = 64, 8  # CTC_AMD_PREFIX_MAX, CTC_AMD_PREFIX_GROUP
NBEST_MAX, NBEST_GROUP = 64, 8  # CTC_AMD_NBEST_MAX, CTC_AMD_NBEST_GROUP: hypotheses per utterance, and per workgroup (one logits read)

_c_int, _c_int64, _c_void_p, _c_size_t = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t

_COMMON = [_c_int, _c_int,            # kind, wrt
           _c_void_p, _c_void_p, _c_int,  # logits, labels, label_stride
           _c_void_p, _c_void_p, _c_int,  # label_length, logit_length, blank_index
           _c_int, _c_int, _c_int, _c_int]  # B, T, V, U
# the same for the producer-format entry points: element type and strides behind the logits pointer
_COMMON_EX = [_c_int, _c_int,                               # kind, wrt
              _c_void_p, _c_int, _c_int64, _c_int64,        # logits, dtype, stride_b, stride_t
              _c_void_p, _c_int, _c_void_p, _c_void_p, _c_int,  # labels, label_stride, label_length, logit_length, blank_index
              _c_int, _c_int, _c_int, _c_int]               # B, T, V, U
_OUT_EX = [_c_void_p, _c_void_p, _c_int, _c_int64, _c_int64]  # loss, grad, dtype, stride_b, stride_t

# the two step calls of the prefix scorer: no labels, N behind the shape, then the row statistics
_PREFIX_EX = [_c_int, _c_int, _c_void_p, _c_int, _c_int64, _c_int64,  # kind, wrt, logits, dtype, stride_b, stride_t
              _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int,      # logit_length, blank_index, B, T, V, N
              _c_void_p, _c_size_t]                                   # rows, bytes

# every symbol include/ctc_amd.h declares, with its argument types
SIGNATURES = {
    "ctc_amd_abi_version": (_c_int, []),
    "ctc_amd_last_error": (ctypes.c_char_p, []),
    "ctc_amd_pipeline_name": (ctypes.c_char_p, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "ctc_amd_debug_override": (_c_int, [ctypes.c_char_p, ctypes.c_char_p]),
    "ctc_amd_debug_flags_offset": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),
    "ctc_amd_debug_hvp_flags_offset": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),
    "ctc_amd_reduce_loss": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p]),
    "ctc_amd_probe_copy": (_c_int, [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_probe_spin": (_c_int, [_c_int, _c_int, ctypes.c_float, _c_void_p]),
    "ctc_amd_check_labels": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p]),
    "ctc_amd_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),
    "ctc_amd_loss_grad": (_c_int, _COMMON + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_loss_grad_ex": (_c_int, _COMMON_EX + _OUT_EX + [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),  # d_loss, ws, bytes, stream
    "ctc_amd_loss_grad_packed": (_c_int, [_c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_int64,          # kind, wrt, logits, dtype, row_offsets, row_stride
                                          *_COMMON_EX[6:],                                                 # labels .. U
                                          _c_void_p, _c_void_p, _c_int, _c_int64,                          # loss, grad, dtype, grad row stride
                                          _c_void_p, _c_void_p, _c_size_t, _c_void_p]),                    # d_loss, ws, bytes, stream
    "ctc_amd_loss_grad_sum": (_c_int, _COMMON_EX + _OUT_EX + [_c_void_p, _c_void_p, _c_void_p,             # d_loss, sum2, zero_next
                                                             _c_void_p, _c_size_t, _c_void_p]),          # ws, bytes, stream
    "ctc_amd_loss_forward": (_c_int, _COMMON_EX + [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),           # loss, ws, bytes, stream
    "ctc_amd_grad_resume": (_c_int, _COMMON_EX + _OUT_EX + [_c_void_p, _c_void_p, _c_size_t, _c_void_p]),  # d_loss, ws, bytes, stream
    "ctc_amd_alpha_beta": (_c_int, _COMMON + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_hessian": (_c_int, _COMMON + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_log_posterior": (_c_int, _COMMON + [_c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_hvp": (_c_int, _COMMON + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_best_path_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),
    "ctc_amd_best_path": (_c_int, _COMMON_EX + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),  # score, tokens, label_index, ws, bytes, stream
    "ctc_amd_greedy_decode_workspace_bytes": (_c_int, [_c_int, _c_int, ctypes.POINTER(_c_size_t)]),
    "ctc_amd_greedy_decode": (_c_int, [_c_int, _c_int, _c_void_p, _c_int, _c_int64, _c_int64,      # kind, wrt, logits, dtype, stride_b, stride_t
                                       _c_void_p, _c_int, _c_int, _c_int, _c_int,                  # logit_length, blank_index, B, T, V
                                       _c_void_p, _c_void_p, _c_void_p, _c_void_p,                 # score, tokens, decoded, decoded_length
                                       _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),    # frames, label_score, ws, bytes, stream
    "ctc_amd_beam_search_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # B, T, V, W, K
    "ctc_amd_beam_search": (_c_int, [_c_int, _c_int, _c_void_p, _c_int, _c_int64, _c_int64,        # kind, wrt, logits, dtype, stride_b, stride_t
                                     _c_void_p, _c_int, _c_int, _c_int, _c_int,                    # logit_length, blank_index, B, T, V
                                     _c_int, _c_int, _c_int,                                       # beam_width, top_k, nbest
                                     _c_void_p, _c_void_p, _c_void_p,                              # score, decoded, decoded_length
                                     _c_void_p, _c_size_t, _c_void_p]),                            # ws, bytes, stream
    "ctc_amd_nbest_loss_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, N
    "ctc_amd_nbest_loss": (_c_int, _COMMON_EX + [_c_int, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),  # N, loss, ws, bytes, stream
    "ctc_amd_nbest_loss_grad_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, N
    "ctc_amd_nbest_loss_grad": (_c_int, _COMMON_EX + [_c_int, _c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),  # N, weight, loss .. grad strides, ws, bytes, stream
    "ctc_amd_nbest_best_path_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, N
    "ctc_amd_nbest_best_path": (_c_int, _COMMON_EX + [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,  # N, score, tokens, label_index, first_frame, last_frame
                                                      _c_void_p, _c_size_t, _c_void_p]),                           # ws, bytes, stream
    "ctc_amd_wildcard_best_path_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U
    "ctc_amd_wildcard_best_path": (_c_int, _COMMON_EX + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,  # score, tokens, label_index, first_frame, last_frame, label_score
                                                         _c_void_p, _c_size_t, _c_void_p]),                              # ws, bytes, stream
    "ctc_amd_long_best_path_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile
    "ctc_amd_long_best_path": (_c_int, _COMMON_EX + [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,  # frames_per_tile, score, tokens, label_index, first_frame, last_frame
                                                     _c_void_p, _c_size_t, _c_void_p]),                          # ws, bytes, stream
    "ctc_amd_long_wildcard_best_path_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile
    "ctc_amd_long_wildcard_best_path": (_c_int, _COMMON_EX + [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,  # frames_per_tile, score, tokens, label_index, first_frame, last_frame, label_score
                                                              _c_void_p, _c_size_t, _c_void_p]),                                     # ws, bytes, stream
    "ctc_amd_wildcard_loss_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, want_grad
    "ctc_amd_wildcard_loss_grad": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +    # .. blank_index, wildcard_log_weight, B, T, V, U
                                   [_c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),     # d_loss, loss .. grad strides, ws, bytes, stream
    "ctc_amd_long_wildcard_loss_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile, want_grad
    "ctc_amd_long_wildcard_loss_grad": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +  # .. blank_index, wildcard_log_weight, B, T, V, U
                                        [_c_int, _c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),  # frames_per_tile, d_loss, loss .. grad strides, ws, bytes, stream
    "ctc_amd_long_wildcard_loss_ckpt_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile, want_grad
    "ctc_amd_long_wildcard_loss_grad_ckpt": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +  # .. blank_index, wildcard_log_weight, B, T, V, U
                                             [_c_int, _c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),  # frames_per_tile, d_loss, loss .. grad strides, ws, bytes, stream
    "ctc_amd_label_posterior_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U
    "ctc_amd_label_posterior": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +       # .. blank_index, wildcard_log_weight, B, T, V, U
                                [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,             # loss, label_posterior, blank_posterior, duration, expected_frame
                                 _c_void_p, _c_size_t, _c_void_p]),                                 # ws, bytes, stream
    "ctc_amd_long_label_posterior_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile
    "ctc_amd_long_label_posterior": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +  # .. blank_index, wildcard_log_weight, B, T, V, U
                                     [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,  # frames_per_tile, loss, label_posterior, blank_posterior, duration, expected_frame
                                      _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),       # peak_posterior, peak_frame, ws, bytes, stream
    # the four windowed entry points: their counterparts with (frame_window, window_stride) behind blank_index
    "ctc_amd_windowed_loss_grad": (_c_int, _COMMON_EX[:11] + [_c_void_p, _c_int, ctypes.c_float] + _COMMON_EX[11:] +
                                   [_c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_windowed_label_posterior": (_c_int, _COMMON_EX[:11] + [_c_void_p, _c_int, ctypes.c_float] + _COMMON_EX[11:] +
                                         [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_windowed_best_path": (_c_int, _COMMON_EX[:11] + [_c_void_p, _c_int] + _COMMON_EX[11:] +
                                   [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_long_windowed_best_path": (_c_int, _COMMON_EX[:11] + [_c_void_p, _c_int] + _COMMON_EX[11:] +
                                        [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                         _c_void_p, _c_size_t, _c_void_p]),
    # optional wildcards: the counterparts' arguments
    "ctc_amd_optional_wildcard_best_path_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U
    "ctc_amd_optional_wildcard_best_path": (_c_int, _COMMON_EX + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                                                  _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_optional_wildcard_loss_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, want_grad
    "ctc_amd_optional_wildcard_loss_grad": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +
                                            [_c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_optional_wildcard_label_posterior_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U
    "ctc_amd_optional_wildcard_label_posterior": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +
                                                  [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    # ... and the three long-form ones of the summed lattice, in the same manner
    "ctc_amd_long_windowed_loss_grad": (_c_int, _COMMON_EX[:11] + [_c_void_p, _c_int, ctypes.c_float] + _COMMON_EX[11:] +
                                        [_c_int, _c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_long_windowed_loss_grad_ckpt": (_c_int, _COMMON_EX[:11] + [_c_void_p, _c_int, ctypes.c_float] + _COMMON_EX[11:] +
                                             [_c_int, _c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_long_windowed_label_posterior": (_c_int, _COMMON_EX[:11] + [_c_void_p, _c_int, ctypes.c_float] + _COMMON_EX[11:] +
                                              [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                               _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    # ... and the three long-form ones with optional wildcards: the arguments of ctc_amd_long_wildcard_loss_grad / _grad_ckpt and
    # ctc_amd_long_label_posterior
    "ctc_amd_long_optional_wildcard_loss_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile, want_grad
    "ctc_amd_long_optional_wildcard_loss_grad": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +
                                                 [_c_int, _c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_long_optional_wildcard_loss_ckpt_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile, want_grad
    "ctc_amd_long_optional_wildcard_loss_grad_ckpt": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +
                                                      [_c_int, _c_void_p] + _OUT_EX + [_c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_long_optional_wildcard_label_posterior_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # kind, B, T, V, U, frames_per_tile
    "ctc_amd_long_optional_wildcard_label_posterior": (_c_int, _COMMON_EX[:11] + [ctypes.c_float] + _COMMON_EX[11:] +
                                                       [_c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                                        _c_void_p, _c_void_p, _c_void_p, _c_size_t, _c_void_p]),
    "ctc_amd_edit_distance_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # B, N, R
    "ctc_amd_edit_distance": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p,  # hyp, hyp_stride, hyp_length, ref, ref_stride, ref_length
                                       _c_int, _c_int, _c_int, _c_void_p,                           # B, N, R, distance
                                       _c_void_p, _c_size_t, _c_void_p]),                           # ws, bytes, stream
    "ctc_amd_edit_counts_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t)]),  # B, N, R, hyp_stride, rows_per_tile
    "ctc_amd_edit_counts": (_c_int, [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p,  # hyp, hyp_stride, hyp_length, ref, ref_stride, ref_length
                                     _c_int, _c_int, _c_int, _c_int, _c_void_p,                   # B, N, R, rows_per_tile, counts
                                     _c_void_p, _c_size_t, _c_void_p]),                           # ws, bytes, stream
    "ctc_amd_prefix_workspace_bytes": (_c_int, [_c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_size_t), ctypes.POINTER(_c_size_t)]),  # B, T, V, N, rows, state
    "ctc_amd_prefix_rows": (_c_int, [_c_void_p, _c_int, _c_int64, _c_int64, _c_void_p, _c_int, _c_int, _c_int,  # logits, dtype, stride_b, stride_t, logit_length, B, T, V
                                     _c_void_p, _c_size_t, _c_void_p]),                                      # rows, bytes, stream
    "ctc_amd_prefix_extend": (_c_int, _PREFIX_EX + [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,  # state_in, last_in, length_in, parent, token
                                                    _c_void_p, _c_size_t, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),  # state_out, bytes, last_out, length_out, full_score, stream
    "ctc_amd_prefix_score": (_c_int, _PREFIX_EX + [_c_void_p, _c_size_t, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),  # state, bytes, last, length, score, stream
}

_lib = None
override_generation = 0  # bumped by debug_override: cached pipeline names / workspace sizes of ops.py are keyed on it


class CtcAmdError(RuntimeError):
    """An entry point of libctc_amd.so returned a negative code."""


def load() -> ctypes.CDLL:
    """Loads libctc_amd.so (once) and binds every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` at the repo root (needs hipcc). "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.ctc_amd_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"libctc_amd.so ABI version {got} != expected {ABI_VERSION}; rebuild it")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc == OK:
        return
    msg = load().ctc_amd_last_error().decode("utf-8", "replace")
    if rc in (EINVAL, ELABEL):
        raise ValueError(f"{what}: {msg}")
    raise CtcAmdError(f"{what} failed with code {rc}: {msg}")


def pipeline_name(kind: int, wrt: int, B: int, T: int, V: int, U: int, want_grad: bool = True) -> str:
    return load().ctc_amd_pipeline_name(kind, wrt, B, T, V, U, int(want_grad)).decode()


def debug_override(key: str, value: str = "") -> None:
    """Diagnostic (parity tests, benchmarks): force a lower kernel tier ("pipeline": "v1" | "fused5") or the
    general Hessian kernel ("hessian": "slab"); the empty string restores the default.  Process-wide."""
    global override_generation
    check(load().ctc_amd_debug_override(key.encode(), value.encode()), "ctc_amd_debug_override")
    override_generation += 1


def flags_offset(kind: int, B: int, T: int, V: int, U: int) -> int:
    """Diagnostic: where the linear-domain kernel's per-utterance flag words sit in a logits call's workspace."""
    out = _c_size_t(0)
    check(load().ctc_amd_debug_flags_offset(kind, B, T, V, U, ctypes.byref(out)), "ctc_amd_debug_flags_offset")
    return int(out.value)


def hvp_flags_offset(kind: int, B: int, T: int, V: int, U: int) -> int:
    """Diagnostic: where the fused Hessian-vector kernel's per-utterance flag words sit in a WS_HVP workspace."""
    out = _c_size_t(0)
    check(load().ctc_amd_debug_hvp_flags_offset(kind, B, T, V, U, ctypes.byref(out)), "ctc_amd_debug_hvp_flags_offset")
    return int(out.value)


def workspace_bytes(what: int, kind: int, B: int, T: int, V: int, U: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_workspace_bytes(what, kind, B, T, V, U, ctypes.byref(out)), "ctc_amd_workspace_bytes")
    return int(out.value)


def best_path_workspace_bytes(kind: int, B: int, T: int, V: int, U: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_best_path_workspace_bytes(kind, B, T, V, U, ctypes.byref(out)), "ctc_amd_best_path_workspace_bytes")
    return int(out.value)


def greedy_decode_workspace_bytes(B: int, T: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_greedy_decode_workspace_bytes(B, T, ctypes.byref(out)), "ctc_amd_greedy_decode_workspace_bytes")
    return int(out.value)


def beam_search_workspace_bytes(B: int, T: int, V: int, beam_width: int, top_k: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_beam_search_workspace_bytes(B, T, V, beam_width, top_k, ctypes.byref(out)), "ctc_amd_beam_search_workspace_bytes")
    return int(out.value)


def nbest_loss_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, N: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_nbest_loss_workspace_bytes(kind, B, T, V, U, N, ctypes.byref(out)), "ctc_amd_nbest_loss_workspace_bytes")
    return int(out.value)


def nbest_loss_grad_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, N: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_nbest_loss_grad_workspace_bytes(kind, B, T, V, U, N, ctypes.byref(out)), "ctc_amd_nbest_loss_grad_workspace_bytes")
    return int(out.value)


def nbest_best_path_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, N: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_nbest_best_path_workspace_bytes(kind, B, T, V, U, N, ctypes.byref(out)), "ctc_amd_nbest_best_path_workspace_bytes")
    return int(out.value)


def wildcard_best_path_workspace_bytes(kind: int, B: int, T: int, V: int, U: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_wildcard_best_path_workspace_bytes(kind, B, T, V, U, ctypes.byref(out)), "ctc_amd_wildcard_best_path_workspace_bytes")
    return int(out.value)


def long_best_path_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_best_path_workspace_bytes(kind, B, T, V, U, frames_per_tile, ctypes.byref(out)),
          "ctc_amd_long_best_path_workspace_bytes")
    return int(out.value)


def long_wildcard_best_path_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_wildcard_best_path_workspace_bytes(kind, B, T, V, U, frames_per_tile, ctypes.byref(out)),
          "ctc_amd_long_wildcard_best_path_workspace_bytes")
    return int(out.value)


def wildcard_loss_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, want_grad: bool = True) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_wildcard_loss_workspace_bytes(kind, B, T, V, U, int(want_grad), ctypes.byref(out)), "ctc_amd_wildcard_loss_workspace_bytes")
    return int(out.value)


def long_wildcard_loss_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0, want_grad: bool = True) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_wildcard_loss_workspace_bytes(kind, B, T, V, U, frames_per_tile, int(want_grad), ctypes.byref(out)),
          "ctc_amd_long_wildcard_loss_workspace_bytes")
    return int(out.value)


def long_wildcard_loss_ckpt_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0, want_grad: bool = True) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_wildcard_loss_ckpt_workspace_bytes(kind, B, T, V, U, frames_per_tile, int(want_grad), ctypes.byref(out)),
          "ctc_amd_long_wildcard_loss_ckpt_workspace_bytes")
    return int(out.value)


def label_posterior_workspace_bytes(kind: int, B: int, T: int, V: int, U: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_label_posterior_workspace_bytes(kind, B, T, V, U, ctypes.byref(out)), "ctc_amd_label_posterior_workspace_bytes")
    return int(out.value)


def long_optional_wildcard_loss_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0, want_grad: bool = True) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_optional_wildcard_loss_workspace_bytes(kind, B, T, V, U, frames_per_tile, int(want_grad), ctypes.byref(out)),
          "ctc_amd_long_optional_wildcard_loss_workspace_bytes")
    return int(out.value)


def long_optional_wildcard_loss_ckpt_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0, want_grad: bool = True) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_optional_wildcard_loss_ckpt_workspace_bytes(kind, B, T, V, U, frames_per_tile, int(want_grad), ctypes.byref(out)),
          "ctc_amd_long_optional_wildcard_loss_ckpt_workspace_bytes")
    return int(out.value)


def long_optional_wildcard_label_posterior_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_optional_wildcard_label_posterior_workspace_bytes(kind, B, T, V, U, frames_per_tile, ctypes.byref(out)),
          "ctc_amd_long_optional_wildcard_label_posterior_workspace_bytes")
    return int(out.value)


def long_label_posterior_workspace_bytes(kind: int, B: int, T: int, V: int, U: int, frames_per_tile: int = 0) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_long_label_posterior_workspace_bytes(kind, B, T, V, U, frames_per_tile, ctypes.byref(out)),
          "ctc_amd_long_label_posterior_workspace_bytes")
    return int(out.value)


def edit_distance_workspace_bytes(B: int, N: int, R: int) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_edit_distance_workspace_bytes(B, N, R, ctypes.byref(out)), "ctc_amd_edit_distance_workspace_bytes")
    return int(out.value)


def edit_counts_workspace_bytes(B: int, N: int, R: int, hyp_stride: int, rows_per_tile: int = 0) -> int:
    out = _c_size_t(0)
    check(load().ctc_amd_edit_counts_workspace_bytes(B, N, R, hyp_stride, rows_per_tile, ctypes.byref(out)), "ctc_amd_edit_counts_workspace_bytes")
    return int(out.value)


def prefix_workspace_bytes(B: int, T: int, V: int, N: int):
    """(rows_bytes, state_bytes) of the prefix scorer."""
    rows, state = _c_size_t(0), _c_size_t(0)
    check(load().ctc_amd_prefix_workspace_bytes(B, T, V, N, ctypes.byref(rows), ctypes.byref(state)), "ctc_amd_prefix_workspace_bytes")
    return int(rows.value), int(state.value)
