"""Python host mirror of omr_core's public API over libomr_gpu.so (include/omr_gpu.h).

Names follow the reference (omr_core/src/lib.rs:21-31): KeyGen, SecretKeyPack, DetectionKey,
Detector (detect / detect_with_time_info / encode_pertinent_indices /
encode_pertinent_payloads), RetrievalParams, Payload helpers. Every compute call goes through
the HIP C ABI; there is no CPU fallback: if libomr_gpu.so is missing this module raises.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import weakref
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OMR_GPU_LIB", os.path.join(HERE, "libomr_gpu.so"))

N0, CLUE_COUNT, N1, NI, N2 = 512, 7, 1024, 670, 2048
Q1, Q2, P = 134215681, 1125899906826241, 257
KS_DIGITS, TRACE_STEPS, TRACE_DIGITS, PAYLOAD_LENGTH = 27, 11, 25, 612
BSK1_SHAPE = (N0, 8, 2, N1)
KSK_SHAPE = (N1, KS_DIGITS, NI + 1)
BSK2_SHAPE = (NI, 12, 2, N2)
TK_SHAPE = (TRACE_STEPS, TRACE_DIGITS, 2, N2)
# seeded detection key (include/omr_gpu.h): the bodies, and per component (omr_key_component order)
# the rows, the masks per row and the element type
BSK1_B_SHAPE = (N0, 8, N1)
KSK_B_SHAPE = (N1, KS_DIGITS)
BSK2_B_SHAPE = (NI, 12, N2)
TK_B_SHAPE = (TRACE_STEPS, TRACE_DIGITS, N2)
KEY_BSK1, KEY_KSK, KEY_BSK2, KEY_TRACE = 0, 1, 2, 3
KEY_COMPONENTS = ((N0 * 8, N1, np.uint32), (N1 * KS_DIGITS, NI, np.uint32), (NI * 12, N2, np.uint64),
                  (TRACE_STEPS * TRACE_DIGITS, N2, np.uint64))

_u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_u16p = np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
_i8p = np.ctypeslib.ndpointer(dtype=np.int8, flags="C_CONTIGUOUS")


class OmrError(RuntimeError):
    pass


class _RetrievalParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "index_slots_per_bucket", "slots_per_bucket", "slots_per_segment", "segment_per_cipher",
        "max_encode_indices_cipher_count", "combination_count", "cmb_count_per_cipher", "cmb_cipher_count")]


class _KeyView(C.Structure):
    _fields_ = [("bsk1", C.c_void_p), ("ksk", C.c_void_p), ("bsk2", C.c_void_p), ("trace_key", C.c_void_p)]


class _SeededKeyView(C.Structure):
    _fields_ = [("bsk1_b", C.c_void_p), ("ksk_b", C.c_void_p), ("bsk2_b", C.c_void_p), ("trace_key_b", C.c_void_p),
                ("mask_seed", C.c_uint64)]


class _Timing(C.Structure):
    """omr_detect_timing: DetectTimeInfo (detector.rs:51-57) in milliseconds of device time."""
    _fields_ = [("total_ms", C.c_float), ("first_level_ms", C.c_float), ("second_level_ms", C.c_float),
                ("trace_ms", C.c_float), ("key_switch_ms", C.c_float), ("messages", C.c_size_t),
                ("trace_separate", C.c_int)]


class _DigestInfo(C.Structure):
    """omr_digest_info."""
    _fields_ = [("index_ct", C.c_uint32), ("payload_ct", C.c_uint32), ("combination_count", C.c_uint32),
                ("cmb_count_per_cipher", C.c_uint32), ("all_payloads_count", C.c_size_t), ("messages", C.c_size_t),
                ("pv_capacity_messages", C.c_size_t)]


class _PayloadLayout(C.Structure):
    """omr_payload_layout."""
    _fields_ = [(n, C.c_uint32) for n in ("payload_len", "combination_count", "cmb_count_per_cipher", "stripes",
                                          "payload_ct")]


class _AuditSummary(C.Structure):
    """omr_audit_summary."""
    _fields_ = [(n, C.c_uint64) for n in ("ciphertexts", "zero", "one_hot", "other", "max_abs_residual")] + \
               [("residual_bits", C.c_uint64 * 50)]


class _KeyAuditSummary(C.Structure):
    """omr_key_audit_summary."""
    _fields_ = [(n, C.c_uint64) for n in ("rows", "noncanonical", "max_abs_noise", "rows_over", "first_row_over")] + \
               [("noise_bits", C.c_uint64 * 50)]


# omr_launch_kind, in index order (omr_ctx_launch_record)
LAUNCH_KINDS = ("br2f", "br2f_guard", "br2l", "br2x", "br2y", "br2y_helpers", "br2_from", "guard_fallback",
                "trace_fft", "trace_fft_guard", "trace_x", "trace_kernel")

# omr_ct_audit as a structured dtype (16 bytes)
AUDIT_RECORD = np.dtype([("max_abs_residual", np.uint64), ("nonzero", np.uint32), ("first", np.uint32)])
AUDIT_RESIDUAL_BINS = 50


EXPORTS = {
    "omr_last_error": (C.c_char_p, []),
    "omr_version": (C.c_char_p, []),
    "omr_detect_kernels": (C.c_char_p, []),
    "omr_keygen_secret": (C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
    "omr_secret_destroy": (None, [C.c_void_p]),
    "omr_secret_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_keygen_detection_key": (C.c_int, [C.c_void_p, C.c_uint64, _u32p, _u32p, _u64p, _u64p, C.c_int]),
    "omr_gen_clues": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, _u16p, _u16p, C.c_int]),
    "omr_gen_clues_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "omr_keygen_detection_key_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    # sender (include/omr_gpu.h "Sender"); omr_clue_key pointers are void *
    "omr_secret_clue_key": (C.c_int, [C.c_void_p, C.c_void_p]),
    "omr_clue_key_validate": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "omr_clue_key_noise_support": (C.c_int, [C.POINTER(C.c_uint64)]),
    "omr_clue_key_audit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "omr_sender_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "omr_sender_destroy": (None, [C.c_void_p]),
    "omr_sender_gen_clues": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_int]),
    "omr_sender_gen_clues_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "omr_clue_open": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_int]),
    "omr_clue_open_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "omr_keygen_seeded_key": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p, _u32p, _u64p, _u64p, C.c_int]),
    "omr_keygen_seeded_key_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "omr_expand_detection_key": (C.c_int, [C.POINTER(_SeededKeyView), _u32p, _u32p, _u64p, _u64p, C.c_int]),
    "omr_expand_detection_key_device": (C.c_int, [C.POINTER(_SeededKeyView), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "omr_key_masks": (C.c_int, [C.c_uint64, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]),
    "omr_key_masks_device": (C.c_int, [C.c_uint64, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "omr_ctx_create_seeded": (C.c_int, [C.POINTER(_SeededKeyView), C.c_int, C.POINTER(C.c_void_p)]),
    "omr_get_retrieval_params": (C.c_int, [C.c_size_t, C.c_size_t, C.POINTER(_RetrievalParams)]),
    "omr_payload_weights": (C.c_int, [_u8p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, _u16p]),
    "omr_indexed_weights_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_int]),
    "omr_indexed_weights_table": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                            C.c_int]),
    "omr_indexed_weights_table_device": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                   C.c_void_p, C.c_void_p]),
    "omr_encode_payloads_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "omr_encode_payloads_indexed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                     C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                     C.c_uint32, C.c_void_p, C.c_void_p]),
    "omr_digest_begin_indexed": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_void_p)]),
    "omr_digest_device_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "omr_retrieve_payloads_indexed": (C.c_int, [C.c_void_p, _u64p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_void_p,
                                                np.ctypeslib.ndpointer(dtype=np.uintp, flags="C_CONTIGUOUS"),
                                                C.c_size_t, _u16p]),
    "omr_ctx_create": (C.c_int, [C.POINTER(_KeyView), C.c_int, C.POINTER(C.c_void_p)]),
    "omr_ctx_destroy": (None, [C.c_void_p]),
    "omr_ctx_set_batch": (C.c_int, [C.c_void_p, C.c_size_t]),
    "omr_ctx_set_latency_threshold": (C.c_int, [C.c_void_p, C.c_size_t]),
    "omr_ctx_set_exact_level1": (C.c_int, [C.c_void_p, C.c_int]),
    "omr_ctx_set_encode_chunks": (C.c_int, [C.c_void_p, C.c_size_t]),
    "omr_detect_batch": (C.c_int, [C.c_void_p, _u16p, _u16p, C.c_size_t, _u64p]),
    "omr_detect": (C.c_int, [C.c_void_p, _u16p, _u16p, _u64p]),
    "omr_ctx_set_coalescing": (C.c_int, [C.c_void_p, C.c_size_t, C.c_long]),
    "omr_ctx_coalescing_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "omr_detect_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "omr_ctx_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "omr_last_timing": (C.c_int, [C.c_void_p, C.POINTER(_Timing)]),
    "omr_detect_with_time_info": (C.c_int, [C.c_void_p, _u16p, _u16p, C.c_size_t, _u64p, C.POINTER(_Timing)]),
    "omr_ctx_check": (C.c_int, [C.c_void_p, C.c_void_p]),
    "omr_ctx_set_rounding_guard": (C.c_int, [C.c_void_p, C.c_int]),
    "omr_ctx_rounding_margin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "omr_ctx_exactness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_ctx_launch_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "omr_fft_twiddles_dd": (C.c_int, [C.c_int, np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")]),
    "omr_ctx_key_spectrum": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t,
                                       np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")]),
    "omr_encode_indices": (C.c_int, [C.c_void_p, _u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint64,
                                     C.c_uint32, _u64p]),
    "omr_encode_indices_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                            C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "omr_encode_payloads": (C.c_int, [C.c_void_p, _u64p, _u16p, C.c_size_t, C.c_size_t, C.c_size_t, _u16p,
                                      C.c_uint32, C.c_uint32, _u64p]),
    "omr_encode_payloads_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                             C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.c_void_p]),
    "omr_bitmap_ct_count": (C.c_int, [C.c_size_t, C.POINTER(C.c_uint32)]),
    "omr_encode_bitmap": (C.c_int, [C.c_void_p, _u64p, C.c_size_t, C.c_size_t, C.c_size_t, _u64p]),
    "omr_encode_bitmap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                           C.c_void_p]),
    "omr_bitmap_indices": (C.c_int, [_u16p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "omr_retrieve_bitmap": (C.c_int, [C.c_void_p, _u64p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "omr_digest_enable_bitmap": (C.c_int, [C.c_void_p]),
    "omr_digest_read_bitmap": (C.c_int, [C.c_void_p, C.c_void_p]),
    "omr_digest_merge_bitmap": (C.c_int, [C.c_void_p, C.c_void_p]),
    "omr_digest_begin": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_void_p)]),
    "omr_digest_update": (C.c_int, [C.c_void_p, _u16p, _u16p, _u16p, C.c_size_t, C.c_size_t]),
    "omr_digest_update_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]),
    "omr_digest_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_digest_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_digest_get_info": (C.c_int, [C.c_void_p, C.POINTER(_DigestInfo)]),
    "omr_digest_destroy": (None, [C.c_void_p]),
    "omr_first_level": (C.c_int, [C.c_void_p, _u16p, _u16p, C.c_size_t, _u32p]),
    "omr_sum_key_switch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "omr_blind_rotate_level1": (C.c_int, [C.c_void_p, _u16p, _u16p, C.c_size_t, _u64p]),
    "omr_fft1_mul": (C.c_int, [C.c_void_p, _u32p, _u32p, C.c_size_t, _u64p]),
    "omr_decrypt_decode": (C.c_int, [C.c_void_p, _u64p, C.c_size_t, _u32p]),
    "omr_retrieve_indices": (C.c_int, [C.c_void_p, _u64p, C.c_uint32, C.c_size_t, C.c_size_t,
                                       np.ctypeslib.ndpointer(dtype=np.uintp, flags="C_CONTIGUOUS"),
                                       C.c_size_t, C.POINTER(C.c_size_t)]),
    "omr_retrieve_payloads": (C.c_int, [C.c_void_p, _u64p, C.c_uint32, C.c_size_t, C.c_uint32, _u16p,
                                        np.ctypeslib.ndpointer(dtype=np.uintp, flags="C_CONTIGUOUS"),
                                        C.c_size_t, _u16p]),
    "omr_auditor_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "omr_auditor_destroy": (None, [C.c_void_p]),
    "omr_auditor_set_grid": (C.c_int, [C.c_void_p, C.c_uint]),
    "omr_auditor_set_staging": (C.c_int, [C.c_void_p, C.c_size_t]),
    "omr_audit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "omr_audit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_audit_cpu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "omr_compact_ct_bytes": (C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
    "omr_compact_residual_bound": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "omr_compact_cts_cpu": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int]),
    "omr_compact_expand_cpu": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int]),
    "omr_compact_cts_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "omr_compact_cts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "omr_ctx_set_compact_grid": (C.c_int, [C.c_void_p, C.c_uint]),
    "omr_ctx_set_compact_staging": (C.c_int, [C.c_void_p, C.c_size_t]),
    "omr_compact_expand_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "omr_audit_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "omr_digest_read_compact": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_key_noise_support": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "omr_audit_key_rows_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_audit_key_rows_cpu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_int]),
    "omr_audit_key": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_audit_key_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_audit_key_cpu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "omr_key_count_noncanonical_device": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "omr_key_validate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "omr_key_validate_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "omr_key_validate_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "omr_key_validate_seeded_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "omr_second_level": (C.c_int, [C.c_void_p, _u32p, C.c_size_t, _u64p]),
    "omr_blind_rotate_level2": (C.c_int, [C.c_void_p, _u32p, C.c_size_t, _u64p]),
    "omr_blind_rotate_level1_from": (C.c_int, [C.c_void_p, _u16p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "omr_blind_rotate_level2_from": (C.c_int, [C.c_void_p, _u32p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "omr_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "omr_ntt": (C.c_int, [C.c_int, C.c_int, _u64p, C.c_size_t, C.c_int]),
    "omr_solve_mod257_cpu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                       C.POINTER(C.c_size_t), C.c_int]),
    "omr_solve_geometry": (C.c_int, [C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "omr_solve_mod257_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "omr_solve_profile": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float * 4)]),
    "omr_auditor_retrieve_indices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_size_t,
                                               C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "omr_auditor_retrieve_payloads": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_size_t, C.c_uint32,
                                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "omr_auditor_retrieve_payloads_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_size_t,
                                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "omr_auditor_decode_digest_indexed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int,
                                                    C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p]),
    # reference payload weights by seek (include/omr_gpu.h); the omr_weight_seek pointers are void *
    "omr_weight_seek_build_cpu": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "omr_weight_seek_build_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "omr_weight_seek_build_zone_cpu": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]),
    "omr_weight_seek_build_zone_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "omr_payload_weights_at": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]),
    "omr_encode_payloads_seek": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_void_p]),
    "omr_encode_payloads_seek_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                  C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "omr_digest_begin_seek": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_void_p)]),
    "omr_retrieve_payloads_seek": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "omr_auditor_retrieve_payloads_seek": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_size_t,
                                                     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                     C.c_void_p]),
    # payload length as a board parameter (include/omr_gpu.h)
    "omr_get_payload_layout": (C.c_int, [C.c_size_t, C.c_size_t, C.POINTER(_PayloadLayout)]),
    "omr_encode_payloads_indexed_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                  C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.c_uint32, C.c_void_p]),
    "omr_encode_payloads_indexed_len_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                         C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                         C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "omr_digest_begin_indexed_len": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.POINTER(C.c_void_p)]),
    "omr_digest_get_payload_layout": (C.c_int, [C.c_void_p, C.POINTER(_PayloadLayout)]),
    "omr_retrieve_payloads_indexed_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t,
                                                    C.POINTER(_PayloadLayout), C.c_void_p, C.c_void_p, C.c_size_t,
                                                    C.c_void_p]),
    "omr_auditor_retrieve_payloads_indexed_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_size_t,
                                                            C.POINTER(_PayloadLayout), C.c_void_p, C.c_void_p,
                                                            C.c_size_t, C.c_void_p]),
}

_lib = None


def lib():
    """Load libomr_gpu.so (fails loudly: there is no CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OmrError(f"{LIB_PATH} not found: build it with `make -C tfhe-omr_amd` "
                           "(or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(st: int, what: str) -> None:
    if st != 0:
        raise OmrError(f"{what} failed ({st}): {lib().omr_last_error().decode()}")


@dataclass
class RetrievalParams:
    """RetrievalParams::new(257, 2048, all, pertinent, 130, 25, 2) (retrieval_params.rs:50-106)."""
    all_payloads_count: int
    pertinent_count: int
    index_slots_per_bucket: int = 0
    slots_per_bucket: int = 0
    slots_per_segment: int = 0
    segment_per_cipher: int = 0
    max_encode_indices_cipher_count: int = 0
    combination_count: int = 0
    cmb_count_per_cipher: int = 0
    cmb_cipher_count: int = 0

    def __post_init__(self):
        rp = _RetrievalParams()
        _check(lib().omr_get_retrieval_params(self.all_payloads_count, self.pertinent_count, C.byref(rp)),
               "omr_get_retrieval_params")
        for n, _ in _RetrievalParams._fields_:
            setattr(self, n, getattr(rp, n))


PAYLOAD_LEN_MAX = 16384     # OMR_PAYLOAD_LEN_MAX
PAYLOAD_PER_CT_MAX = 16     # OMR_PAYLOAD_PER_CT_MAX


@dataclass
class PayloadLayout:
    """omr_payload_layout: the payload digest of a board whose payloads are payload_len words long
    (include/omr_gpu.h, "Payload length as a board parameter"). PayloadLayout.of() asks the library; the
    fields may be set by hand for a digest encoded with fewer combinations per ciphertext."""
    payload_len: int
    combination_count: int
    cmb_count_per_cipher: int
    stripes: int
    payload_ct: int

    @classmethod
    def of(cls, pertinent_count: int, payload_len: int) -> "PayloadLayout":
        t = _PayloadLayout()
        _check(lib().omr_get_payload_layout(pertinent_count, payload_len, C.byref(t)), "omr_get_payload_layout")
        return cls(**{n: getattr(t, n) for n, _ in _PayloadLayout._fields_})

    def _struct(self) -> "_PayloadLayout":
        return _PayloadLayout(self.payload_len, self.combination_count, self.cmb_count_per_cipher, self.stripes,
                              self.payload_ct)


def _layout_ref(layout):
    """A PayloadLayout as the C struct by reference; None passes NULL."""
    return None if layout is None else C.byref(layout._struct())


def payload_weights(seed: bytes, rp: RetrievalParams) -> np.ndarray:
    """Seeded weights in the reference order (detector.rs:376-387): [n_ct*per_ct][all] u16."""
    n = rp.cmb_cipher_count * rp.cmb_count_per_cipher * rp.all_payloads_count
    out = np.zeros(n, dtype=np.uint16)
    _check(lib().omr_payload_weights(np.frombuffer(bytes(seed), dtype=np.uint8).copy(), rp.all_payloads_count,
                                     rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher, out),
           "omr_payload_weights")
    return out


def _seed_ptr(seed):
    """The address of a 32-byte weight seed (and the array that keeps it alive); None passes NULL."""
    if seed is None:
        return None, None
    a = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
    if a.size != 32:
        raise OmrError("weight seed must be 32 bytes")
    return a.ctypes.data, a


def indexed_weights_at(seed: bytes, combination_count: int, indices, first_combo: int = 0, n_combos: int = None,
                       nthreads: int = 0) -> np.ndarray:
    """omr_indexed_weights_at: u16 [n_combos][len(indices)], w(first_combo + r, indices[k]) of the indexed
    payload weights (include/omr_gpu.h); rows at or beyond combination_count are zero. n_combos defaults to
    the combinations from first_combo up to combination_count (the recipient's matrix for first_combo = 0)."""
    idx = np.ascontiguousarray(indices, dtype=np.uintp).reshape(-1)
    n = max(combination_count - first_combo, 0) if n_combos is None else n_combos
    out = np.empty((n, idx.size), np.uint16)
    ptr, _keep = _seed_ptr(seed)
    _check(lib().omr_indexed_weights_at(ptr, combination_count, first_combo, n, idx.ctypes.data, idx.size,
                                        out.ctypes.data, nthreads), "omr_indexed_weights_at")
    return out


def indexed_weights_table(seed: bytes, rp: RetrievalParams, nthreads: int = 0) -> np.ndarray:
    """omr_indexed_weights_table: the indexed weights in payload_weights' layout, [n_ct*per_ct][all] u16 flat."""
    out = np.empty(rp.cmb_cipher_count * rp.cmb_count_per_cipher * rp.all_payloads_count, dtype=np.uint16)
    ptr, _keep = _seed_ptr(seed)
    _check(lib().omr_indexed_weights_table(ptr, rp.all_payloads_count, rp.combination_count, rp.cmb_cipher_count,
                                           rp.cmb_count_per_cipher, out.ctypes.data, nthreads),
           "omr_indexed_weights_table")
    return out


def indexed_weights_table_device(seed: bytes, all_payloads_count: int, combination_count: int, n_ct: int, per_ct: int,
                                 d_out: int, stream: int = 0) -> None:
    """omr_indexed_weights_table_device: the same table into a device buffer u16 [n_ct*per_ct][all]."""
    ptr, _keep = _seed_ptr(seed)
    _check(lib().omr_indexed_weights_table_device(ptr, all_payloads_count, combination_count, n_ct, per_ct,
                                                  d_out or None, stream or None), "omr_indexed_weights_table_device")


WEIGHT_SEEK_MAX = 32
WEIGHT_ZONE = 0xFFFFFFFE


class _WeightSeek(C.Structure):
    _fields_ = [("draws", C.c_uint64), ("n", C.c_uint32), ("zone", C.c_uint32), ("at", C.c_uint64 * WEIGHT_SEEK_MAX)]


class WeightSeek:
    """omr_weight_seek (include/omr_gpu.h, "Reference payload weights by seek"): the rejections of
    omr_payload_weights' stream that matter for its first `draws` accepted draws; `at[k] = r_k - k`."""

    def __init__(self, draws: int = 0, at=(), zone: int = WEIGHT_ZONE, n: int = None):
        self._t = _WeightSeek(draws, len(at) if n is None else n, zone)
        for k, v in enumerate(at):
            self._t.at[k] = v

    draws = property(lambda self: self._t.draws)
    n = property(lambda self: self._t.n)
    zone = property(lambda self: self._t.zone)
    at = property(lambda self: [int(self._t.at[k]) for k in range(min(self._t.n, WEIGHT_SEEK_MAX))])

    @property
    def ptr(self):
        return C.addressof(self._t)

    def __eq__(self, other):
        return (self.draws, self.n, self.zone, self.at) == (other.draws, other.n, other.zone, other.at)

    def __repr__(self):
        return f"WeightSeek(draws={self.draws}, at={self.at}, zone={self.zone:#x})"

    @classmethod
    def build(cls, seed: bytes, draws: int, zone: int = None, device: bool = False, nthreads: int = 0,
              stream: int = 0) -> "WeightSeek":
        """omr_weight_seek_build_cpu / _device (zone given: the _zone_ stage entries): scan the stream of
        `seed` for the rejections of its first `draws` draws, on the host or on the current HIP device."""
        s = cls()
        ptr, _keep = _seed_ptr(seed)
        L = lib()
        if device:
            st = (L.omr_weight_seek_build_device(ptr, draws, s.ptr, stream or None) if zone is None else
                  L.omr_weight_seek_build_zone_device(ptr, draws, zone, s.ptr, stream or None))
        else:
            st = (L.omr_weight_seek_build_cpu(ptr, draws, nthreads, s.ptr) if zone is None else
                  L.omr_weight_seek_build_zone_cpu(ptr, draws, zone, nthreads, s.ptr))
        _check(st, "omr_weight_seek_build_device" if device else "omr_weight_seek_build_cpu")
        return s

    @classmethod
    def for_board(cls, seed: bytes, rp: "RetrievalParams", device: bool = False) -> "WeightSeek":
        """The seek of a board: combination_count * all draws."""
        return cls.build(seed, rp.combination_count * rp.all_payloads_count, device=device)


def _seek_ptr(seek):
    return None if seek is None else seek.ptr


def payload_weights_at(seed: bytes, all_payloads_count: int, combination_count: int, seek: "WeightSeek", indices,
                       first_combo: int = 0, n_combos: int = None, nthreads: int = 0) -> np.ndarray:
    """omr_payload_weights_at: u16 [n_combos][len(indices)], omr_payload_weights' weight (first_combo + r,
    indices[k]) found through the seek, no table; rows at or beyond combination_count are zero."""
    idx = np.ascontiguousarray(indices, dtype=np.uintp).reshape(-1)
    n = max(combination_count - first_combo, 0) if n_combos is None else n_combos
    out = np.empty((n, idx.size), np.uint16)
    ptr, _keep = _seed_ptr(seed)
    _check(lib().omr_payload_weights_at(ptr, all_payloads_count, combination_count, _seek_ptr(seek), first_combo, n,
                                        idx.ctypes.data, idx.size, out.ctypes.data, nthreads), "omr_payload_weights_at")
    return out


@dataclass
class DetectionKey:
    """Coefficient-domain evaluation keys (key_gen/detection.rs:9-16) in the ABI layout."""
    bsk1: np.ndarray
    ksk: np.ndarray
    bsk2: np.ndarray
    trace_key: np.ndarray

    def size(self) -> int:
        return sum(a.nbytes for a in (self.bsk1, self.ksk, self.bsk2, self.trace_key))


@dataclass
class SeededKey:
    """The seeded form of a detection key (include/omr_gpu.h): the bodies and the public mask seed,
    153,120,776 bytes instead of 380,227,584."""
    bsk1_b: np.ndarray
    ksk_b: np.ndarray
    bsk2_b: np.ndarray
    trace_key_b: np.ndarray
    mask_seed: int

    def size(self) -> int:
        return sum(a.nbytes for a in (self.bsk1_b, self.ksk_b, self.bsk2_b, self.trace_key_b)) + 8

    def _view(self) -> "_SeededKeyView":
        for a, shape, dt in ((self.bsk1_b, BSK1_B_SHAPE, np.uint32), (self.ksk_b, KSK_B_SHAPE, np.uint32),
                             (self.bsk2_b, BSK2_B_SHAPE, np.uint64), (self.trace_key_b, TK_B_SHAPE, np.uint64)):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise OmrError(f"seeded key body has shape {a.shape} {a.dtype}, expected {shape} {dt}")
        return _SeededKeyView(self.bsk1_b.ctypes.data, self.ksk_b.ctypes.data, self.bsk2_b.ctypes.data,
                              self.trace_key_b.ctypes.data, self.mask_seed)

    def expand(self, nthreads: int = 0) -> DetectionKey:
        """omr_expand_detection_key: the full key on the host."""
        dk = DetectionKey(np.empty(BSK1_SHAPE, np.uint32), np.empty(KSK_SHAPE, np.uint32),
                          np.empty(BSK2_SHAPE, np.uint64), np.empty(TK_SHAPE, np.uint64))
        view = self._view()
        _check(lib().omr_expand_detection_key(C.byref(view), dk.bsk1.reshape(-1), dk.ksk.reshape(-1),
                                              dk.bsk2.reshape(-1), dk.trace_key.reshape(-1), nthreads),
               "omr_expand_detection_key")
        return dk


def expand_detection_key_device(d_bodies, mask_seed: int, d_bsk1: int, d_ksk: int, d_bsk2: int, d_trace_key: int,
                                stream: int = 0) -> None:
    """omr_expand_detection_key_device: d_bodies is a SeededKey (host bodies) or four raw pointers
    (bsk1_b, ksk_b, bsk2_b, trace_key_b; host or device memory); the full key goes to device buffers."""
    view = d_bodies._view() if isinstance(d_bodies, SeededKey) else _SeededKeyView(*d_bodies, mask_seed)
    _check(lib().omr_expand_detection_key_device(C.byref(view), d_bsk1, d_ksk, d_bsk2, d_trace_key, stream or None),
           "omr_expand_detection_key_device")


def key_masks(mask_seed: int, component: int, first_row: int, rows: int) -> np.ndarray:
    """omr_key_masks: the masks [rows][N] of a row range of one component of a seeded key (host)."""
    _, n, dt = KEY_COMPONENTS[component] if 0 <= component < 4 else (0, 1, np.uint32)
    out = np.empty((max(rows, 0), n), dt)
    _check(lib().omr_key_masks(mask_seed, component, first_row, rows, out.ctypes.data), "omr_key_masks")
    return out


def key_masks_device(mask_seed: int, component: int, first_row: int, rows: int, d_out: int, stream: int = 0) -> None:
    """omr_key_masks_device: the same rows into a device buffer; returns when the stream is done."""
    _check(lib().omr_key_masks_device(mask_seed, component, first_row, rows, d_out or None, stream or None),
           "omr_key_masks_device")


class SecretKeyPack:
    """KeyGen::generate_secret_key / SecretKeyPack (key_gen/secret.rs:46-209), seeded."""

    def __init__(self, seed: int):
        h = C.c_void_p()
        _check(lib().omr_keygen_secret(seed, C.byref(h)), "omr_keygen_secret")
        self._h = h
        self.seed = seed
        # bound now: at interpreter shutdown the module's globals (lib) may already be None
        self._destroy = lib().omr_secret_destroy

    def __del__(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def export(self):
        s0 = np.zeros(N0, np.uint8)
        s1 = np.zeros(N1, np.int8)
        sint = np.zeros(NI, np.uint8)
        s2 = np.zeros(N2, np.int8)
        _check(lib().omr_secret_export(self._h, s0.ctypes.data, s1.ctypes.data, sint.ctypes.data,
                                       s2.ctypes.data), "omr_secret_export")
        return dict(s0=s0, s1=s1, s_int=sint, s2=s2)

    def generate_detection_key(self, seed: int, nthreads: int = 0) -> DetectionKey:
        bsk1 = np.empty(BSK1_SHAPE, np.uint32)
        ksk = np.empty(KSK_SHAPE, np.uint32)
        bsk2 = np.empty(BSK2_SHAPE, np.uint64)
        tk = np.empty(TK_SHAPE, np.uint64)
        _check(lib().omr_keygen_detection_key(self._h, seed, bsk1.reshape(-1), ksk.reshape(-1), bsk2.reshape(-1),
                                              tk.reshape(-1), nthreads), "omr_keygen_detection_key")
        return DetectionKey(bsk1, ksk, bsk2, tk)

    def generate_seeded_key(self, seed: int, mask_seed: int, nthreads: int = 0) -> SeededKey:
        """omr_keygen_seeded_key: the bodies of the key whose masks come from the public mask_seed."""
        sk = SeededKey(np.empty(BSK1_B_SHAPE, np.uint32), np.empty(KSK_B_SHAPE, np.uint32),
                       np.empty(BSK2_B_SHAPE, np.uint64), np.empty(TK_B_SHAPE, np.uint64), mask_seed)
        _check(lib().omr_keygen_seeded_key(self._h, seed, mask_seed, sk.bsk1_b.reshape(-1), sk.ksk_b.reshape(-1),
                                           sk.bsk2_b.reshape(-1), sk.trace_key_b.reshape(-1), nthreads),
               "omr_keygen_seeded_key")
        return sk

    def gen_clues(self, seed: int, first: int, count: int, nthreads: int = 0):
        """Sender::gen_clues for global message indices [first, first+count)."""
        a = np.empty((count, N0), np.uint16)
        b = np.empty((count, CLUE_COUNT), np.uint16)
        _check(lib().omr_gen_clues(self._h, seed, first, count, a.reshape(-1), b.reshape(-1), nthreads),
               "omr_gen_clues")
        return a, b

    # Device generators: same streams, bit-identical results, written to
    # device buffers (ABI layout) of the current HIP device; return when the stream is done.
    def gen_clues_device(self, seed: int, first: int, count: int, d_clue_a: int, d_clue_b: int, stream: int = 0):
        _check(lib().omr_gen_clues_device(self._h, seed, first, count, d_clue_a, d_clue_b, stream or None),
               "omr_gen_clues_device")

    def generate_detection_key_device(self, seed: int, d_bsk1: int, d_ksk: int, d_bsk2: int, d_trace_key: int,
                                      stream: int = 0):
        _check(lib().omr_keygen_detection_key_device(self._h, seed, d_bsk1, d_ksk, d_bsk2, d_trace_key,
                                                     stream or None), "omr_keygen_detection_key_device")

    def generate_seeded_key_device(self, seed: int, mask_seed: int, d_bsk1_b: int, d_ksk_b: int, d_bsk2_b: int,
                                   d_trace_key_b: int, stream: int = 0):
        _check(lib().omr_keygen_seeded_key_device(self._h, seed, mask_seed, d_bsk1_b, d_ksk_b, d_bsk2_b,
                                                  d_trace_key_b, stream or None), "omr_keygen_seeded_key_device")

    # Sender side and clue opening (include/omr_gpu.h "Sender")
    def clue_key(self) -> "ClueKey":
        """SecretKeyPack::generate_clue_key (key_gen/secret.rs:99-107): the public key a sender needs."""
        w = np.empty((2, N0), np.uint16)
        _check(lib().omr_secret_clue_key(self._h, w.ctypes.data), "omr_secret_clue_key")
        return ClueKey(w[0], w[1])

    def open_clues(self, clue_a, clue_b, values: bool = True, pertinent: bool = True, noise: bool = True,
                   nthreads: int = 0) -> dict:
        """SecretKeyPack::decrypt_clue (secret.rs:267-270) for all 7 clues of each message, on the CPU:
        values u8 [count][7], pertinent u8 [count], max_abs_noise u8 [count] (those asked for)."""
        a = np.ascontiguousarray(clue_a, np.uint16).reshape(-1, N0)
        b = np.ascontiguousarray(clue_b, np.uint16).reshape(-1, CLUE_COUNT)
        n = a.shape[0]
        assert b.shape[0] == n
        out = {}
        if values:
            out["values"] = np.empty((n, CLUE_COUNT), np.uint8)
        if pertinent:
            out["pertinent"] = np.empty(n, np.uint8)
        if noise:
            out["max_abs_noise"] = np.empty(n, np.uint8)
        ptr = [out[k].ctypes.data if k in out else None for k in ("values", "pertinent", "max_abs_noise")]
        _check(lib().omr_clue_open(self._h, a.ctypes.data, b.ctypes.data, n, ptr[0], ptr[1], ptr[2], nthreads),
               "omr_clue_open")
        return out

    def open_clues_device(self, d_clue_a: int, d_clue_b: int, count: int, d_values: int = 0, d_pertinent: int = 0,
                          d_max_abs_noise: int = 0, stream: int = 0) -> None:
        """The same on device buffers of the current HIP device; returns when the stream is done."""
        _check(lib().omr_clue_open_device(self._h, d_clue_a or None, d_clue_b or None, count, d_values or None,
                                          d_pertinent or None, d_max_abs_noise or None, stream or None),
               "omr_clue_open_device")


@dataclass
class ClueKey:
    """omr_clue_key: LwePublicKeyRlweMode (A, B = A s0 + E) over Z_2048[X]/(X^512 + 1), u16 [512] each."""
    a: np.ndarray
    b: np.ndarray

    def words(self) -> np.ndarray:
        """The wire form, u16 [2][512]."""
        return np.stack([np.asarray(self.a, np.uint16).reshape(N0), np.asarray(self.b, np.uint16).reshape(N0)])


def _clue_key_table(keys) -> np.ndarray:
    """ClueKey, a sequence of them, or an array [n][2][512] -> contiguous u16 [n][2][512]."""
    if isinstance(keys, ClueKey):
        keys = [keys]
    if not isinstance(keys, np.ndarray):
        keys = np.stack([k.words() for k in keys]) if len(keys) else np.empty((0, 2, N0), np.uint16)
    return np.ascontiguousarray(keys, np.uint16).reshape(-1, 2, N0)


def clue_key_noise_support() -> int:
    k = C.c_uint64()
    _check(lib().omr_clue_key_noise_support(C.byref(k)), "omr_clue_key_noise_support")
    return k.value


def validate_clue_keys(keys) -> int:
    """The words >= 2048 of a table of clue keys (reports, does not reject)."""
    t = _clue_key_table(keys)
    n = C.c_uint64()
    _check(lib().omr_clue_key_validate(t.ctypes.data, t.shape[0], C.byref(n)), "omr_clue_key_validate")
    return n.value


def audit_clue_key(secret: "SecretKeyPack", key, limit: int = None) -> dict:
    """omr_clue_key_audit: the noise B - A s0 of a clue key against the pack's s0 (limit None = K)."""
    t = _clue_key_table(key)
    assert t.shape[0] == 1
    mx, over, nc = C.c_uint64(), C.c_uint32(), C.c_uint32()
    _check(lib().omr_clue_key_audit(secret._h, t.ctypes.data, (1 << 64) - 1 if limit is None else limit,
                                    C.byref(mx), C.byref(over), C.byref(nc)), "omr_clue_key_audit")
    return dict(max_abs_noise=mx.value, coeffs_over=over.value, noncanonical=nc.value)


class Sender:
    """Sender::new / Sender::gen_clues (sender.rs:27-32) over a table of public clue keys: the clue of
    global message index first + m under key recipient[m]. device None: CPU only."""

    def __init__(self, keys, device: int = None):
        t = _clue_key_table(keys)
        h = C.c_void_p()
        _check(lib().omr_sender_create(t.ctypes.data, t.shape[0], -1 if device is None else device, C.byref(h)),
               "omr_sender_create")
        self._h = h
        self.n_keys = t.shape[0]
        self._destroy = lib().omr_sender_destroy

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def gen_clues(self, seed: int, first: int, count: int, recipient=None, nthreads: int = 0, out=None):
        """(clue_a u16 [count][512], clue_b u16 [count][7]); out = (clue_a, clue_b) writes into given arrays."""
        a, b = out if out is not None else (np.empty((count, N0), np.uint16), np.empty((count, CLUE_COUNT), np.uint16))
        assert a.dtype == np.uint16 and b.dtype == np.uint16 and a.size == count * N0 and b.size == count * CLUE_COUNT
        assert a.flags.c_contiguous and b.flags.c_contiguous
        r = None if recipient is None else np.ascontiguousarray(recipient, np.uint32)
        assert r is None or r.shape == (count,)
        _check(lib().omr_sender_gen_clues(self._h, None if r is None else r.ctypes.data, seed, first, count,
                                          a.ctypes.data, b.ctypes.data, nthreads), "omr_sender_gen_clues")
        return a, b

    def gen_clues_device(self, seed: int, first: int, count: int, d_clue_a: int, d_clue_b: int, d_recipient: int = 0,
                         stream: int = 0) -> None:
        """The same bits into device buffers of the sender's device; d_recipient u32 [count] or 0."""
        _check(lib().omr_sender_gen_clues_device(self._h, d_recipient or None, seed, first, count, d_clue_a or None,
                                                 d_clue_b or None, stream or None), "omr_sender_gen_clues_device")


# ---- on-disk container (the reference has no serialization) ----------------
# Little-endian: b"OMRF" | u32 version = 1 | u32 kind | u32 n_arrays | n_arrays x
# {u32 dtype (1 = u16, 2 = u32, 3 = u64), u32 ndim, u64 dims[4]} | arrays in order, each starting
# at a 64-byte aligned offset, C order. Kinds: 1 detection key (bsk1, ksk, bsk2, trace_key in the
# ABI layout of include/omr_gpu.h), 2 clues (clue_a [D][512], clue_b [D][7], first_index [1]),
# 3 NttRlweCiphertexts (u64 [n][2][2048], e.g. a pertinency vector or a digest), 4 seeded detection key
# (bsk1_b, ksk_b, bsk2_b, trace_key_b in the layout of include/omr_gpu.h, then mask_seed u64 [1]).
_FILE_MAGIC, _FILE_VERSION = b"OMRF", 1
KIND_DETECTION_KEY, KIND_CLUES, KIND_CIPHERTEXTS, KIND_SEEDED_KEY = 1, 2, 3, 4
_DT = {np.dtype(np.uint16): 1, np.dtype(np.uint32): 2, np.dtype(np.uint64): 3}
_DT_INV = {v: k for k, v in _DT.items()}


def write_arrays(path: str, kind: int, arrays) -> None:
    arrays = [np.ascontiguousarray(a) for a in arrays]
    head = bytearray(_FILE_MAGIC + np.array([_FILE_VERSION, kind, len(arrays)], "<u4").tobytes())
    for a in arrays:
        if a.dtype not in _DT or a.ndim > 4:
            raise OmrError(f"unsupported array {a.dtype} ndim {a.ndim}")
        dims = list(a.shape) + [0] * (4 - a.ndim)
        head += np.array([_DT[a.dtype], a.ndim], "<u4").tobytes() + np.array(dims, "<u8").tobytes()
    with open(path, "wb") as f:
        f.write(head)
        for a in arrays:
            f.write(b"\0" * (-f.tell() % 64))
            f.write(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes())


def read_arrays(path: str, kind: int):
    """Arrays of an OMRF file (memory-mapped, read-only) after checking magic, version and kind."""
    with open(path, "rb") as f:
        hdr = f.read(16)
        if len(hdr) < 16 or hdr[:4] != _FILE_MAGIC:
            raise OmrError(f"{path}: not an OMRF file")
        version, k, n = np.frombuffer(hdr[4:16], "<u4")
        if version != _FILE_VERSION or k != kind:
            raise OmrError(f"{path}: version {version} kind {k}, expected {_FILE_VERSION} / {kind}")
        descs = [f.read(40) for _ in range(n)]
        off = f.tell()
    out = []
    for d in descs:
        dt, nd = np.frombuffer(d[:8], "<u4")
        shape = tuple(int(x) for x in np.frombuffer(d[8:], "<u8")[:nd])
        off += -off % 64
        a = np.memmap(path, dtype=_DT_INV[int(dt)].newbyteorder("<"), mode="r", offset=off, shape=shape)
        out.append(a)
        off += a.nbytes
    return out


def save_detection_key(path: str, dk: "DetectionKey") -> None:
    write_arrays(path, KIND_DETECTION_KEY, [dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key])


def load_detection_key(path: str) -> "DetectionKey":
    b1, k, b2, t = read_arrays(path, KIND_DETECTION_KEY)
    return DetectionKey(bsk1=np.array(b1), ksk=np.array(k), bsk2=np.array(b2), trace_key=np.array(t))


def save_seeded_key(path: str, sk: "SeededKey") -> None:
    write_arrays(path, KIND_SEEDED_KEY, [sk.bsk1_b, sk.ksk_b, sk.bsk2_b, sk.trace_key_b,
                                         np.array([sk.mask_seed], np.uint64)])


def load_seeded_key(path: str) -> "SeededKey":
    b1, k, b2, t, seed = read_arrays(path, KIND_SEEDED_KEY)
    return SeededKey(np.array(b1), np.array(k), np.array(b2), np.array(t), int(seed[0]))


def save_clues(path: str, clue_a, clue_b, first: int = 0) -> None:
    write_arrays(path, KIND_CLUES, [np.asarray(clue_a, np.uint16), np.asarray(clue_b, np.uint16),
                                    np.array([first], np.uint64)])


def load_clues(path: str):
    """(clue_a, clue_b, first_index)."""
    a, b, first = read_arrays(path, KIND_CLUES)
    return np.array(a), np.array(b), int(first[0])


def save_ciphertexts(path: str, cts) -> None:
    write_arrays(path, KIND_CIPHERTEXTS, [np.asarray(cts, np.uint64).reshape(-1, 2, N2)])


def load_ciphertexts(path: str) -> np.ndarray:
    return np.array(read_arrays(path, KIND_CIPHERTEXTS)[0])


def fft_twiddles_dd(level: int) -> np.ndarray:
    """The key transform's double-double twiddles [n - 1][4] (re.hi, re.lo, im.hi, im.lo)."""
    n = 512 if level == 1 else 1024
    out = np.zeros(4 * (n - 1), dtype=np.float64)
    _check(lib().omr_fft_twiddles_dd(int(level), out), "omr_fft_twiddles_dd")
    return out.reshape(n - 1, 4)


BITMAP_BITS, BITMAP_MESSAGES_PER_CT = 8, 16384


def bitmap_ct_count(all_payloads_count: int) -> int:
    """omr_bitmap_ct_count: bitmap ciphertexts of a board, ceil(all / 16384)."""
    n = C.c_uint32()
    _check(lib().omr_bitmap_ct_count(all_payloads_count, C.byref(n)), "omr_bitmap_ct_count")
    return n.value


def _indices_call(call, what, cap):
    """Runs call(indices pointer, cap, found) and once more with room for `found` if cap was too small."""
    while True:
        buf = np.zeros(max(1, cap), dtype=np.uintp)
        found = C.c_size_t()
        _check(call(buf.ctypes.data, buf.size, C.byref(found)), what)
        if found.value <= buf.size:
            return [int(v) for v in buf[:found.value]]
        cap = found.value


def bitmap_indices(decoded, all_payloads_count: int, cap: int = 1024) -> list[int]:
    """omr_bitmap_indices: the global indices of the set bits of decoded bitmap ciphertexts
    ([n_ct][2048] values < 256, e.g. Auditor.audit's `decoded` or Retriever.decrypt_decode), increasing."""
    d = np.ascontiguousarray(decoded).reshape(-1, N2)
    if d.dtype != np.uint16:
        if (d > 0xFFFF).any():
            raise OmrError("decoded bitmap values must fit 16 bits")
        d = d.astype(np.uint16)
    return _indices_call(lambda i, c, f: lib().omr_bitmap_indices(d.reshape(-1), d.shape[0], all_payloads_count,
                                                                  i, c, f), "omr_bitmap_indices", cap)


def detect_kernels() -> dict:
    """{'br1': name, 'ks': name, 'br2': name} of the kernels this build launches."""
    return dict(kv.split("=") for kv in lib().omr_detect_kernels().decode().split())


class Retriever:
    """Retriever (retriever.rs:25-260): client-side digest decoding with the pack's s2 (CPU)."""

    def __init__(self, params: RetrievalParams, secret: "SecretKeyPack"):
        self.params = params
        self._sk = secret

    def decrypt_decode(self, cts) -> np.ndarray:
        """Decoded plaintexts mod 257 of NttRlweCiphertexts u64 [n][2][2048]: u32 [n][2048]."""
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2, N2)
        out = np.empty((cts.shape[0], N2), np.uint32)
        _check(lib().omr_decrypt_decode(self._sk._h, cts.reshape(-1), cts.shape[0], out.reshape(-1)),
               "omr_decrypt_decode")
        return out

    def decode_pertinent_indices(self, idx_cts) -> list[int]:
        rp = self.params
        cts = np.ascontiguousarray(idx_cts, dtype=np.uint64).reshape(-1, 2, N2)
        buf = np.zeros(max(1, rp.pertinent_count) * 4 + 64, dtype=np.uintp)
        found = C.c_size_t()
        _check(lib().omr_retrieve_indices(self._sk._h, cts.reshape(-1), cts.shape[0], rp.all_payloads_count,
                                          rp.pertinent_count, buf, buf.size, C.byref(found)),
               "omr_retrieve_indices")
        return [int(v) for v in buf[:min(found.value, buf.size)]]

    def decode_combined_payloads_and_solve(self, pay_cts, weights, indices) -> np.ndarray:
        rp = self.params
        cts = np.ascontiguousarray(pay_cts, dtype=np.uint64).reshape(-1, 2, N2)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        out = np.zeros((len(idx), PAYLOAD_LENGTH), np.uint16)
        _check(lib().omr_retrieve_payloads(self._sk._h, cts.reshape(-1), cts.shape[0], rp.all_payloads_count,
                                           rp.combination_count,
                                           np.ascontiguousarray(weights, dtype=np.uint16).reshape(-1), idx,
                                           len(idx), out.reshape(-1)), "omr_retrieve_payloads")
        return out

    def decode_combined_payloads_and_solve_indexed(self, pay_cts, seed: bytes, indices) -> np.ndarray:
        """omr_retrieve_payloads_indexed: the same solve, the matrix from the indexed weights of `seed`."""
        rp = self.params
        cts = np.ascontiguousarray(pay_cts, dtype=np.uint64).reshape(-1, 2, N2)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        out = np.zeros((len(idx), PAYLOAD_LENGTH), np.uint16)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_retrieve_payloads_indexed(self._sk._h, cts.reshape(-1), cts.shape[0], rp.all_payloads_count,
                                                   rp.combination_count, ptr, idx, len(idx), out.reshape(-1)),
               "omr_retrieve_payloads_indexed")
        return out

    def decode_combined_payloads_and_solve_indexed_len(self, pay_cts, seed: bytes, indices,
                                                       layout: "PayloadLayout") -> np.ndarray:
        """omr_retrieve_payloads_indexed_len: u16 [len(indices)][layout.payload_len] from a digest of `layout`."""
        cts = np.ascontiguousarray(pay_cts, dtype=np.uint64).reshape(-1, 2, N2)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        out = np.zeros((len(idx), layout.payload_len if layout else 0), np.uint16)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_retrieve_payloads_indexed_len(self._sk._h, cts.ctypes.data, cts.shape[0],
                                                       self.params.all_payloads_count, _layout_ref(layout), ptr,
                                                       idx.ctypes.data, len(idx), out.ctypes.data),
               "omr_retrieve_payloads_indexed_len")
        return out

    def decode_combined_payloads_and_solve_seek(self, pay_cts, seed: bytes, indices, seek: "WeightSeek" = None,
                                                combination_count: int = None) -> np.ndarray:
        """omr_retrieve_payloads_seek: the solve of decode_combined_payloads_and_solve, the matrix taken from
        the reference's stream through the seek (None: built inside the call); no table."""
        rp = self.params
        cts = np.ascontiguousarray(pay_cts, dtype=np.uint64).reshape(-1, 2, N2)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        out = np.zeros((len(idx), PAYLOAD_LENGTH), np.uint16)
        ptr, _keep = _seed_ptr(seed)
        cc = rp.combination_count if combination_count is None else combination_count
        _check(lib().omr_retrieve_payloads_seek(self._sk._h, cts.ctypes.data, cts.shape[0], rp.all_payloads_count, cc,
                                                ptr, _seek_ptr(seek), idx.ctypes.data, len(idx), out.ctypes.data),
               "omr_retrieve_payloads_seek")
        return out

    def decode_bitmap(self, bitmap_cts, cap: int = 1024) -> list[int]:
        """omr_retrieve_bitmap: every pertinent global index of the board, increasing, from its bitmap
        digest u64 [bitmap_ct_count(all)][2][2048]; needs no pertinent count."""
        cts = np.ascontiguousarray(bitmap_cts, dtype=np.uint64).reshape(-1, 2, N2)
        return _indices_call(lambda i, c, f: lib().omr_retrieve_bitmap(
            self._sk._h, cts.reshape(-1), cts.shape[0], self.params.all_payloads_count, i, c, f),
            "omr_retrieve_bitmap", cap)

    def decode_digest(self, idx_cts, pay_cts, seed: bytes, indexed: bool = False):
        """Retriever::decode_digest: sorted pertinent indices and their payloads (mod 257); the
        weights and the system's rows follow the board's RetrievalParams (retriever.rs:196, :215-239).
        indexed=True: the digest was encoded with indexed weights; no board-wide table is drawn."""
        indices = self.decode_pertinent_indices(idx_cts)
        if indexed:
            return indices, self.decode_combined_payloads_and_solve_indexed(pay_cts, seed, indices)
        weights = payload_weights(seed, self.params)
        return indices, self.decode_combined_payloads_and_solve(pay_cts, weights, indices)


# ---- solve mod 257 (include/omr_gpu.h, "Solve mod 257") ---------------------------------------
SOLVE_MAX_ROWS = 8192
NOT_INVERTIBLE = 4  # OMR_ERR_NOT_INVERTIBLE


class SingularMatrix(OmrError):
    """OMR_ERR_NOT_INVERTIBLE of a solve: `column` is the first column without a pivot."""

    def __init__(self, column: int):
        super().__init__(f"omr_solve_mod257 failed ({NOT_INVERTIBLE}): Matrix is not invertible (column {column})")
        self.column = column


def solve_geometry() -> dict:
    """omr_solve_geometry: {'panel_cols', 'tile_rows', 'tile_width'} of the device solver of this build."""
    p, r, w = C.c_uint(), C.c_uint(), C.c_uint()
    _check(lib().omr_solve_geometry(C.byref(p), C.byref(r), C.byref(w)), "omr_solve_geometry")
    return {"panel_cols": p.value, "tile_rows": r.value, "tile_width": w.value}


def solve_mod257_cpu(matrix, rhs, nthreads: int = 1) -> np.ndarray:
    """omr_solve_mod257_cpu: the solution u16 [cols][width] of [matrix | rhs] mod 257 (matrix u16 [rows][cols],
    rhs u16 [rows][width], words reduced mod 257 first) by solve_matrix_mod_257's elimination; raises
    SingularMatrix (with the column) when a column has no pivot."""
    m = np.ascontiguousarray(matrix, dtype=np.uint16)
    r = np.ascontiguousarray(rhs, dtype=np.uint16)
    if m.ndim != 2 or r.ndim != 2 or m.shape[0] != r.shape[0]:
        raise OmrError("solve_mod257_cpu: matrix [rows][cols] and rhs [rows][width] expected")
    rows, cols = m.shape
    out = np.zeros((cols, r.shape[1]), np.uint16)
    col = C.c_size_t()
    st = lib().omr_solve_mod257_cpu(m.ctypes.data, r.ctypes.data, rows, cols, r.shape[1], out.ctypes.data,
                                    C.byref(col), nthreads)
    if st == NOT_INVERTIBLE:
        raise SingularMatrix(col.value)
    _check(st, "omr_solve_mod257_cpu")
    return out


# ---- compact ciphertexts (include/omr_gpu.h, "Compact ciphertexts") ---------------------------
COMPACT_MIN_BITS, COMPACT_MAX_BITS = 16, 32


def compact_ct_bytes(bits: int) -> int:
    """omr_compact_ct_bytes: 512 * bits bytes per compact ciphertext."""
    n = C.c_size_t()
    _check(lib().omr_compact_ct_bytes(bits, C.byref(n)), "omr_compact_ct_bytes")
    return n.value


def compact_residual_bound(secret: "SecretKeyPack", bits: int) -> int:
    """omr_compact_residual_bound: R(bits) for the pack's s2, in the auditor's residual units."""
    r = C.c_uint64()
    _check(lib().omr_compact_residual_bound(secret._h, bits, C.byref(r)), "omr_compact_residual_bound")
    return r.value


def _packed(packed, bits: int) -> np.ndarray:
    """Compact ciphertexts as u8 [n][512 * bits]."""
    p = np.ascontiguousarray(packed, dtype=np.uint8)
    ctb = compact_ct_bytes(bits)
    if p.size % ctb:
        raise OmrError(f"compact ciphertexts at {bits} bits must be a multiple of {ctb} bytes")
    return p.reshape(-1, ctb)


def compact_cts_cpu(cts, bits: int, nthreads: int = 0) -> np.ndarray:
    """omr_compact_cts_cpu: NttRlweCiphertexts u64 [n][2][2048] -> u8 [n][512 * bits], on the CPU."""
    cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2, N2)
    out = np.empty((cts.shape[0], compact_ct_bytes(bits)), np.uint8)
    _check(lib().omr_compact_cts_cpu(cts.ctypes.data, cts.shape[0], bits, out.ctypes.data, nthreads),
           "omr_compact_cts_cpu")
    return out


def compact_expand_cpu(packed, bits: int, nthreads: int = 0) -> np.ndarray:
    """omr_compact_expand_cpu: u8 [n][512 * bits] -> NttRlweCiphertexts u64 [n][2][2048], on the CPU."""
    p = _packed(packed, bits)
    out = np.empty((p.shape[0], 2, N2), np.uint64)
    _check(lib().omr_compact_expand_cpu(p.ctypes.data, p.shape[0], bits, out.ctypes.data, nthreads),
           "omr_compact_expand_cpu")
    return out


def _summary_dict(t: "_AuditSummary") -> dict:
    d = {n: int(getattr(t, n)) for n in ("ciphertexts", "zero", "one_hot", "other", "max_abs_residual")}
    d["residual_bits"] = np.array(t.residual_bits[:], dtype=np.uint64)
    return d


def audit_classes(records):
    """(zero, one_hot, other) index arrays of audit records: zero has no decoded coefficient != 0,
    one-hot decodes to [1, 0, .., 0] (the omd KAT of a pertinent message), other is anything else."""
    r = np.asarray(records)
    zero = r["nonzero"] == 0
    one_hot = (r["nonzero"] == 1) & (r["first"] == 1)
    return np.nonzero(zero)[0], np.nonzero(one_hot)[0], np.nonzero(~zero & ~one_hot)[0]


def _audit_host(call, what, cts):
    cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2, N2)
    n = cts.shape[0]
    records = np.zeros(n, AUDIT_RECORD)
    decoded = np.zeros((n, N2), np.uint16)
    t = _AuditSummary()
    _check(call(cts.ctypes.data, n, records.ctypes.data, decoded.ctypes.data, C.addressof(t)), what)
    return records, decoded, _summary_dict(t)


def audit_cpu(secret: "SecretKeyPack", cts, nthreads: int = 0):
    """omr_audit_cpu: (records [n] of AUDIT_RECORD, decoded u16 [n][2048], summary dict) of
    NttRlweCiphertexts u64 [n][2][2048] under the pack's s2, on the CPU (no GPU, no auditor)."""
    return _audit_host(lambda c, n, r, d, s: lib().omr_audit_cpu(secret._h, c, n, r, d, s, nthreads),
                       "omr_audit_cpu", cts)


# ---- key audit (include/omr_gpu.h, "Key audit") ----
KEY_LIMIT_K = 2**64 - 1  # a limit that stands for the generators' noise support K
# words per row of each component in the key layout (an RLWE row is a then b; a KSK row a[670] then b)
KEY_ROW_ELEMS = (2 * N1, NI + 1, 2 * N2, 2 * N2)


def key_noise_support(component: int) -> int:
    """omr_key_noise_support: the largest |e| the generators can draw for the component."""
    k = C.c_uint64()
    _check(lib().omr_key_noise_support(component, C.byref(k)), "omr_key_noise_support")
    return k.value


def _key_summary_new() -> "_KeyAuditSummary":
    t = _KeyAuditSummary()
    t.first_row_over = 2**64 - 1
    return t


def _key_summary_dict(t: "_KeyAuditSummary") -> dict:
    d = {n: int(getattr(t, n)) for n in ("rows", "noncanonical", "max_abs_noise", "rows_over", "first_row_over")}
    d["noise_bits"] = np.array(t.noise_bits[:], dtype=np.uint64)
    return d


def key_summary_init_bytes() -> bytes:
    """An omr_key_audit_summary to add into (440 bytes): zeros with first_row_over = UINT64_MAX."""
    return bytes(_key_summary_new())


def key_summary_from_bytes(buf) -> dict:
    """The dict form of an omr_key_audit_summary copied back from the device (440 bytes)."""
    return _key_summary_dict(_KeyAuditSummary.from_buffer_copy(bytes(buf)))


def _key_rows(component: int, rows) -> np.ndarray:
    if not 0 <= component < 4:
        return np.ascontiguousarray(rows).reshape(1, -1)  # the library reports the component
    return np.ascontiguousarray(rows, dtype=KEY_COMPONENTS[component][2]).reshape(-1, KEY_ROW_ELEMS[component])


def audit_key_rows_cpu(secret: "SecretKeyPack", component: int, rows, first_row: int = 0, limit: int = KEY_LIMIT_K,
                       nthreads: int = 0, n_rows: int = None):
    """omr_audit_key_rows_cpu over host rows [n][row words] that start at component row first_row:
    (row_max u64 [n], summary dict)."""
    r = _key_rows(component, rows)
    n = r.shape[0] if n_rows is None else n_rows
    row_max = np.zeros(max(n, 0), np.uint64)
    t = _key_summary_new()
    _check(lib().omr_audit_key_rows_cpu(secret._h, component, r.ctypes.data, first_row, n, limit, row_max.ctypes.data,
                                        C.addressof(t), nthreads), "omr_audit_key_rows_cpu")
    return row_max, _key_summary_dict(t)


def _limits(limit):
    return None if limit is None else (C.c_uint64 * 4)(*limit)


def _key_view(key) -> "_KeyView":
    """A DetectionKey (host arrays) or four raw pointers (host or device memory; 0 skips a component)."""
    if isinstance(key, DetectionKey):
        arrs = [np.ascontiguousarray(a) for a in (key.bsk1, key.ksk, key.bsk2, key.trace_key)]
        v = _KeyView(*[a.ctypes.data for a in arrs])
        v._keep = arrs
        return v
    return _KeyView(*[p or None for p in key])


def _key_audit_whole(call, what, view, limit):
    out = (_KeyAuditSummary * 4)(*[_key_summary_new() for _ in range(4)])
    _check(call(C.byref(view), _limits(limit), out), what)
    return [_key_summary_dict(t) for t in out]


def audit_key_cpu(secret: "SecretKeyPack", key, limit=None, nthreads: int = 0):
    """omr_audit_key_cpu: the four summaries (omr_key_component order) of a key in host memory."""
    return _key_audit_whole(lambda v, l, o: lib().omr_audit_key_cpu(secret._h, v, l, o, nthreads), "omr_audit_key_cpu",
                            _key_view(key), limit)


def validate_key(key, device: int = None, nthreads: int = 0) -> list:
    """Words >= q per component, without a secret: omr_key_validate* of a DetectionKey / SeededKey in host
    memory, or with `device` of four raw device pointers (a fifth entry, the mask seed, marks a seeded key's
    bodies)."""
    out = (C.c_uint64 * 4)()
    seeded = isinstance(key, SeededKey) or (not isinstance(key, DetectionKey) and len(key) == 5)
    if isinstance(key, SeededKey):
        view = key._view()
    elif seeded:
        view = _SeededKeyView(*[p or None for p in key[:4]], key[4])
    else:
        view = _key_view(key)
    name = "omr_key_validate" + ("_seeded" if seeded else "") + ("" if device is None else "_device")
    if device is None:
        _check(getattr(lib(), name)(C.byref(view), out, nthreads), name)
    else:
        _check(getattr(lib(), name)(C.byref(view), device, out), name)
    return [int(v) for v in out]


def key_count_noncanonical_device(level: int, d_words: int, n: int, d_count: int, stream: int = 0) -> None:
    """omr_key_count_noncanonical_device: adds the words >= q of the level into the u64 at d_count."""
    _check(lib().omr_key_count_noncanonical_device(level, d_words or None, n, d_count or None, stream or None),
           "omr_key_count_noncanonical_device")


class Auditor:
    """omr_auditor: the level-2 secret on one device; decrypts, classifies and noise-audits
    NttRlweCiphertexts (pertinency vectors, digests) on the GPU. The counterpart of the reference's
    NoiseSigmaInfo (retriever.rs:390-560) and of the omd KAT (omd.rs:48-58), in exact integers."""

    classes = staticmethod(audit_classes)

    def __init__(self, pack: "SecretKeyPack", device: int = 0):
        h = C.c_void_p()
        _check(lib().omr_auditor_create(pack._h, device, C.byref(h)), "omr_auditor_create")
        self._h = h
        self._destroy = lib().omr_auditor_destroy
        self._sk = pack
        self.device = device

    def set_grid(self, workgroups: int = 0):
        _check(lib().omr_auditor_set_grid(self._h, workgroups), "omr_auditor_set_grid")

    def set_staging(self, max_ciphertexts: int = 0):
        _check(lib().omr_auditor_set_staging(self._h, max_ciphertexts), "omr_auditor_set_staging")

    def audit(self, cts):
        """Host ciphertexts u64 [n][2][2048] through the device (omr_audit): (records, decoded, summary)."""
        return _audit_host(lambda c, n, r, d, s: lib().omr_audit(self._h, c, n, r, d, s), "omr_audit", cts)

    def audit_cpu(self, cts, nthreads: int = 0):
        """The same results from omr_audit_cpu."""
        return audit_cpu(self._sk, cts, nthreads)

    def audit_device(self, d_cts: int, n: int, d_records: int = 0, d_decoded: int = 0, d_summary: int = 0,
                     stream: int = 0) -> None:
        """Device pointers (omr_audit_device): d_records [n] of 16-byte records, d_decoded u16 [n][2048],
        d_summary 440 bytes that are added into (the caller zeroes them); 0 skips an output. Enqueued
        on `stream`; the caller synchronises."""
        _check(lib().omr_audit_device(self._h, d_cts, n, d_records or None, d_decoded or None, d_summary or None,
                                      stream or None), "omr_audit_device")

    def audit_compact(self, packed, bits: int):
        """Compact ciphertexts u8 [n][512 * bits] in host memory through the device (omr_audit_compact):
        expanded and audited there; (records, decoded, summary) as from audit() of their expansion."""
        p = _packed(packed, bits)
        n = p.shape[0]
        records = np.zeros(n, AUDIT_RECORD)
        decoded = np.zeros((n, N2), np.uint16)
        t = _AuditSummary()
        _check(lib().omr_audit_compact(self._h, p.ctypes.data, n, bits, records.ctypes.data, decoded.ctypes.data,
                                       C.addressof(t)), "omr_audit_compact")
        return records, decoded, _summary_dict(t)

    def expand_device(self, d_packed: int, n: int, bits: int, d_cts: int, stream: int = 0) -> None:
        """Device pointers (omr_compact_expand_device): n compact ciphertexts -> u64 [n][2][2048]. Enqueued
        on `stream`; the caller synchronises."""
        _check(lib().omr_compact_expand_device(self._h, d_packed or None, n, bits, d_cts or None, stream or None),
               "omr_compact_expand_device")

    def audit_key(self, key, limit=None) -> list:
        """omr_audit_key: the four summaries (omr_key_component order) of a DetectionKey in host memory or of
        four raw pointers (host or device memory of the auditor's device; 0 skips a component). limit: four
        values, None = the generators' support K."""
        return _key_audit_whole(lambda v, l, o: lib().omr_audit_key(self._h, v, l, o), "omr_audit_key", _key_view(key),
                                limit)

    def audit_seeded_key(self, key, limit=None) -> list:
        """omr_audit_key_seeded: a SeededKey (host bodies) or (bsk1_b, ksk_b, bsk2_b, trace_key_b, mask_seed)
        raw pointers, expanded on the device into temporaries and audited there."""
        view = key._view() if isinstance(key, SeededKey) else _SeededKeyView(*[p or None for p in key[:4]], key[4])
        return _key_audit_whole(lambda v, l, o: lib().omr_audit_key_seeded(self._h, v, l, o), "omr_audit_key_seeded",
                                view, limit)

    def audit_key_cpu(self, key, limit=None, nthreads: int = 0) -> list:
        """The same results from omr_audit_key_cpu."""
        return audit_key_cpu(self._sk, key, limit, nthreads)

    def audit_key_rows(self, component: int, d_rows: int, first_row: int, rows: int, limit: int = KEY_LIMIT_K,
                       d_row_max: int = 0, d_summary: int = 0, stream: int = 0) -> None:
        """Device pointers (omr_audit_key_rows_device): d_rows at component row first_row, d_row_max u64 [rows],
        d_summary 440 bytes that are added into (key_summary_init_bytes()); 0 skips an output. Enqueued on
        `stream`; the caller synchronises."""
        _check(lib().omr_audit_key_rows_device(self._h, component, d_rows or None, first_row, rows, limit,
                                               d_row_max or None, d_summary or None, stream or None),
               "omr_audit_key_rows_device")

    # ---- solve mod 257 and retrieval on the device (include/omr_gpu.h, "Solve mod 257") ----
    def solve_mod257_device(self, d_matrix: int, d_rhs: int, rows: int, cols: int, width: int, d_solution: int,
                            d_status: int, stream: int = 0) -> None:
        """Device pointers (omr_solve_mod257_device): d_matrix u16 [rows][cols], d_rhs u16 [rows][width],
        d_solution u16 [cols][width], d_status u32 (0 = solved, 1 + i = no pivot in column i, d_solution then
        not written). Enqueued on `stream`; the caller synchronises."""
        _check(lib().omr_solve_mod257_device(self._h, d_matrix or None, d_rhs or None, rows, cols, width,
                                             d_solution or None, d_status or None, stream or None),
               "omr_solve_mod257_device")

    def solve_profile(self, enable: bool = True) -> list:
        """omr_solve_profile: synchronises the last solve and returns its device milliseconds per step [panel,
        swaps and pivot block, trailing update, back substitution] (zeros unless it was profiled); later solves
        are profiled if `enable`."""
        ms = (C.c_float * 4)()
        _check(lib().omr_solve_profile(self._h, int(enable), C.byref(ms)), "omr_solve_profile")
        return [float(v) for v in ms]

    @staticmethod
    def _cts(cts, bits: int) -> np.ndarray:
        """Full (bits = 0: u64 [n][2][2048]) or compact (u8 [n][512 * bits]) ciphertexts, n in shape[0]."""
        if bits:
            return _packed(cts, bits)
        return np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2, N2)

    def retrieve_indices(self, idx_cts, all_payloads_count: int, pertinent_count: int, bits: int = 0,
                         cap: int = None) -> list:
        """omr_auditor_retrieve_indices: Retriever.decode_pertinent_indices with the decode on the device; every
        index found, increasing."""
        c = self._cts(idx_cts, bits)
        return _indices_call(lambda i, n, f: lib().omr_auditor_retrieve_indices(
            self._h, c.ctypes.data, c.shape[0], bits, all_payloads_count, pertinent_count, i, n, f),
            "omr_auditor_retrieve_indices", max(1, pertinent_count) * 4 + 64 if cap is None else cap)

    def retrieve_payloads(self, pay_cts, all_payloads_count: int, combination_count: int, weights, indices,
                          bits: int = 0) -> np.ndarray:
        """omr_auditor_retrieve_payloads: u16 [len(indices)][612], the table path of
        Retriever.decode_combined_payloads_and_solve with decode, right-hand side and solve on the device."""
        c = self._cts(pay_cts, bits)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        w = np.ascontiguousarray(weights, dtype=np.uint16).reshape(-1)
        out = np.zeros((len(idx), PAYLOAD_LENGTH), np.uint16)
        _check(lib().omr_auditor_retrieve_payloads(self._h, c.ctypes.data, c.shape[0], bits, all_payloads_count,
                                                   combination_count, w.ctypes.data, idx.ctypes.data, len(idx),
                                                   out.ctypes.data), "omr_auditor_retrieve_payloads")
        return out

    def retrieve_payloads_indexed(self, pay_cts, all_payloads_count: int, combination_count: int, seed: bytes, indices,
                                  bits: int = 0) -> np.ndarray:
        """omr_auditor_retrieve_payloads_indexed: the same with the matrix built on the device from the indexed
        weights of `seed`."""
        c = self._cts(pay_cts, bits)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        out = np.zeros((len(idx), PAYLOAD_LENGTH), np.uint16)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_auditor_retrieve_payloads_indexed(self._h, c.ctypes.data, c.shape[0], bits, all_payloads_count,
                                                           combination_count, ptr, idx.ctypes.data, len(idx),
                                                           out.ctypes.data), "omr_auditor_retrieve_payloads_indexed")
        return out

    def retrieve_payloads_indexed_len(self, pay_cts, all_payloads_count: int, layout: "PayloadLayout", seed: bytes,
                                      indices, bits: int = 0) -> np.ndarray:
        """omr_auditor_retrieve_payloads_indexed_len: u16 [len(indices)][layout.payload_len], the right-hand side
        gathered across the stripes and the solve on the device."""
        c = self._cts(pay_cts, bits)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        out = np.zeros((len(idx), layout.payload_len if layout else 0), np.uint16)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_auditor_retrieve_payloads_indexed_len(self._h, c.ctypes.data, c.shape[0], bits,
                                                               all_payloads_count, _layout_ref(layout), ptr,
                                                               idx.ctypes.data, len(idx), out.ctypes.data),
               "omr_auditor_retrieve_payloads_indexed_len")
        return out

    def retrieve_payloads_seek(self, pay_cts, all_payloads_count: int, combination_count: int, seed: bytes, indices,
                               seek: "WeightSeek" = None, bits: int = 0) -> np.ndarray:
        """omr_auditor_retrieve_payloads_seek: the same with the reference's weights found through the seek
        (None: built on the auditor's device inside the call); the bits of retrieve_payloads given the table."""
        c = self._cts(pay_cts, bits)
        idx = np.ascontiguousarray(sorted(indices), dtype=np.uintp)
        out = np.zeros((len(idx), PAYLOAD_LENGTH), np.uint16)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_auditor_retrieve_payloads_seek(self._h, c.ctypes.data, c.shape[0], bits, all_payloads_count,
                                                        combination_count, ptr, _seek_ptr(seek), idx.ctypes.data,
                                                        len(idx), out.ctypes.data), "omr_auditor_retrieve_payloads_seek")
        return out

    def decode_digest(self, idx_cts, pay_cts, seed: bytes, all_payloads_count: int, pertinent_count: int, bits: int = 0,
                      cap: int = None):
        """omr_auditor_decode_digest_indexed: Retriever.decode_digest(indexed=True) in one call on the device:
        (sorted indices, payloads u16 [found][612], summary dict of every ciphertext decoded)."""
        ci, cp = self._cts(idx_cts, bits), self._cts(pay_cts, bits)
        cap = max(1, pertinent_count) * 4 + 64 if cap is None else cap
        idx = np.zeros(max(1, cap), dtype=np.uintp)
        out = np.zeros((max(1, cap), PAYLOAD_LENGTH), np.uint16)
        found, t = C.c_size_t(), _AuditSummary()
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_auditor_decode_digest_indexed(self._h, ci.ctypes.data, ci.shape[0], cp.ctypes.data, cp.shape[0],
                                                       bits, all_payloads_count, pertinent_count, ptr, idx.ctypes.data,
                                                       cap, C.byref(found), out.ctypes.data, C.addressof(t)),
               "omr_auditor_decode_digest_indexed")
        return [int(v) for v in idx[:found.value]], out[:found.value].copy(), _summary_dict(t)

    @staticmethod
    def summary_from_bytes(buf) -> dict:
        """The dict form of an omr_audit_summary copied back from the device (440 bytes)."""
        return _summary_dict(_AuditSummary.from_buffer_copy(bytes(buf)))

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


# Contexts still open at interpreter exit are destroyed by an atexit hook, which runs before the
# HIP runtime's own exit-time teardown (a context freed after it faults, e.g. under rocprofv3).
_LIVE_DETECTORS: "weakref.WeakSet[Detector]" = weakref.WeakSet()
_destroy_ctx = None  # omr_ctx_destroy, bound by the first Detector (usable at interpreter shutdown)


def _bind_destroy():
    global _destroy_ctx
    if _destroy_ctx is None:
        _destroy_ctx = lib().omr_ctx_destroy


@atexit.register
def _close_live_detectors():
    for d in list(_LIVE_DETECTORS):
        d.close()


class Detector:
    """Detector (detector.rs:35-453) on one MI355X."""

    def __init__(self, detection_key: DetectionKey, device: int = 0):
        view = _KeyView(detection_key.bsk1.ctypes.data, detection_key.ksk.ctypes.data,
                        detection_key.bsk2.ctypes.data, detection_key.trace_key.ctypes.data)
        for a, shape, dt in ((detection_key.bsk1, BSK1_SHAPE, np.uint32), (detection_key.ksk, KSK_SHAPE, np.uint32),
                             (detection_key.bsk2, BSK2_SHAPE, np.uint64), (detection_key.trace_key, TK_SHAPE, np.uint64)):
            if a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise OmrError(f"detection key component has shape {a.shape} {a.dtype}, expected {shape} {dt}")
        h = C.c_void_p()
        _check(lib().omr_ctx_create(C.byref(view), device, C.byref(h)), "omr_ctx_create")
        self._h = h
        self.device = device
        _bind_destroy()
        _LIVE_DETECTORS.add(self)

    @classmethod
    def from_device_key(cls, d_bsk1: int, d_ksk: int, d_bsk2: int, d_trace_key: int, device: int = 0):
        """Detector over key components already in the HBM of `device` (device pointers, ABI
        layout), e.g. from SecretKeyPack.generate_detection_key_device."""
        self = cls.__new__(cls)
        view = _KeyView(d_bsk1, d_ksk, d_bsk2, d_trace_key)
        h = C.c_void_p()
        _check(lib().omr_ctx_create(C.byref(view), device, C.byref(h)), "omr_ctx_create")
        self._h = h
        self.device = device
        _bind_destroy()
        _LIVE_DETECTORS.add(self)
        return self

    @classmethod
    def from_seeded_key(cls, key, device: int = 0, mask_seed: int = 0):
        """Detector from a seeded key (omr_ctx_create_seeded): a SeededKey with host bodies, or four raw
        pointers (bsk1_b, ksk_b, bsk2_b, trace_key_b; host memory or HBM of `device`) and the mask_seed.
        The key is expanded on the device; the expanded copy is freed before this returns."""
        self = cls.__new__(cls)
        view = key._view() if isinstance(key, SeededKey) else _SeededKeyView(*key, mask_seed)
        h = C.c_void_p()
        _check(lib().omr_ctx_create_seeded(C.byref(view), device, C.byref(h)), "omr_ctx_create_seeded")
        self._h = h
        self.device = device
        _bind_destroy()
        _LIVE_DETECTORS.add(self)
        return self

    def close(self):
        if getattr(self, "_h", None):
            for dg in list(getattr(self, "_sessions", ())):  # a session must go before its context
                dg.close()
            (_destroy_ctx or lib().omr_ctx_destroy)(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def handle(self):
        return self._h

    def set_batch(self, batch: int):
        _check(lib().omr_ctx_set_batch(self._h, batch), "omr_ctx_set_batch")

    def set_encode_chunks(self, max_chunks: int):
        """At most max_chunks partial digests per encode ciphertext (0 = default 4,096)."""
        _check(lib().omr_ctx_set_encode_chunks(self._h, max_chunks), "omr_ctx_set_encode_chunks")

    def set_latency_threshold(self, max_messages: int):
        """Chunks of at most max_messages messages use the latency kernels (0: never)."""
        _check(lib().omr_ctx_set_latency_threshold(self._h, max_messages), "omr_ctx_set_latency_threshold")

    def set_exact_level1(self, enable: bool = True):
        """Level 1 on the exact modular NTT for every launch (omr_ctx_set_exact_level1: the
        reference's arithmetic, bit-identical outputs, slower); False restores the FFT kernels."""
        _check(lib().omr_ctx_set_exact_level1(self._h, 1 if enable else 0), "omr_ctx_set_exact_level1")

    # detect (detector.rs:135) — one clue set -> NttRlweCiphertext [2][2048]
    def detect(self, clue_a, clue_b) -> np.ndarray:
        """One message (omr_detect): thread-safe; concurrent callers are coalesced into batched
        launches (ctypes releases the GIL during the call)."""
        a = np.ascontiguousarray(clue_a, dtype=np.uint16).reshape(N0)
        b = np.ascontiguousarray(clue_b, dtype=np.uint16).reshape(CLUE_COUNT)
        out = np.empty((2, N2), np.uint64)
        _check(lib().omr_detect(self._h, a, b, out.reshape(-1)), "omr_detect")
        return out

    def set_coalescing(self, max_messages: int = 0, window_us: int = 0):
        _check(lib().omr_ctx_set_coalescing(self._h, int(max_messages), int(window_us)), "omr_ctx_set_coalescing")

    def coalescing_stats(self) -> tuple:
        calls, launches = C.c_size_t(), C.c_size_t()
        _check(lib().omr_ctx_coalescing_stats(self._h, C.byref(calls), C.byref(launches)), "omr_ctx_coalescing_stats")
        return calls.value, launches.value

    def detect_batch(self, clue_a, clue_b) -> np.ndarray:
        clue_a = np.ascontiguousarray(clue_a, dtype=np.uint16)
        clue_b = np.ascontiguousarray(clue_b, dtype=np.uint16)
        D = clue_a.shape[0]
        if clue_a.shape != (D, N0) or clue_b.shape != (D, CLUE_COUNT):
            raise OmrError("clues must be u16 [D][512] and [D][7]")
        out = np.empty((D, 2, N2), np.uint64)
        _check(lib().omr_detect_batch(self._h, clue_a.reshape(-1), clue_b.reshape(-1), D, out.reshape(-1)),
               "omr_detect_batch")
        return out

    def detect_batch_device(self, d_clue_a: int, d_clue_b: int, D: int, d_out: int, stream: int = 0):
        _check(lib().omr_detect_batch_device(self._h, d_clue_a, d_clue_b, D, d_out, stream or None),
               "omr_detect_batch_device")

    def check(self, stream: int = 0):
        """omr_ctx_check: sync `stream` (0: the whole device) and raise if an earlier call's device
        work failed."""
        _check(lib().omr_ctx_check(self._h, stream or None), "omr_ctx_check")

    def set_rounding_guard(self, enable: bool = True):
        """Run the guarded FFT kernel variants (same output) that record the rounding margin."""
        _check(lib().omr_ctx_set_rounding_guard(self._h, int(bool(enable))), "omr_ctx_set_rounding_guard")

    def rounding_margin(self, reset: bool = False) -> dict:
        """{"observed": [level1, level2] largest |y - rint(y)| of the guarded runs so far,
        "apriori": [E1, E2] proven bounds on |computed - exact|, "kappa": key-spectrum maxima}."""
        obs, apr, kap = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
        _check(lib().omr_ctx_rounding_margin(self._h, obs, apr, kap, int(bool(reset))), "omr_ctx_rounding_margin")
        return {"observed": list(obs), "apriori": list(apr), "kappa": list(kap)}

    def exactness(self) -> dict:
        """The exactness contract (omr_ctx_exactness): {"guarded": [l1, l2] guarded on every launch
        (automatically when the key's a priori bound E >= 0.5), "breaches": [l1, l2] launches whose
        margin reached 1 - E (each such launch re-run on the exact NTT)}."""
        g, b = (C.c_int * 2)(), (C.c_uint64 * 2)()
        _check(lib().omr_ctx_exactness(self._h, g, b), "omr_ctx_exactness")
        return {"guarded": [bool(v) for v in g], "breaches": list(b)}

    def launch_record(self) -> dict:
        """Cumulative launches per level-2 rotation / trace kernel since creation (omr_ctx_launch_record):
        LAUNCH_KINDS name -> count. Host counters; compare two reads."""
        counts = (C.c_uint64 * len(LAUNCH_KINDS))()
        _check(lib().omr_ctx_launch_record(self._h, counts), "omr_ctx_launch_record")
        return dict(zip(LAUNCH_KINDS, (int(v) for v in counts)))

    def key_spectrum(self, level: int, first: int, count: int) -> np.ndarray:
        """Stored key-spectrum values [count] complex (omr_ctx_key_spectrum)."""
        out = np.zeros(2 * count, dtype=np.float64)
        _check(lib().omr_ctx_key_spectrum(self._h, int(level), int(first), int(count), out), "omr_ctx_key_spectrum")
        return out.view(np.complex128)

    def enable_timing(self, mode: int = 1):
        """0 off; 1 and 2 are the same, stage events around the production kernels (the trace is
        always its own launch, so trace_separate is always 1)."""
        _check(lib().omr_ctx_enable_timing(self._h, int(mode)), "omr_ctx_enable_timing")

    def last_timing(self) -> dict:
        t = _Timing()
        _check(lib().omr_last_timing(self._h, C.byref(t)), "omr_last_timing")
        return {n: getattr(t, n) for n, _ in _Timing._fields_}

    # detect_with_time_info (detector.rs:169-221): DetectTimeInfo of one batch (device time),
    # detect + timing in one locked call
    def detect_with_time_info(self, clue_a, clue_b):
        clue_a = np.ascontiguousarray(clue_a, dtype=np.uint16)
        clue_b = np.ascontiguousarray(clue_b, dtype=np.uint16)
        D = clue_a.shape[0]
        if clue_a.shape != (D, N0) or clue_b.shape != (D, CLUE_COUNT):
            raise OmrError("clues must be u16 [D][512] and [D][7]")
        out = np.empty((D, 2, N2), np.uint64)
        t = _Timing()
        _check(lib().omr_detect_with_time_info(self._h, clue_a.reshape(-1), clue_b.reshape(-1), D, out.reshape(-1),
                                               C.byref(t)), "omr_detect_with_time_info")
        return out, {n: getattr(t, n) for n, _ in _Timing._fields_}

    # encode_pertinent_indices (detector.rs:223-339)
    def encode_pertinent_indices(self, rp: RetrievalParams, pertinency_vector, seed: int, ct: int = 0,
                                 global_offset: int = 0) -> np.ndarray:
        pv = np.ascontiguousarray(pertinency_vector, dtype=np.uint64)
        D = pv.shape[0]
        out = np.empty((2, N2), np.uint64)
        _check(lib().omr_encode_indices(self._h, pv.reshape(-1), D, global_offset, rp.all_payloads_count, seed, ct,
                                        out.reshape(-1)), "omr_encode_indices")
        return out

    # encode_pertinent_payloads (detector.rs:341-453)
    def encode_pertinent_payloads(self, pertinency_vector, payloads, weights, rp: RetrievalParams,
                                  global_offset: int = 0) -> np.ndarray:
        pv = np.ascontiguousarray(pertinency_vector, dtype=np.uint64)
        pay = np.ascontiguousarray(payloads, dtype=np.uint16)
        w = np.ascontiguousarray(weights, dtype=np.uint16)
        D = pv.shape[0]
        n_ct, per = rp.cmb_cipher_count, rp.cmb_count_per_cipher
        out = np.empty((n_ct, 2, N2), np.uint64)
        _check(lib().omr_encode_payloads(self._h, pv.reshape(-1), pay.reshape(-1), D, global_offset,
                                         rp.all_payloads_count, w, n_ct, per, out.reshape(-1)), "omr_encode_payloads")
        return out

    def encode_pertinent_payloads_indexed(self, pertinency_vector, payloads, seed: bytes, rp: RetrievalParams,
                                          global_offset: int = 0, first_ct: int = 0, n_ct: int = None) -> np.ndarray:
        """omr_encode_payloads_indexed: encode_pertinent_payloads with indexed weights (no table), the
        ciphertexts [first_ct, first_ct + n_ct) of the digest (default: all of rp's)."""
        pv = np.ascontiguousarray(pertinency_vector, dtype=np.uint64)
        pay = np.ascontiguousarray(payloads, dtype=np.uint16)
        D = pv.shape[0]
        n = rp.cmb_cipher_count - first_ct if n_ct is None else n_ct
        out = np.empty((max(n, 0), 2, N2), np.uint64)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_encode_payloads_indexed(self._h, pv.ctypes.data, pay.ctypes.data, D, global_offset,
                                                 rp.all_payloads_count, ptr, rp.combination_count, first_ct, n,
                                                 rp.cmb_count_per_cipher, out.ctypes.data),
               "omr_encode_payloads_indexed")
        return out

    def encode_bitmap(self, pertinency_vector, all_payloads_count: int, global_offset: int = 0) -> np.ndarray:
        """omr_encode_bitmap (none in the reference): the board's bitmap digest u64
        [bitmap_ct_count(all)][2][2048] over the messages global_offset.. of the pertinency vector."""
        pv = np.ascontiguousarray(pertinency_vector, dtype=np.uint64).reshape(-1, 2, N2)
        out = np.empty((bitmap_ct_count(all_payloads_count), 2, N2), np.uint64)
        _check(lib().omr_encode_bitmap(self._h, pv.reshape(-1), pv.shape[0], global_offset, all_payloads_count,
                                       out.reshape(-1)), "omr_encode_bitmap")
        return out

    # device-pointer variants (chaining on the caller's HIP stream; pointers are raw addresses)
    def encode_bitmap_device(self, d_pv: int, D: int, global_offset: int, all_payloads_count: int, d_out: int,
                             stream: int = 0) -> None:
        _check(lib().omr_encode_bitmap_device(self._h, d_pv or None, D, global_offset, all_payloads_count, d_out,
                                              stream or None), "omr_encode_bitmap_device")

    def encode_indices_device(self, d_pv: int, D: int, global_offset: int, all_payloads_count: int, seed: int,
                              first_ct: int, n_ct: int, d_out: int, stream: int = 0) -> None:
        _check(lib().omr_encode_indices_device(self._h, d_pv, D, global_offset, all_payloads_count, seed, first_ct,
                                               n_ct, d_out, stream or None), "omr_encode_indices_device")

    def encode_payloads_device(self, d_pv: int, d_payloads: int, D: int, global_offset: int,
                               all_payloads_count: int, d_weights: int, n_ct: int, per_ct: int, d_out: int,
                               stream: int = 0) -> None:
        _check(lib().omr_encode_payloads_device(self._h, d_pv, d_payloads, D, global_offset, all_payloads_count,
                                                d_weights, n_ct, per_ct, d_out, stream or None),
               "omr_encode_payloads_device")

    def encode_pertinent_payloads_indexed_device(self, d_pv: int, d_payloads: int, D: int, global_offset: int,
                                                 all_payloads_count: int, seed: bytes, combination_count: int,
                                                 first_ct: int, n_ct: int, per_ct: int, d_out: int,
                                                 stream: int = 0) -> None:
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_encode_payloads_indexed_device(self._h, d_pv or None, d_payloads or None, D, global_offset,
                                                        all_payloads_count, ptr, combination_count, first_ct, n_ct,
                                                        per_ct, d_out or None, stream or None),
               "omr_encode_payloads_indexed_device")

    def encode_pertinent_payloads_indexed_len(self, pertinency_vector, payloads, seed: bytes, all_payloads_count: int,
                                              combination_count: int, per_ct: int, first_ct: int, n_ct: int,
                                              global_offset: int = 0, payload_len: int = None) -> np.ndarray:
        """omr_encode_payloads_indexed_len: payloads u16 [D][payload_len] (default: the array's width), the
        ciphertexts [first_ct, first_ct + n_ct) of the length's layout at per_ct combinations per group."""
        pv = np.ascontiguousarray(pertinency_vector, dtype=np.uint64)
        pay = np.ascontiguousarray(payloads, dtype=np.uint16)
        L = pay.shape[1] if payload_len is None else payload_len
        out = np.empty((min(max(n_ct, 0), 65535), 2, N2), np.uint64)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_encode_payloads_indexed_len(self._h, pv.ctypes.data, pay.ctypes.data, pv.shape[0],
                                                     global_offset, all_payloads_count, ptr, combination_count, L,
                                                     per_ct, first_ct, n_ct, out.ctypes.data),
               "omr_encode_payloads_indexed_len")
        return out

    def encode_pertinent_payloads_indexed_len_device(self, d_pv: int, d_payloads: int, D: int, global_offset: int,
                                                     all_payloads_count: int, seed: bytes, combination_count: int,
                                                     payload_len: int, per_ct: int, first_ct: int, n_ct: int,
                                                     d_out: int, stream: int = 0) -> None:
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_encode_payloads_indexed_len_device(self._h, d_pv or None, d_payloads or None, D,
                                                            global_offset, all_payloads_count, ptr, combination_count,
                                                            payload_len, per_ct, first_ct, n_ct, d_out or None,
                                                            stream or None),
               "omr_encode_payloads_indexed_len_device")

    def encode_pertinent_payloads_seek(self, pertinency_vector, payloads, seed: bytes, seek: "WeightSeek",
                                       rp: RetrievalParams, global_offset: int = 0, first_ct: int = 0,
                                       n_ct: int = None) -> np.ndarray:
        """omr_encode_payloads_seek: encode_pertinent_payloads' bits without its table, the reference's
        weights found through the seek; the ciphertexts [first_ct, first_ct + n_ct) (default: all of rp's)."""
        pv = np.ascontiguousarray(pertinency_vector, dtype=np.uint64)
        pay = np.ascontiguousarray(payloads, dtype=np.uint16)
        n = rp.cmb_cipher_count - first_ct if n_ct is None else n_ct
        out = np.empty((max(n, 0), 2, N2), np.uint64)
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_encode_payloads_seek(self._h, pv.ctypes.data, pay.ctypes.data, pv.shape[0], global_offset,
                                              rp.all_payloads_count, ptr, _seek_ptr(seek), rp.combination_count,
                                              first_ct, n, rp.cmb_count_per_cipher, out.ctypes.data),
               "omr_encode_payloads_seek")
        return out

    def encode_pertinent_payloads_seek_device(self, d_pv: int, d_payloads: int, D: int, global_offset: int,
                                              all_payloads_count: int, seed: bytes, seek: "WeightSeek",
                                              combination_count: int, first_ct: int, n_ct: int, per_ct: int,
                                              d_out: int, stream: int = 0) -> None:
        ptr, _keep = _seed_ptr(seed)
        _check(lib().omr_encode_payloads_seek_device(self._h, d_pv or None, d_payloads or None, D, global_offset,
                                                     all_payloads_count, ptr, _seek_ptr(seek), combination_count,
                                                     first_ct, n_ct, per_ct, d_out or None, stream or None),
               "omr_encode_payloads_seek_device")

    # compact ciphertexts (include/omr_gpu.h, "Compact ciphertexts"): the server side
    def compact_cts(self, cts, bits: int) -> np.ndarray:
        """omr_compact_cts: host NttRlweCiphertexts u64 [n][2][2048] -> u8 [n][512 * bits] through the device."""
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2, N2)
        out = np.empty((cts.shape[0], compact_ct_bytes(bits)), np.uint8)
        _check(lib().omr_compact_cts(self._h, cts.ctypes.data, cts.shape[0], bits, out.ctypes.data), "omr_compact_cts")
        return out

    def compact_cts_device(self, d_cts: int, n: int, bits: int, d_out: int, stream: int = 0) -> None:
        """omr_compact_cts_device: device pointers, enqueued on `stream`; the caller synchronises."""
        _check(lib().omr_compact_cts_device(self._h, d_cts or None, n, bits, d_out or None, stream or None),
               "omr_compact_cts_device")

    def set_compact_grid(self, workgroups: int = 0):
        _check(lib().omr_ctx_set_compact_grid(self._h, workgroups), "omr_ctx_set_compact_grid")

    def set_compact_staging(self, max_ciphertexts: int = 0):
        _check(lib().omr_ctx_set_compact_staging(self._h, max_ciphertexts), "omr_ctx_set_compact_staging")

    def digest_session(self, all_payloads_count: int, pertinent_count: int, index_seed: int, weight_seed: bytes,
                       stream: int = 0, indexed: bool = False, seek: bool = False,
                       payload_len: int = None) -> "DigestSession":
        """A digest session on this detector (omr_digest_begin): detect + encode a board piece by
        piece without holding its pertinency vector. A context manager. indexed=True: a session with
        indexed payload weights (omr_digest_begin_indexed), which holds no weight table. seek=True: the
        reference's weights without the table (omr_digest_begin_seek): the digest of the default session.
        payload_len=L (with indexed=True): a board whose payloads are L words long (omr_digest_begin_indexed_len)."""
        return DigestSession(self, all_payloads_count, pertinent_count, index_seed, weight_seed, stream, indexed, seek,
                             payload_len)

    # ---- stage entry points (benches/two_level_bs.rs) ----
    def first_level(self, clue_a, clue_b) -> np.ndarray:
        clue_a = np.ascontiguousarray(clue_a, dtype=np.uint16).reshape(-1, N0)
        clue_b = np.ascontiguousarray(clue_b, dtype=np.uint16).reshape(-1, CLUE_COUNT)
        out = np.empty((clue_a.shape[0], NI + 1), np.uint32)
        _check(lib().omr_first_level(self._h, clue_a.reshape(-1), clue_b.reshape(-1), clue_a.shape[0],
                                     out.reshape(-1)), "omr_first_level")
        return out

    def sum_key_switch(self, ext) -> np.ndarray:
        """The first level after its rotations on supplied extracted LWEs (u32 [n][7][1025], canonical): sum
        of the seven, key switch, modulus switch, body offset; u32 [n][671] (omr_sum_key_switch)."""
        ext = np.ascontiguousarray(ext, dtype=np.uint32).reshape(-1, CLUE_COUNT, N1 + 1)
        out = np.empty((ext.shape[0], NI + 1), np.uint32)
        _check(lib().omr_sum_key_switch(self._h, ext.ctypes.data, ext.shape[0], out.ctypes.data),
               "omr_sum_key_switch")
        return out

    def blind_rotate_level1(self, lwe_a, lwe_b=None, acc0=None) -> np.ndarray:
        """acc0 (u64 [n][2][1024], canonical): the initial accumulators instead of (0, X^-b LUT1); lwe_b is
        then ignored (omr_blind_rotate_level1_from)."""
        lwe_a = np.ascontiguousarray(lwe_a, dtype=np.uint16).reshape(-1, N0)
        out = np.empty((lwe_a.shape[0], 2, N1), np.uint64)
        if acc0 is not None:
            acc0 = np.ascontiguousarray(acc0, dtype=np.uint64).reshape(lwe_a.shape[0], 2, N1)
            _check(lib().omr_blind_rotate_level1_from(self._h, lwe_a.reshape(-1), None, lwe_a.shape[0],
                                                      acc0.ctypes.data, out.ctypes.data),
                   "omr_blind_rotate_level1_from")
            return out
        lwe_b = np.ascontiguousarray(lwe_b, dtype=np.uint16).reshape(-1)
        _check(lib().omr_blind_rotate_level1(self._h, lwe_a.reshape(-1), lwe_b, lwe_a.shape[0], out.reshape(-1)),
               "omr_blind_rotate_level1")
        return out

    def fft1_mul(self, a, k) -> np.ndarray:
        """a * k mod (X^1024 + 1, q1) through the level-1 FFT path (a digit-sized)."""
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, N1)
        k = np.ascontiguousarray(k, dtype=np.uint32).reshape(-1, N1)
        out = np.empty(a.shape, np.uint64)
        _check(lib().omr_fft1_mul(self._h, a.reshape(-1), k.reshape(-1), a.shape[0], out.reshape(-1)),
               "omr_fft1_mul")
        return out

    def second_level(self, lwe_int) -> np.ndarray:
        lwe = np.ascontiguousarray(lwe_int, dtype=np.uint32).reshape(-1, NI + 1)
        out = np.empty((lwe.shape[0], 2, N2), np.uint64)
        _check(lib().omr_second_level(self._h, lwe.reshape(-1), lwe.shape[0], out.reshape(-1)), "omr_second_level")
        return out

    def blind_rotate_level2(self, lwe_int, acc0=None) -> np.ndarray:
        """acc0 (u64 [n][2][2048], canonical): the initial accumulators instead of (0, X^-b LUT2); the LWE
        bodies are then ignored (omr_blind_rotate_level2_from)."""
        lwe = np.ascontiguousarray(lwe_int, dtype=np.uint32).reshape(-1, NI + 1)
        out = np.empty((lwe.shape[0], 2, N2), np.uint64)
        if acc0 is not None:
            acc0 = np.ascontiguousarray(acc0, dtype=np.uint64).reshape(lwe.shape[0], 2, N2)
            _check(lib().omr_blind_rotate_level2_from(self._h, lwe.reshape(-1), lwe.shape[0], acc0.ctypes.data,
                                                      out.ctypes.data), "omr_blind_rotate_level2_from")
            return out
        _check(lib().omr_blind_rotate_level2(self._h, lwe.reshape(-1), lwe.shape[0], out.reshape(-1)),
               "omr_blind_rotate_level2")
        return out

    def trace(self, rlwe) -> np.ndarray:
        """The homomorphic trace alone on coefficient-domain RLWEs (u64 [n][2][2048], canonical): what
        second_level runs after its rotation; NTT-domain output (omr_trace)."""
        rlwe = np.ascontiguousarray(rlwe, dtype=np.uint64).reshape(-1, 2, N2)
        out = np.empty(rlwe.shape, np.uint64)
        _check(lib().omr_trace(self._h, rlwe.ctypes.data, rlwe.shape[0], out.ctypes.data), "omr_trace")
        return out


class DigestSession:
    """omr_digest_*: the board flow of examples/omr.rs:160-203 (detect, encode_pertinent_indices,
    encode_pertinent_payloads) over message ranges fed in any order; the running digest stays on the
    device and at most one detect chunk of pertinency ciphertexts is ever allocated."""

    def __init__(self, detector: "Detector", all_payloads_count: int, pertinent_count: int, index_seed: int,
                 weight_seed: bytes, stream: int = 0, indexed: bool = False, seek: bool = False,
                 payload_len: int = None):
        seed = np.frombuffer(bytes(weight_seed), dtype=np.uint8).copy()
        if seed.size != 32:
            raise OmrError("weight_seed must be 32 bytes")
        h = C.c_void_p()
        if indexed and seek:
            raise OmrError("a session uses indexed weights or the reference's weights by seek, not both")
        if payload_len is not None and not indexed:
            raise OmrError("a payload length of its own needs indexed weights")
        begin, what = ((lib().omr_digest_begin_indexed, "omr_digest_begin_indexed") if indexed else
                       (lib().omr_digest_begin_seek, "omr_digest_begin_seek") if seek else
                       (lib().omr_digest_begin, "omr_digest_begin"))
        if payload_len is not None:
            _check(lib().omr_digest_begin_indexed_len(detector.handle, all_payloads_count, pertinent_count, index_seed,
                                                      seed.ctypes.data, payload_len, stream or None, C.byref(h)),
                   "omr_digest_begin_indexed_len")
        else:
            _check(begin(detector.handle, all_payloads_count, pertinent_count, index_seed, seed.ctypes.data,
                         stream or None, C.byref(h)), what)
        self._h = h
        self._destroy = lib().omr_digest_destroy
        self._detector = detector  # the context outlives the session
        if not hasattr(detector, "_sessions"):
            detector._sessions = weakref.WeakSet()
        detector._sessions.add(self)
        self._info = self.info()
        self._len = self.payload_layout().payload_len

    def update(self, clue_a, clue_b, payloads, global_offset: int = 0) -> None:
        """Host arrays u16 [D][512], [D][7], [D][payload_len] (612 unless the session was begun with a
        payload_len of its own) for global indices global_offset..+D; returns when the device has finished
        with them."""
        a = np.ascontiguousarray(clue_a, dtype=np.uint16)
        b = np.ascontiguousarray(clue_b, dtype=np.uint16)
        p = np.ascontiguousarray(payloads, dtype=np.uint16)
        D = a.shape[0]
        if a.shape != (D, N0) or b.shape != (D, CLUE_COUNT) or p.shape != (D, self._len):
            raise OmrError(f"clues must be u16 [D][512] and [D][7], payloads u16 [D][{self._len}]")
        _check(lib().omr_digest_update(self._h, a.reshape(-1), b.reshape(-1), p.reshape(-1), D, global_offset),
               "omr_digest_update")

    def update_device(self, d_clue_a: int, d_clue_b: int, d_payloads: int, D: int, global_offset: int = 0) -> None:
        """Device pointers (same layouts, the payloads [D][payload_len] of the session); enqueued on the session's stream, the caller keeps the
        buffers alive until read() or Detector.check()."""
        _check(lib().omr_digest_update_device(self._h, d_clue_a, d_clue_b, d_payloads, D, global_offset),
               "omr_digest_update_device")

    def merge(self, idx_cts, pay_cts) -> None:
        """Add another session's read() output (e.g. another GPU's shard) mod q2."""
        i = None if idx_cts is None else np.ascontiguousarray(idx_cts, dtype=np.uint64)
        p = None if pay_cts is None else np.ascontiguousarray(pay_cts, dtype=np.uint64)
        if (i is not None and i.size != self._info["index_ct"] * 2 * N2) or \
                (p is not None and p.size != self._info["payload_ct"] * 2 * N2):
            raise OmrError("digest arrays must be u64 [index_ct][2][2048] and [payload_ct][2][2048]")
        _check(lib().omr_digest_merge(self._h, None if i is None else i.ctypes.data,
                                      None if p is None else p.ctypes.data), "omr_digest_merge")

    def read(self):
        """(idx_cts u64 [index_ct][2][2048], pay_cts u64 [payload_ct][2][2048]) after a stream sync."""
        idx = np.empty((self._info["index_ct"], 2, N2), np.uint64)
        pay = np.empty((self._info["payload_ct"], 2, N2), np.uint64)
        _check(lib().omr_digest_read(self._h, idx.ctypes.data, pay.ctypes.data), "omr_digest_read")
        return idx, pay

    def read_compact(self, bits: int, bitmap: bool = False):
        """omr_digest_read_compact: the digest at `bits` bits per coefficient, (idx u8 [index_ct][512 * bits],
        pay u8 [payload_ct][512 * bits]) and, with bitmap=True, the bitmap digest the same way as a third
        array. The running digest is not modified."""
        ctb = compact_ct_bytes(bits)
        idx = np.empty((self._info["index_ct"], ctb), np.uint8)
        pay = np.empty((self._info["payload_ct"], ctb), np.uint8)
        bmp = np.empty((bitmap_ct_count(self._info["all_payloads_count"]), ctb), np.uint8) if bitmap else None
        _check(lib().omr_digest_read_compact(self._h, bits, idx.ctypes.data, pay.ctypes.data,
                                             bmp.ctypes.data if bitmap else None), "omr_digest_read_compact")
        return (idx, pay, bmp) if bitmap else (idx, pay)

    def enable_bitmap(self) -> None:
        """omr_digest_enable_bitmap: also keep the board's bitmap digest; before the first update or merge."""
        _check(lib().omr_digest_enable_bitmap(self._h), "omr_digest_enable_bitmap")

    def read_bitmap(self) -> np.ndarray:
        """The bitmap digest u64 [bitmap_ct_count(all)][2][2048] after a stream sync."""
        out = np.empty((bitmap_ct_count(self._info["all_payloads_count"]), 2, N2), np.uint64)
        _check(lib().omr_digest_read_bitmap(self._h, out.ctypes.data), "omr_digest_read_bitmap")
        return out

    def merge_bitmap(self, bitmap_cts) -> None:
        """Add another session's read_bitmap() output mod q2."""
        b = np.ascontiguousarray(bitmap_cts, dtype=np.uint64)
        if b.size != bitmap_ct_count(self._info["all_payloads_count"]) * 2 * N2:
            raise OmrError("bitmap array must be u64 [bitmap_ct_count(all)][2][2048]")
        _check(lib().omr_digest_merge_bitmap(self._h, b.ctypes.data), "omr_digest_merge_bitmap")

    def info(self) -> dict:
        t = _DigestInfo()
        _check(lib().omr_digest_get_info(self._h, C.byref(t)), "omr_digest_get_info")
        return {n: getattr(t, n) for n, _ in _DigestInfo._fields_}

    def payload_layout(self) -> "PayloadLayout":
        """omr_digest_get_payload_layout: the layout of the session's payload digest."""
        t = _PayloadLayout()
        _check(lib().omr_digest_get_payload_layout(self._h, C.byref(t)), "omr_digest_get_payload_layout")
        return PayloadLayout(**{n: getattr(t, n) for n, _ in _PayloadLayout._fields_})

    def device_bytes(self) -> dict:
        """omr_digest_device_bytes: the device memory the session owns now, and the weights' share of it."""
        total, weights = C.c_size_t(), C.c_size_t()
        _check(lib().omr_digest_device_bytes(self._h, C.byref(total), C.byref(weights)), "omr_digest_device_bytes")
        return {"total": total.value, "weights": weights.value}

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def ntt(level: int, polys, inverse: bool = False, device: int = 0) -> np.ndarray:
    p = np.array(polys, dtype=np.uint64, copy=True)
    n = (1024 if level == 1 else 2048)
    p2 = p.reshape(-1, n)
    flat = np.ascontiguousarray(p2).reshape(-1)
    _check(lib().omr_ntt(level, int(inverse), flat, p2.shape[0], device), "omr_ntt")
    return flat.reshape(p.shape)


class KeyGen:
    """KeyGen::generate_secret_key (key_gen/mod.rs:21-27)."""

    @staticmethod
    def generate_secret_key(seed: int) -> SecretKeyPack:
        return SecretKeyPack(seed)
