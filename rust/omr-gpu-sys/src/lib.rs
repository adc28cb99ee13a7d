//! `omr-gpu-sys` — thin FFI crate over `libomr_gpu.so`, the MI355X-native InstantOMR detector.
//!
//! [`ffi`] declares every entry point of `include/omr_gpu.h` (the C ABI); the safe layer mirrors
//! the `omr_core` API surface the detect path exposes (`omr_core/src/lib.rs:28-31`):
//! [`GpuDetector`] for `Detector` (`detector.rs:85-110` `new`, `:135-138` `detect`, `:169-175`
//! `detect_with_time_info`, `:223-227` `encode_pertinent_indices`, `:341-350`
//! `encode_pertinent_payloads`), [`SecretKeyPack`] for `KeyGen::generate_secret_key` /
//! `SecretKeyPack` (`key_gen/secret.rs:46-209`) with seeded streams, [`RetrievalParams`]
//! (`parameters/retrieval_params.rs:50-106`) and [`Retriever`] (`retriever.rs:188-260`).
//! [`Auditor`] decrypts, classifies and noise-audits ciphertexts on the device (the counterpart of
//! `NoiseSigmaInfo`, `retriever.rs:390-560`).
//! [`DigestSession`] runs the whole board flow (`examples/omr.rs:160-203`) inside the library
//! without a pertinency vector on the caller's side.
//!
//! Differences a caller sees, all forced by determinism across GPUs and shards: keys, clues and
//! the bucket choices of `encode_pertinent_indices` come from seeded counter-based streams (the
//! reference draws from `thread_rng`), so those calls take a seed; `encode_pertinent_payloads`
//! takes the 32-byte seed the reference passes to `StdRng::from_seed` (`examples/omr.rs:197-203`)
//! and draws the same weights (`detector.rs:376-387`). `detect_batch` replaces
//! `clues.par_iter().map(|c| detector.detect(c))` (`examples/omr.rs:160-164`).
//!
//! The crate has no dependencies; `build.rs` links `libomr_gpu.so` and the HIP runtime.

use std::ffi::CStr;
use std::fmt;
use std::os::raw::{c_char, c_int, c_long, c_uint, c_void};
use std::time::Duration;

/// Raw bindings of `include/omr_gpu.h`, one declaration per C entry point.
pub mod ffi {
    use super::*;

    pub type OmrStatus = c_int;
    pub const OMR_OK: OmrStatus = 0;
    pub const OMR_ERR_INVALID_ARGUMENT: OmrStatus = 1;
    pub const OMR_ERR_DEVICE: OmrStatus = 2;
    pub const OMR_ERR_OUT_OF_MEMORY: OmrStatus = 3;
    pub const OMR_ERR_NOT_INVERTIBLE: OmrStatus = 4;

    pub const OMR_N0: usize = 512;
    pub const OMR_Q0: u32 = 2048;
    pub const OMR_CLUE_COUNT: usize = 7;
    pub const OMR_Q1: u32 = 134215681;
    pub const OMR_N1: usize = 1024;
    pub const OMR_KS_DIGITS: usize = 27;
    pub const OMR_NI: usize = 670;
    pub const OMR_QI: u32 = 4096;
    pub const OMR_Q2: u64 = 1125899906826241;
    pub const OMR_N2: usize = 2048;
    pub const OMR_TRACE_STEPS: usize = 11;
    pub const OMR_TRACE_DIGITS: usize = 25;
    pub const OMR_P: u32 = 257;
    pub const OMR_PAYLOAD_LEN: usize = 612;
    pub const OMR_PAYLOAD_LEN_MAX: usize = 16384;
    pub const OMR_PAYLOAD_PER_CT_MAX: u32 = 16;

    #[repr(C)]
    pub struct OmrSecretKeyPack {
        _private: [u8; 0],
    }
    #[repr(C)]
    pub struct OmrCtx {
        _private: [u8; 0],
    }
    #[repr(C)]
    pub struct OmrDigest {
        _private: [u8; 0],
    }
    #[repr(C)]
    pub struct OmrAuditor {
        _private: [u8; 0],
    }
    #[repr(C)]
    pub struct OmrSender {
        _private: [u8; 0],
    }
    /// `omr_clue_key`: LwePublicKeyRlweMode (A, B = A s0 + E) over Z_2048[X]/(X^512 + 1), the wire form.
    #[repr(C)]
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub struct OmrClueKey {
        pub a: [u16; OMR_N0],
        pub b: [u16; OMR_N0],
    }
    pub const OMR_AUDIT_RESIDUAL_BINS: usize = 50;
    /// `omr_ct_audit`: the record that classifies one ciphertext.
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct OmrCtAudit {
        pub max_abs_residual: u64,
        pub nonzero: u32,
        pub first: u32,
    }
    /// `omr_audit_summary`: integer tallies that every audit call adds into.
    #[repr(C)]
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub struct OmrAuditSummary {
        pub ciphertexts: u64,
        pub zero: u64,
        pub one_hot: u64,
        pub other: u64,
        pub max_abs_residual: u64,
        pub residual_bits: [u64; OMR_AUDIT_RESIDUAL_BINS],
    }
    impl Default for OmrAuditSummary {
        fn default() -> Self {
            Self { ciphertexts: 0, zero: 0, one_hot: 0, other: 0, max_abs_residual: 0,
                   residual_bits: [0; OMR_AUDIT_RESIDUAL_BINS] }
        }
    }
    /// `omr_key_audit_summary`: integer tallies that every key-audit call adds into. `Default` is the
    /// value to start from: zeros and `first_row_over = u64::MAX` (no row over the limit yet).
    #[repr(C)]
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub struct OmrKeyAuditSummary {
        pub rows: u64,
        pub noncanonical: u64,
        pub max_abs_noise: u64,
        pub rows_over: u64,
        pub first_row_over: u64,
        pub noise_bits: [u64; OMR_AUDIT_RESIDUAL_BINS],
    }
    impl Default for OmrKeyAuditSummary {
        fn default() -> Self {
            Self { rows: 0, noncanonical: 0, max_abs_noise: 0, rows_over: 0, first_row_over: u64::MAX,
                   noise_bits: [0; OMR_AUDIT_RESIDUAL_BINS] }
        }
    }
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct OmrDigestInfo {
        pub index_ct: u32,
        pub payload_ct: u32,
        pub combination_count: u32,
        pub cmb_count_per_cipher: u32,
        pub all_payloads_count: usize,
        pub messages: usize,
        pub pv_capacity_messages: usize,
    }
    /// `OMR_WEIGHT_SEEK_MAX`: the rejections an `omr_weight_seek` holds.
    pub const OMR_WEIGHT_SEEK_MAX: usize = 32;
    /// `omr_weight_seek` (include/omr_gpu.h, "Reference payload weights by seek").
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct OmrWeightSeek {
        pub draws: u64,
        pub n: u32,
        pub zone: u32,
        pub at: [u64; OMR_WEIGHT_SEEK_MAX],
    }
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct OmrRetrievalParams {
        pub index_slots_per_bucket: u32,
        pub slots_per_bucket: u32,
        pub slots_per_segment: u32,
        pub segment_per_cipher: u32,
        pub max_encode_indices_cipher_count: u32,
        pub combination_count: u32,
        pub cmb_count_per_cipher: u32,
        pub cmb_cipher_count: u32,
    }
    /// `omr_payload_layout`: the payload digest of a board whose payloads are `payload_len` words long.
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct OmrPayloadLayout {
        pub payload_len: u32,
        pub combination_count: u32,
        pub cmb_count_per_cipher: u32,
        pub stripes: u32,
        pub payload_ct: u32,
    }
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct OmrDetectionKeyView {
        pub bsk1: *const u32,
        pub ksk: *const u32,
        pub bsk2: *const u64,
        pub trace_key: *const u64,
    }
    /// The seeded form of a detection key: the bodies and the public mask seed.
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct OmrSeededKeyView {
        pub bsk1_b: *const u32,
        pub ksk_b: *const u32,
        pub bsk2_b: *const u64,
        pub trace_key_b: *const u64,
        pub mask_seed: u64,
    }
    /// `omr_key_component`: the `component` argument of `omr_key_masks`.
    pub const OMR_KEY_BSK1: c_int = 0;
    pub const OMR_KEY_KSK: c_int = 1;
    pub const OMR_KEY_BSK2: c_int = 2;
    pub const OMR_KEY_TRACE: c_int = 3;
    /// `omr_launch_kind`: the indices of `omr_ctx_launch_record`'s counters.
    pub const OMR_LAUNCH_BR2F: usize = 0;
    pub const OMR_LAUNCH_BR2F_GUARD: usize = 1;
    pub const OMR_LAUNCH_BR2L: usize = 2;
    pub const OMR_LAUNCH_BR2X: usize = 3;
    pub const OMR_LAUNCH_BR2Y: usize = 4;
    pub const OMR_LAUNCH_BR2Y_HELPERS: usize = 5;
    pub const OMR_LAUNCH_BR2_FROM: usize = 6;
    pub const OMR_LAUNCH_GUARD_FALLBACK: usize = 7;
    pub const OMR_LAUNCH_TRACE_FFT: usize = 8;
    pub const OMR_LAUNCH_TRACE_FFT_GUARD: usize = 9;
    pub const OMR_LAUNCH_TRACE_X: usize = 10;
    pub const OMR_LAUNCH_TRACE_KERNEL: usize = 11;
    pub const OMR_LAUNCH_COUNT: usize = 12;
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct OmrDetectTiming {
        pub total_ms: f32,
        pub first_level_ms: f32,
        pub second_level_ms: f32,
        pub trace_ms: f32,
        pub key_switch_ms: f32,
        pub messages: usize,
        pub trace_separate: c_int,
    }

    extern "C" {
        pub fn omr_last_error() -> *const c_char;
        pub fn omr_version() -> *const c_char;

        // key generation (key_gen/mod.rs:21-27, key_gen/secret.rs:46-178, clue.rs:27-34)
        pub fn omr_keygen_secret(seed: u64, out: *mut *mut OmrSecretKeyPack) -> OmrStatus;
        pub fn omr_secret_destroy(sk: *mut OmrSecretKeyPack);
        pub fn omr_secret_export(sk: *const OmrSecretKeyPack, s0: *mut u8, s1: *mut i8, s_int: *mut u8,
                                 s2: *mut i8) -> OmrStatus;
        pub fn omr_keygen_detection_key(sk: *const OmrSecretKeyPack, seed: u64, bsk1: *mut u32, ksk: *mut u32,
                                        bsk2: *mut u64, trace_key: *mut u64, nthreads: c_int) -> OmrStatus;
        pub fn omr_gen_clues(sk: *const OmrSecretKeyPack, seed: u64, first: u64, count: usize, clue_a: *mut u16,
                             clue_b: *mut u16, nthreads: c_int) -> OmrStatus;
        pub fn omr_gen_clues_device(sk: *const OmrSecretKeyPack, seed: u64, first: u64, count: usize,
                                    d_clue_a: *mut u16, d_clue_b: *mut u16, stream: *mut c_void) -> OmrStatus;
        pub fn omr_keygen_detection_key_device(sk: *const OmrSecretKeyPack, seed: u64, d_bsk1: *mut u32,
                                               d_ksk: *mut u32, d_bsk2: *mut u64, d_trace_key: *mut u64,
                                               stream: *mut c_void) -> OmrStatus;

        // sender: public clue keys, mixed-recipient clues, clue opening (sender.rs:27-32, secret.rs:99-107, :267-270)
        pub fn omr_secret_clue_key(sk: *const OmrSecretKeyPack, out: *mut OmrClueKey) -> OmrStatus;
        pub fn omr_clue_key_validate(keys: *const OmrClueKey, n_keys: usize, noncanonical: *mut u64) -> OmrStatus;
        pub fn omr_clue_key_noise_support(k: *mut u64) -> OmrStatus;
        pub fn omr_clue_key_audit(sk: *const OmrSecretKeyPack, key: *const OmrClueKey, limit: u64,
                                  max_abs_noise: *mut u64, coeffs_over: *mut u32, noncanonical: *mut u32) -> OmrStatus;
        pub fn omr_sender_create(keys: *const OmrClueKey, n_keys: usize, device: c_int,
                                 out: *mut *mut OmrSender) -> OmrStatus;
        pub fn omr_sender_destroy(s: *mut OmrSender);
        pub fn omr_sender_gen_clues(s: *const OmrSender, recipient: *const u32, seed: u64, first: u64, count: usize,
                                    clue_a: *mut u16, clue_b: *mut u16, nthreads: c_int) -> OmrStatus;
        pub fn omr_sender_gen_clues_device(s: *mut OmrSender, d_recipient: *const u32, seed: u64, first: u64,
                                           count: usize, d_clue_a: *mut u16, d_clue_b: *mut u16,
                                           hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_clue_open(sk: *const OmrSecretKeyPack, clue_a: *const u16, clue_b: *const u16, count: usize,
                             values: *mut u8, pertinent: *mut u8, max_abs_noise: *mut u8, nthreads: c_int) -> OmrStatus;
        pub fn omr_clue_open_device(sk: *const OmrSecretKeyPack, d_clue_a: *const u16, d_clue_b: *const u16,
                                    count: usize, d_values: *mut u8, d_pertinent: *mut u8, d_max_abs_noise: *mut u8,
                                    hip_stream: *mut c_void) -> OmrStatus;

        // seeded detection key: the bodies of a key whose masks come from a public seed
        pub fn omr_keygen_seeded_key(sk: *const OmrSecretKeyPack, seed: u64, mask_seed: u64, bsk1_b: *mut u32,
                                     ksk_b: *mut u32, bsk2_b: *mut u64, trace_key_b: *mut u64,
                                     nthreads: c_int) -> OmrStatus;
        pub fn omr_keygen_seeded_key_device(sk: *const OmrSecretKeyPack, seed: u64, mask_seed: u64,
                                            d_bsk1_b: *mut u32, d_ksk_b: *mut u32, d_bsk2_b: *mut u64,
                                            d_trace_key_b: *mut u64, stream: *mut c_void) -> OmrStatus;
        pub fn omr_expand_detection_key(key: *const OmrSeededKeyView, bsk1: *mut u32, ksk: *mut u32,
                                        bsk2: *mut u64, trace_key: *mut u64, nthreads: c_int) -> OmrStatus;
        pub fn omr_expand_detection_key_device(key: *const OmrSeededKeyView, d_bsk1: *mut u32, d_ksk: *mut u32,
                                               d_bsk2: *mut u64, d_trace_key: *mut u64,
                                               stream: *mut c_void) -> OmrStatus;
        pub fn omr_key_masks(mask_seed: u64, component: c_int, first_row: usize, rows: usize,
                             out: *mut c_void) -> OmrStatus;
        pub fn omr_key_masks_device(mask_seed: u64, component: c_int, first_row: usize, rows: usize,
                                    d_out: *mut c_void, stream: *mut c_void) -> OmrStatus;

        // retrieval layout and payload weights (retrieval_params.rs:50-106, detector.rs:376-387)
        pub fn omr_get_retrieval_params(all_payloads_count: usize, pertinent_count: usize,
                                        out: *mut OmrRetrievalParams) -> OmrStatus;
        pub fn omr_payload_weights(seed: *const u8, all_payloads_count: usize, combination_count: u32,
                                   cmb_cipher_count: u32, cmb_count_per_cipher: u32, out: *mut u16) -> OmrStatus;

        // retriever (retriever.rs:63-130, 188-260; matrix.rs:164-247)
        pub fn omr_decrypt_decode(sk: *const OmrSecretKeyPack, ct: *const u64, n: usize, out: *mut u32) -> OmrStatus;
        pub fn omr_retrieve_indices(sk: *const OmrSecretKeyPack, idx_cts: *const u64, n_ct: u32,
                                    all_payloads_count: usize, pertinent_count: usize, indices: *mut usize,
                                    cap: usize, found: *mut usize) -> OmrStatus;
        pub fn omr_retrieve_payloads(sk: *const OmrSecretKeyPack, pay_cts: *const u64, n_ct: u32,
                                     all_payloads_count: usize, combination_count: u32, weights: *const u16,
                                     indices: *const usize,
                                     n_indices: usize, payloads: *mut u16) -> OmrStatus;

        // auditor (omd.rs:48-58 KAT and NoiseSigmaInfo, retriever.rs:390-560, in exact integers)
        pub fn omr_auditor_create(sk: *const OmrSecretKeyPack, device: c_int, out: *mut *mut OmrAuditor) -> OmrStatus;
        pub fn omr_auditor_destroy(aud: *mut OmrAuditor);
        pub fn omr_auditor_set_grid(aud: *mut OmrAuditor, workgroups: c_uint) -> OmrStatus;
        pub fn omr_auditor_set_staging(aud: *mut OmrAuditor, max_ciphertexts: usize) -> OmrStatus;
        pub fn omr_audit_device(aud: *mut OmrAuditor, d_cts: *const u64, n: usize, d_records: *mut OmrCtAudit,
                                d_decoded: *mut u16, d_summary: *mut OmrAuditSummary,
                                hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_audit(aud: *mut OmrAuditor, cts: *const u64, n: usize, records: *mut OmrCtAudit,
                         decoded: *mut u16, summary: *mut OmrAuditSummary) -> OmrStatus;
        pub fn omr_audit_cpu(sk: *const OmrSecretKeyPack, cts: *const u64, n: usize, records: *mut OmrCtAudit,
                             decoded: *mut u16, summary: *mut OmrAuditSummary, nthreads: c_int) -> OmrStatus;

        // detector (detector.rs:85-453)
        pub fn omr_ctx_create(key: *const OmrDetectionKeyView, device: c_int, out: *mut *mut OmrCtx) -> OmrStatus;
        pub fn omr_ctx_create_seeded(key: *const OmrSeededKeyView, device: c_int, out: *mut *mut OmrCtx) -> OmrStatus;
        pub fn omr_ctx_destroy(ctx: *mut OmrCtx);
        pub fn omr_detect_kernels() -> *const c_char;
        pub fn omr_ctx_set_batch(ctx: *mut OmrCtx, batch: usize) -> OmrStatus;
        pub fn omr_ctx_set_latency_threshold(ctx: *mut OmrCtx, max_messages: usize) -> OmrStatus;
        pub fn omr_ctx_set_exact_level1(ctx: *mut OmrCtx, enable: c_int) -> OmrStatus;
        pub fn omr_ctx_set_encode_chunks(ctx: *mut OmrCtx, max_chunks: usize) -> OmrStatus;
        pub fn omr_detect_batch(ctx: *mut OmrCtx, clue_a: *const u16, clue_b: *const u16, d: usize,
                                out: *mut u64) -> OmrStatus;
        pub fn omr_detect(ctx: *mut OmrCtx, clue_a: *const u16, clue_b: *const u16, out: *mut u64) -> OmrStatus;
        pub fn omr_ctx_set_coalescing(ctx: *mut OmrCtx, max_messages: usize, window_us: c_long) -> OmrStatus;
        pub fn omr_ctx_coalescing_stats(ctx: *mut OmrCtx, calls: *mut usize, launches: *mut usize) -> OmrStatus;
        pub fn omr_detect_batch_device(ctx: *mut OmrCtx, d_clue_a: *const u16, d_clue_b: *const u16, d: usize,
                                       d_out: *mut u64, hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_ctx_enable_timing(ctx: *mut OmrCtx, mode: c_int) -> OmrStatus;
        pub fn omr_last_timing(ctx: *mut OmrCtx, t: *mut OmrDetectTiming) -> OmrStatus;
        pub fn omr_detect_with_time_info(ctx: *mut OmrCtx, clue_a: *const u16, clue_b: *const u16, d: usize,
                                         out: *mut u64, t: *mut OmrDetectTiming) -> OmrStatus;
        pub fn omr_ctx_check(ctx: *mut OmrCtx, hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_ctx_set_rounding_guard(ctx: *mut OmrCtx, enable: c_int) -> OmrStatus;
        pub fn omr_ctx_rounding_margin(ctx: *mut OmrCtx, observed: *mut f64, apriori: *mut f64, kappa: *mut f64,
                                       reset: c_int) -> OmrStatus;
        pub fn omr_ctx_exactness(ctx: *mut OmrCtx, guarded: *mut c_int, breaches: *mut u64) -> OmrStatus;
        pub fn omr_ctx_launch_record(ctx: *mut OmrCtx, counts: *mut u64) -> OmrStatus;
        pub fn omr_fft_twiddles_dd(level: c_int, out: *mut f64) -> OmrStatus;
        pub fn omr_ctx_key_spectrum(ctx: *mut OmrCtx, level: c_int, first: usize, count: usize,
                                    out: *mut f64) -> OmrStatus;
        pub fn omr_encode_indices(ctx: *mut OmrCtx, pv: *const u64, d: usize, global_offset: usize,
                                  all_payloads_count: usize, seed: u64, ct: u32, out: *mut u64) -> OmrStatus;
        pub fn omr_encode_indices_device(ctx: *mut OmrCtx, d_pv: *const u64, d: usize, global_offset: usize,
                                         all_payloads_count: usize, seed: u64, first_ct: u32, n_ct: u32,
                                         d_out: *mut u64, hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_encode_payloads(ctx: *mut OmrCtx, pv: *const u64, payloads: *const u16, d: usize,
                                   global_offset: usize, all_payloads_count: usize, weights: *const u16, n_ct: u32,
                                   cmb_per_ct: u32, out: *mut u64) -> OmrStatus;
        pub fn omr_encode_payloads_device(ctx: *mut OmrCtx, d_pv: *const u64, d_payloads: *const u16, d: usize,
                                          global_offset: usize, all_payloads_count: usize, d_weights: *const u16,
                                          n_ct: u32, cmb_per_ct: u32, d_out: *mut u64,
                                          hip_stream: *mut c_void) -> OmrStatus;

        // digest session (examples/omr.rs:160-203 inside the library)
        pub fn omr_digest_begin(ctx: *mut OmrCtx, all_payloads_count: usize, pertinent_count: usize,
                                index_seed: u64, weight_seed: *const u8, hip_stream: *mut c_void,
                                out: *mut *mut OmrDigest) -> OmrStatus;
        pub fn omr_digest_update(dg: *mut OmrDigest, clue_a: *const u16, clue_b: *const u16, payloads: *const u16,
                                 d: usize, global_offset: usize) -> OmrStatus;
        pub fn omr_digest_update_device(dg: *mut OmrDigest, d_clue_a: *const u16, d_clue_b: *const u16,
                                        d_payloads: *const u16, d: usize, global_offset: usize) -> OmrStatus;
        pub fn omr_digest_merge(dg: *mut OmrDigest, idx_cts: *const u64, pay_cts: *const u64) -> OmrStatus;
        pub fn omr_digest_read(dg: *mut OmrDigest, idx_cts: *mut u64, pay_cts: *mut u64) -> OmrStatus;
        pub fn omr_digest_get_info(dg: *mut OmrDigest, info: *mut OmrDigestInfo) -> OmrStatus;
        pub fn omr_digest_destroy(dg: *mut OmrDigest);
        pub fn omr_digest_enable_bitmap(dg: *mut OmrDigest) -> OmrStatus;
        pub fn omr_digest_read_bitmap(dg: *mut OmrDigest, bitmap_cts: *mut u64) -> OmrStatus;
        pub fn omr_digest_merge_bitmap(dg: *mut OmrDigest, bitmap_cts: *const u64) -> OmrStatus;

        // indexed payload weights (none in the reference)
        pub fn omr_indexed_weights_at(seed: *const u8, combination_count: u32, first_combo: u32, n_combos: u32,
                                      indices: *const usize, n_indices: usize, out: *mut u16,
                                      nthreads: c_int) -> OmrStatus;
        pub fn omr_indexed_weights_table(seed: *const u8, all_payloads_count: usize, combination_count: u32,
                                         cmb_cipher_count: u32, cmb_count_per_cipher: u32, out: *mut u16,
                                         nthreads: c_int) -> OmrStatus;
        pub fn omr_indexed_weights_table_device(seed: *const u8, all_payloads_count: usize, combination_count: u32,
                                                cmb_cipher_count: u32, cmb_count_per_cipher: u32, d_out: *mut u16,
                                                hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_encode_payloads_indexed_device(ctx: *mut OmrCtx, d_pv: *const u64, d_payloads: *const u16,
                                                  d: usize, global_offset: usize, all_payloads_count: usize,
                                                  seed: *const u8, combination_count: u32, first_ct: u32,
                                                  n_ct: u32, cmb_per_ct: u32, d_out: *mut u64,
                                                  hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_encode_payloads_indexed(ctx: *mut OmrCtx, pv: *const u64, payloads: *const u16, d: usize,
                                           global_offset: usize, all_payloads_count: usize, seed: *const u8,
                                           combination_count: u32, first_ct: u32, n_ct: u32, cmb_per_ct: u32,
                                           out: *mut u64) -> OmrStatus;
        pub fn omr_digest_begin_indexed(ctx: *mut OmrCtx, all_payloads_count: usize, pertinent_count: usize,
                                        index_seed: u64, weight_seed: *const u8, hip_stream: *mut c_void,
                                        out: *mut *mut OmrDigest) -> OmrStatus;
        pub fn omr_digest_device_bytes(dg: *mut OmrDigest, total: *mut usize, weights: *mut usize) -> OmrStatus;
        pub fn omr_retrieve_payloads_indexed(sk: *const OmrSecretKeyPack, pay_cts: *const u64, n_ct: u32,
                                             all_payloads_count: usize, combination_count: u32,
                                             weight_seed: *const u8, indices: *const usize, n_indices: usize,
                                             payloads: *mut u16) -> OmrStatus;

        // payload length as a board parameter (none in the reference)
        pub fn omr_get_payload_layout(pertinent_count: usize, payload_len: usize,
                                      out: *mut OmrPayloadLayout) -> OmrStatus;
        pub fn omr_encode_payloads_indexed_len_device(ctx: *mut OmrCtx, d_pv: *const u64, d_payloads: *const u16,
                                                      d: usize, global_offset: usize, all_payloads_count: usize,
                                                      seed: *const u8, combination_count: u32, payload_len: u32,
                                                      cmb_per_ct: u32, first_ct: u32, n_ct: u32, d_out: *mut u64,
                                                      hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_encode_payloads_indexed_len(ctx: *mut OmrCtx, pv: *const u64, payloads: *const u16, d: usize,
                                               global_offset: usize, all_payloads_count: usize, seed: *const u8,
                                               combination_count: u32, payload_len: u32, cmb_per_ct: u32,
                                               first_ct: u32, n_ct: u32, out: *mut u64) -> OmrStatus;
        pub fn omr_digest_begin_indexed_len(ctx: *mut OmrCtx, all_payloads_count: usize, pertinent_count: usize,
                                            index_seed: u64, weight_seed: *const u8, payload_len: usize,
                                            hip_stream: *mut c_void, out: *mut *mut OmrDigest) -> OmrStatus;
        pub fn omr_digest_get_payload_layout(dg: *mut OmrDigest, layout: *mut OmrPayloadLayout) -> OmrStatus;
        pub fn omr_retrieve_payloads_indexed_len(sk: *const OmrSecretKeyPack, pay_cts: *const u64, n_ct: u32,
                                                 all_payloads_count: usize, layout: *const OmrPayloadLayout,
                                                 weight_seed: *const u8, indices: *const usize, n_indices: usize,
                                                 payloads: *mut u16) -> OmrStatus;
        pub fn omr_auditor_retrieve_payloads_indexed_len(aud: *mut OmrAuditor, pay_cts: *const c_void, n_ct: u32,
                                                         bits: c_int, all_payloads_count: usize,
                                                         layout: *const OmrPayloadLayout, weight_seed: *const u8,
                                                         indices: *const usize, n_indices: usize,
                                                         payloads: *mut u16) -> OmrStatus;

        // bitmap digest (none in the reference)
        pub fn omr_bitmap_ct_count(all_payloads_count: usize, n_ct: *mut u32) -> OmrStatus;
        pub fn omr_encode_bitmap_device(ctx: *mut OmrCtx, d_pv: *const u64, d: usize, global_offset: usize,
                                        all_payloads_count: usize, d_out: *mut u64, hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_encode_bitmap(ctx: *mut OmrCtx, pv: *const u64, d: usize, global_offset: usize,
                                 all_payloads_count: usize, out: *mut u64) -> OmrStatus;
        pub fn omr_bitmap_indices(decoded: *const u16, n_ct: u32, all_payloads_count: usize, indices: *mut usize,
                                  cap: usize, found: *mut usize) -> OmrStatus;
        pub fn omr_retrieve_bitmap(sk: *const OmrSecretKeyPack, bitmap_cts: *const u64, n_ct: u32,
                                   all_payloads_count: usize, indices: *mut usize, cap: usize,
                                   found: *mut usize) -> OmrStatus;

        // compact ciphertexts (none in the reference): q2 -> 2^bits, bit-packed, 512 * bits bytes each
        pub fn omr_compact_ct_bytes(bits: c_int, bytes: *mut usize) -> OmrStatus;
        pub fn omr_compact_residual_bound(sk: *const OmrSecretKeyPack, bits: c_int, r: *mut u64) -> OmrStatus;
        pub fn omr_compact_cts_cpu(cts: *const u64, n: usize, bits: c_int, out: *mut c_void, nthreads: c_int) -> OmrStatus;
        pub fn omr_compact_expand_cpu(packed: *const c_void, n: usize, bits: c_int, cts_out: *mut u64,
                                      nthreads: c_int) -> OmrStatus;
        pub fn omr_compact_cts_device(ctx: *mut OmrCtx, d_cts: *const u64, n: usize, bits: c_int, d_out: *mut c_void,
                                      hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_compact_cts(ctx: *mut OmrCtx, cts: *const u64, n: usize, bits: c_int, out: *mut c_void) -> OmrStatus;
        pub fn omr_ctx_set_compact_grid(ctx: *mut OmrCtx, workgroups: c_uint) -> OmrStatus;
        pub fn omr_ctx_set_compact_staging(ctx: *mut OmrCtx, max_ciphertexts: usize) -> OmrStatus;
        pub fn omr_compact_expand_device(aud: *mut OmrAuditor, d_packed: *const c_void, n: usize, bits: c_int,
                                         d_cts: *mut u64, hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_audit_compact(aud: *mut OmrAuditor, packed: *const c_void, n: usize, bits: c_int,
                                 records: *mut OmrCtAudit, decoded: *mut u16,
                                 summary: *mut OmrAuditSummary) -> OmrStatus;
        pub fn omr_digest_read_compact(dg: *mut OmrDigest, bits: c_int, idx_packed: *mut c_void,
                                       pay_packed: *mut c_void, bitmap_packed: *mut c_void) -> OmrStatus;

        // key audit
        pub fn omr_key_noise_support(component: c_int, k: *mut u64) -> OmrStatus;
        pub fn omr_audit_key_rows_device(aud: *mut OmrAuditor, component: c_int, d_rows: *const c_void, first_row: usize,
                                         rows: usize, limit: u64, d_row_max: *mut u64,
                                         d_summary: *mut OmrKeyAuditSummary, hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_audit_key_rows_cpu(sk: *const OmrSecretKeyPack, component: c_int, rows_ptr: *const c_void,
                                      first_row: usize, rows: usize, limit: u64, row_max: *mut u64,
                                      summary: *mut OmrKeyAuditSummary, nthreads: c_int) -> OmrStatus;
        pub fn omr_audit_key(aud: *mut OmrAuditor, key: *const OmrDetectionKeyView, limit: *const u64,
                             out: *mut OmrKeyAuditSummary) -> OmrStatus;
        pub fn omr_audit_key_seeded(aud: *mut OmrAuditor, key: *const OmrSeededKeyView, limit: *const u64,
                                    out: *mut OmrKeyAuditSummary) -> OmrStatus;
        pub fn omr_audit_key_cpu(sk: *const OmrSecretKeyPack, key: *const OmrDetectionKeyView, limit: *const u64,
                                 out: *mut OmrKeyAuditSummary, nthreads: c_int) -> OmrStatus;
        pub fn omr_key_count_noncanonical_device(level: c_int, d_words: *const c_void, n: usize, d_count: *mut u64,
                                                 hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_key_validate(key: *const OmrDetectionKeyView, noncanonical: *mut u64, nthreads: c_int) -> OmrStatus;
        pub fn omr_key_validate_device(key: *const OmrDetectionKeyView, device: c_int, noncanonical: *mut u64) -> OmrStatus;
        pub fn omr_key_validate_seeded(key: *const OmrSeededKeyView, noncanonical: *mut u64, nthreads: c_int) -> OmrStatus;
        pub fn omr_key_validate_seeded_device(key: *const OmrSeededKeyView, device: c_int,
                                              noncanonical: *mut u64) -> OmrStatus;

        // solve mod 257 and retrieval on the auditor
        pub fn omr_solve_mod257_cpu(matrix: *const u16, rhs: *const u16, rows: usize, cols: usize, width: usize,
                                    solution: *mut u16, singular_col: *mut usize, nthreads: c_int) -> OmrStatus;
        pub fn omr_solve_geometry(panel_cols: *mut c_uint, tile_rows: *mut c_uint, tile_width: *mut c_uint) -> OmrStatus;
        pub fn omr_solve_mod257_device(aud: *mut OmrAuditor, d_matrix: *const u16, d_rhs: *const u16, rows: usize,
                                       cols: usize, width: usize, d_solution: *mut u16, d_status: *mut u32,
                                       hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_solve_profile(aud: *mut OmrAuditor, enable: c_int, step_ms: *mut f32) -> OmrStatus;
        pub fn omr_auditor_retrieve_indices(aud: *mut OmrAuditor, idx_cts: *const c_void, n_ct: u32, bits: c_int,
                                            all_payloads_count: usize, pertinent_count: usize, indices: *mut usize,
                                            cap: usize, found: *mut usize) -> OmrStatus;
        pub fn omr_auditor_retrieve_payloads(aud: *mut OmrAuditor, pay_cts: *const c_void, n_ct: u32, bits: c_int,
                                             all_payloads_count: usize, combination_count: u32,
                                             weights: *const u16, indices: *const usize, n_indices: usize,
                                             payloads: *mut u16) -> OmrStatus;
        pub fn omr_auditor_retrieve_payloads_indexed(aud: *mut OmrAuditor, pay_cts: *const c_void, n_ct: u32,
                                                     bits: c_int, all_payloads_count: usize, combination_count: u32,
                                                     weight_seed: *const u8, indices: *const usize, n_indices: usize,
                                                     payloads: *mut u16) -> OmrStatus;
        pub fn omr_auditor_decode_digest_indexed(aud: *mut OmrAuditor, idx_cts: *const c_void, n_idx_ct: u32,
                                                 pay_cts: *const c_void, n_pay_ct: u32, bits: c_int,
                                                 all_payloads_count: usize, pertinent_count: usize,
                                                 weight_seed: *const u8, indices: *mut usize, cap: usize,
                                                 found: *mut usize, payloads: *mut u16,
                                                 summary: *mut OmrAuditSummary) -> OmrStatus;

        // reference payload weights by seek (none in the reference)
        pub fn omr_weight_seek_build_cpu(seed: *const u8, draws: u64, nthreads: c_int,
                                         out: *mut OmrWeightSeek) -> OmrStatus;
        pub fn omr_weight_seek_build_device(seed: *const u8, draws: u64, out: *mut OmrWeightSeek,
                                            hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_weight_seek_build_zone_cpu(seed: *const u8, draws: u64, zone: u32, nthreads: c_int,
                                              out: *mut OmrWeightSeek) -> OmrStatus;
        pub fn omr_weight_seek_build_zone_device(seed: *const u8, draws: u64, zone: u32, out: *mut OmrWeightSeek,
                                                 hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_payload_weights_at(seed: *const u8, all_payloads_count: usize, combination_count: u32,
                                      seek: *const OmrWeightSeek, first_combo: u32, n_combos: u32,
                                      indices: *const usize, n_indices: usize, out: *mut u16,
                                      nthreads: c_int) -> OmrStatus;
        pub fn omr_encode_payloads_seek_device(ctx: *mut OmrCtx, d_pv: *const u64, d_payloads: *const u16, d: usize,
                                               global_offset: usize, all_payloads_count: usize, seed: *const u8,
                                               seek: *const OmrWeightSeek, combination_count: u32, first_ct: u32,
                                               n_ct: u32, cmb_per_ct: u32, d_out: *mut u64,
                                               hip_stream: *mut c_void) -> OmrStatus;
        pub fn omr_encode_payloads_seek(ctx: *mut OmrCtx, pv: *const u64, payloads: *const u16, d: usize,
                                        global_offset: usize, all_payloads_count: usize, seed: *const u8,
                                        seek: *const OmrWeightSeek, combination_count: u32, first_ct: u32,
                                        n_ct: u32, cmb_per_ct: u32, out: *mut u64) -> OmrStatus;
        pub fn omr_digest_begin_seek(ctx: *mut OmrCtx, all_payloads_count: usize, pertinent_count: usize,
                                     index_seed: u64, weight_seed: *const u8, hip_stream: *mut c_void,
                                     out: *mut *mut OmrDigest) -> OmrStatus;
        pub fn omr_retrieve_payloads_seek(sk: *const OmrSecretKeyPack, pay_cts: *const u64, n_ct: u32,
                                          all_payloads_count: usize, combination_count: u32,
                                          weight_seed: *const u8, seek: *const OmrWeightSeek,
                                          indices: *const usize, n_indices: usize, payloads: *mut u16) -> OmrStatus;
        pub fn omr_auditor_retrieve_payloads_seek(aud: *mut OmrAuditor, pay_cts: *const c_void, n_ct: u32,
                                                  bits: c_int, all_payloads_count: usize, combination_count: u32,
                                                  weight_seed: *const u8, seek: *const OmrWeightSeek,
                                                  indices: *const usize, n_indices: usize,
                                                  payloads: *mut u16) -> OmrStatus;

        // stage entry points (benches/two_level_bs.rs)
        pub fn omr_first_level(ctx: *mut OmrCtx, clue_a: *const u16, clue_b: *const u16, d: usize,
                               lwe_int: *mut u32) -> OmrStatus;
        pub fn omr_sum_key_switch(ctx: *mut OmrCtx, ext: *const u32, n: usize, lwe_int: *mut u32) -> OmrStatus;
        pub fn omr_blind_rotate_level1(ctx: *mut OmrCtx, lwe_a: *const u16, lwe_b: *const u16, n: usize,
                                       out: *mut u64) -> OmrStatus;
        pub fn omr_fft1_mul(ctx: *mut OmrCtx, a: *const u32, k: *const u32, n: usize, out: *mut u64) -> OmrStatus;
        pub fn omr_second_level(ctx: *mut OmrCtx, lwe_int: *const u32, n: usize, out: *mut u64) -> OmrStatus;
        pub fn omr_blind_rotate_level2(ctx: *mut OmrCtx, lwe_int: *const u32, n: usize, out: *mut u64) -> OmrStatus;
        pub fn omr_blind_rotate_level1_from(ctx: *mut OmrCtx, lwe_a: *const u16, lwe_b: *const u16, n: usize,
                                            acc0: *const u64, out: *mut u64) -> OmrStatus;
        pub fn omr_blind_rotate_level2_from(ctx: *mut OmrCtx, lwe_int: *const u32, n: usize, acc0: *const u64,
                                            out: *mut u64) -> OmrStatus;
        pub fn omr_trace(ctx: *mut OmrCtx, rlwe: *const u64, n: usize, out: *mut u64) -> OmrStatus;
        pub fn omr_ntt(level: c_int, inverse: c_int, polys: *mut u64, n: usize, device: c_int) -> OmrStatus;
    }
}

use ffi::*;

/// A failed library call: the status code and `omr_last_error()`'s message.
#[derive(Debug, Clone)]
pub struct OmrError {
    pub status: OmrStatus,
    pub message: String,
}

impl fmt::Display for OmrError {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "omr_gpu status {}: {}", self.status, self.message)
    }
}
impl std::error::Error for OmrError {}

fn check(st: OmrStatus) -> Result<(), OmrError> {
    if st == OMR_OK {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(omr_last_error()) }.to_string_lossy().into_owned();
    Err(OmrError { status: st, message })
}

/// `CmLweCiphertext<u16>` of one message: mask `a` (512) and the 7 bodies, values mod 2048.
#[derive(Clone)]
pub struct Clue {
    pub a: [u16; OMR_N0],
    pub b: [u16; OMR_CLUE_COUNT],
}

/// `NttRlweCiphertext<SecondLevelField>`: (a, b) in the NTT domain (include/omr_gpu.h order).
#[derive(Clone)]
pub struct NttRlwe {
    pub a: Box<[u64; OMR_N2]>,
    pub b: Box<[u64; OMR_N2]>,
}

impl NttRlwe {
    fn from_flat(v: &[u64]) -> Self {
        let mut a = Box::new([0u64; OMR_N2]);
        let mut b = Box::new([0u64; OMR_N2]);
        a.copy_from_slice(&v[..OMR_N2]);
        b.copy_from_slice(&v[OMR_N2..2 * OMR_N2]);
        NttRlwe { a, b }
    }
    fn flatten(items: &[NttRlwe]) -> Vec<u64> {
        let mut v = Vec::with_capacity(items.len() * 2 * OMR_N2);
        for c in items {
            v.extend_from_slice(&c.a[..]);
            v.extend_from_slice(&c.b[..]);
        }
        v
    }
}

/// `Payload` (payload.rs:14): 612 values, bytes stored as u16.
pub type Payload = [u16; OMR_PAYLOAD_LEN];

/// `RetrievalParams::new(257, 2048, all, pertinent, 130, 25, 2)` (retrieval_params.rs:50-106).
#[derive(Clone, Copy, Debug)]
pub struct RetrievalParams {
    pub all_payloads_count: usize,
    pub pertinent_count: usize,
    pub layout: OmrRetrievalParams,
}

impl RetrievalParams {
    pub fn new(all_payloads_count: usize, pertinent_count: usize) -> Result<Self, OmrError> {
        let mut layout = OmrRetrievalParams::default();
        check(unsafe { omr_get_retrieval_params(all_payloads_count, pertinent_count, &mut layout) })?;
        Ok(Self { all_payloads_count, pertinent_count, layout })
    }
    pub fn max_encode_indices_cipher_count(&self) -> usize {
        self.layout.max_encode_indices_cipher_count as usize
    }
    pub fn combination_count(&self) -> usize {
        self.layout.combination_count as usize
    }
    pub fn cmb_count_per_cipher(&self) -> usize {
        self.layout.cmb_count_per_cipher as usize
    }
}

/// Payload weights `StdRng::from_seed(seed)` + `Uniform<u16>(0, 257)` in the reference order
/// (detector.rs:376-387), `[cmb_cipher_count * cmb_count_per_cipher][all]`.
pub fn payload_weights(seed: &[u8; 32], rp: &RetrievalParams) -> Result<Vec<u16>, OmrError> {
    let l = rp.layout;
    let mut out = vec![0u16; (l.cmb_cipher_count * l.cmb_count_per_cipher) as usize * rp.all_payloads_count];
    check(unsafe {
        omr_payload_weights(seed.as_ptr(), rp.all_payloads_count, l.combination_count, l.cmb_cipher_count,
                            l.cmb_count_per_cipher, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// Indexed payload weights (`omr_indexed_weights_at`, none in the reference): `[n_combos][indices.len()]`,
/// the weight of combination `first_combo + r` for the global message index `indices[k]`; rows at or
/// beyond `combination_count` are zero. A function of (seed, combination, index) alone: no table.
pub fn indexed_weights_at(seed: &[u8; 32], combination_count: u32, first_combo: u32, n_combos: u32,
                          indices: &[usize]) -> Result<Vec<u16>, OmrError> {
    let mut out = vec![0u16; n_combos as usize * indices.len()];
    check(unsafe {
        omr_indexed_weights_at(seed.as_ptr(), combination_count, first_combo, n_combos, indices.as_ptr(),
                               indices.len(), out.as_mut_ptr(), 0)
    })?;
    Ok(out)
}

/// The indexed weights in `payload_weights`' layout (`omr_indexed_weights_table`),
/// `[cmb_cipher_count * cmb_count_per_cipher][all]`.
pub fn indexed_weights_table(seed: &[u8; 32], rp: &RetrievalParams) -> Result<Vec<u16>, OmrError> {
    let l = rp.layout;
    let mut out = vec![0u16; (l.cmb_cipher_count * l.cmb_count_per_cipher) as usize * rp.all_payloads_count];
    check(unsafe {
        omr_indexed_weights_table(seed.as_ptr(), rp.all_payloads_count, l.combination_count, l.cmb_cipher_count,
                                  l.cmb_count_per_cipher, out.as_mut_ptr(), 0)
    })?;
    Ok(out)
}

/// The seek of a board's payload weights (`omr_weight_seek_build_cpu`, or `_device` on the current HIP
/// device): the rejections of the reference's stream within the board's `combination_count * all` draws.
/// With it, `payload_weights`' values are found weight by weight and nobody draws the table.
pub fn weight_seek(seed: &[u8; 32], rp: &RetrievalParams, on_device: bool) -> Result<OmrWeightSeek, OmrError> {
    let draws = rp.layout.combination_count as u64 * rp.all_payloads_count as u64;
    let mut out = OmrWeightSeek::default();
    check(unsafe {
        if on_device {
            omr_weight_seek_build_device(seed.as_ptr(), draws, &mut out, std::ptr::null_mut())
        } else {
            omr_weight_seek_build_cpu(seed.as_ptr(), draws, 0, &mut out)
        }
    })?;
    Ok(out)
}

/// The recipient's matrix in the reference's convention (`omr_payload_weights_at`): `[n_combos][indices.len()]`,
/// `payload_weights`' weight of combination `first_combo + r` for the message `indices[k]`, through the seek.
pub fn payload_weights_at(seed: &[u8; 32], rp: &RetrievalParams, seek: &OmrWeightSeek, first_combo: u32,
                          n_combos: u32, indices: &[usize]) -> Result<Vec<u16>, OmrError> {
    let mut out = vec![0u16; n_combos as usize * indices.len()];
    check(unsafe {
        omr_payload_weights_at(seed.as_ptr(), rp.all_payloads_count, rp.layout.combination_count, seek, first_combo,
                               n_combos, indices.as_ptr(), indices.len(), out.as_mut_ptr(), 0)
    })?;
    Ok(out)
}

/// Coefficient-domain evaluation keys in the include/omr_gpu.h layout (`DetectionKey`,
/// key_gen/detection.rs:9-16).
pub struct DetectionKey {
    pub bsk1: Vec<u32>,
    pub ksk: Vec<u32>,
    pub bsk2: Vec<u64>,
    pub trace_key: Vec<u64>,
}

pub const BSK1_LEN: usize = OMR_N0 * 8 * 2 * OMR_N1;
pub const KSK_LEN: usize = OMR_N1 * OMR_KS_DIGITS * (OMR_NI + 1);
pub const BSK2_LEN: usize = OMR_NI * 12 * 2 * OMR_N2;
pub const TRACE_KEY_LEN: usize = OMR_TRACE_STEPS * OMR_TRACE_DIGITS * 2 * OMR_N2;

/// The seeded form of a `DetectionKey` (include/omr_gpu.h): the bodies and the public mask seed,
/// 153,120,776 bytes instead of 380,227,584.
pub struct SeededKey {
    pub bsk1_b: Vec<u32>,
    pub ksk_b: Vec<u32>,
    pub bsk2_b: Vec<u64>,
    pub trace_key_b: Vec<u64>,
    pub mask_seed: u64,
}

pub const BSK1_B_LEN: usize = BSK1_LEN / 2;
pub const KSK_B_LEN: usize = OMR_N1 * OMR_KS_DIGITS;
pub const BSK2_B_LEN: usize = BSK2_LEN / 2;
pub const TRACE_KEY_B_LEN: usize = TRACE_KEY_LEN / 2;

impl SeededKey {
    fn view(&self) -> Result<OmrSeededKeyView, OmrError> {
        if self.bsk1_b.len() != BSK1_B_LEN || self.ksk_b.len() != KSK_B_LEN || self.bsk2_b.len() != BSK2_B_LEN
            || self.trace_key_b.len() != TRACE_KEY_B_LEN
        {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "seeded key sizes".into() });
        }
        Ok(OmrSeededKeyView { bsk1_b: self.bsk1_b.as_ptr(), ksk_b: self.ksk_b.as_ptr(), bsk2_b: self.bsk2_b.as_ptr(),
                              trace_key_b: self.trace_key_b.as_ptr(), mask_seed: self.mask_seed })
    }
    /// `omr_expand_detection_key`: the full key on `nthreads` host threads (0: all).
    pub fn expand(&self, nthreads: i32) -> Result<DetectionKey, OmrError> {
        let view = self.view()?;
        let mut k = DetectionKey { bsk1: vec![0; BSK1_LEN], ksk: vec![0; KSK_LEN], bsk2: vec![0; BSK2_LEN],
                                   trace_key: vec![0; TRACE_KEY_LEN] };
        check(unsafe {
            omr_expand_detection_key(&view, k.bsk1.as_mut_ptr(), k.ksk.as_mut_ptr(), k.bsk2.as_mut_ptr(),
                                     k.trace_key.as_mut_ptr(), nthreads)
        })?;
        Ok(k)
    }
}

/// `SecretKeyPack` from `KeyGen::generate_secret_key`, deterministic from a 64-bit seed.
pub struct SecretKeyPack {
    raw: *mut OmrSecretKeyPack,
}
unsafe impl Send for SecretKeyPack {}
unsafe impl Sync for SecretKeyPack {}

impl SecretKeyPack {
    pub fn generate(seed: u64) -> Result<Self, OmrError> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { omr_keygen_secret(seed, &mut raw) })?;
        Ok(Self { raw })
    }
    /// `generate_detection_key` (secret.rs:118-178) on `nthreads` host threads (0: all).
    pub fn generate_detection_key(&self, seed: u64, nthreads: i32) -> Result<DetectionKey, OmrError> {
        let mut k = DetectionKey { bsk1: vec![0; BSK1_LEN], ksk: vec![0; KSK_LEN], bsk2: vec![0; BSK2_LEN],
                                   trace_key: vec![0; TRACE_KEY_LEN] };
        check(unsafe {
            omr_keygen_detection_key(self.raw, seed, k.bsk1.as_mut_ptr(), k.ksk.as_mut_ptr(), k.bsk2.as_mut_ptr(),
                                     k.trace_key.as_mut_ptr(), nthreads)
        })?;
        Ok(k)
    }
    /// `omr_keygen_seeded_key`: the bodies of the key whose masks come from the public `mask_seed`.
    pub fn generate_seeded_key(&self, seed: u64, mask_seed: u64, nthreads: i32) -> Result<SeededKey, OmrError> {
        let mut k = SeededKey { bsk1_b: vec![0; BSK1_B_LEN], ksk_b: vec![0; KSK_B_LEN], bsk2_b: vec![0; BSK2_B_LEN],
                                trace_key_b: vec![0; TRACE_KEY_B_LEN], mask_seed };
        check(unsafe {
            omr_keygen_seeded_key(self.raw, seed, mask_seed, k.bsk1_b.as_mut_ptr(), k.ksk_b.as_mut_ptr(),
                                  k.bsk2_b.as_mut_ptr(), k.trace_key_b.as_mut_ptr(), nthreads)
        })?;
        Ok(k)
    }
    /// `Sender::gen_clues` (sender.rs:27-32) for global message indices `first..first + count`.
    pub fn gen_clues(&self, seed: u64, first: u64, count: usize) -> Result<Vec<Clue>, OmrError> {
        let mut a = vec![0u16; count * OMR_N0];
        let mut b = vec![0u16; count * OMR_CLUE_COUNT];
        check(unsafe { omr_gen_clues(self.raw, seed, first, count, a.as_mut_ptr(), b.as_mut_ptr(), 0) })?;
        Ok((0..count)
            .map(|m| {
                let mut c = Clue { a: [0; OMR_N0], b: [0; OMR_CLUE_COUNT] };
                c.a.copy_from_slice(&a[m * OMR_N0..(m + 1) * OMR_N0]);
                c.b.copy_from_slice(&b[m * OMR_CLUE_COUNT..(m + 1) * OMR_CLUE_COUNT]);
                c
            })
            .collect())
    }
}

impl Drop for SecretKeyPack {
    fn drop(&mut self) {
        unsafe { omr_secret_destroy(self.raw) }
    }
}

/// `ClueKey` (key_gen/clue.rs): the public key a sender needs, 2,048 bytes.
pub type ClueKey = OmrClueKey;

impl SecretKeyPack {
    /// `SecretKeyPack::generate_clue_key` (secret.rs:99-107).
    pub fn generate_clue_key(&self) -> Result<ClueKey, OmrError> {
        let mut k = ClueKey { a: [0; OMR_N0], b: [0; OMR_N0] };
        check(unsafe { omr_secret_clue_key(self.raw, &mut k) })?;
        Ok(k)
    }
    /// `SecretKeyPack::decrypt_clue` (secret.rs:267-270) for every clue of every message: whether the message
    /// is pertinent (all seven values zero), per message.
    pub fn open_clues(&self, clues: &[Clue]) -> Result<Vec<bool>, OmrError> {
        let a: Vec<u16> = clues.iter().flat_map(|c| c.a.iter().copied()).collect();
        let b: Vec<u16> = clues.iter().flat_map(|c| c.b.iter().copied()).collect();
        let mut p = vec![0u8; clues.len()];
        check(unsafe {
            omr_clue_open(self.raw, a.as_ptr(), b.as_ptr(), clues.len(), std::ptr::null_mut(), p.as_mut_ptr(),
                          std::ptr::null_mut(), 0)
        })?;
        Ok(p.into_iter().map(|x| x != 0).collect())
    }
}

/// `Sender` (sender.rs:27-32) over a table of clue keys: message `m` of a call is addressed to key
/// `recipient[m]`. CPU entry; a sender created with a device also serves `omr_sender_gen_clues_device`.
pub struct Sender {
    raw: *mut OmrSender,
}
unsafe impl Send for Sender {}

impl Sender {
    /// `Sender::new(clue_key, 7)` for one or more recipients; `device` None: CPU only.
    pub fn new(keys: &[ClueKey], device: Option<i32>) -> Result<Self, OmrError> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { omr_sender_create(keys.as_ptr(), keys.len(), device.unwrap_or(-1), &mut raw) })?;
        Ok(Self { raw })
    }
    /// `Sender::gen_clues` for global message indices `first..first + recipient.len()`.
    pub fn gen_clues(&self, recipient: &[u32], seed: u64, first: u64) -> Result<Vec<Clue>, OmrError> {
        let count = recipient.len();
        let mut a = vec![0u16; count * OMR_N0];
        let mut b = vec![0u16; count * OMR_CLUE_COUNT];
        check(unsafe {
            omr_sender_gen_clues(self.raw, recipient.as_ptr(), seed, first, count, a.as_mut_ptr(), b.as_mut_ptr(), 0)
        })?;
        Ok((0..count)
            .map(|m| {
                let mut c = Clue { a: [0; OMR_N0], b: [0; OMR_CLUE_COUNT] };
                c.a.copy_from_slice(&a[m * OMR_N0..(m + 1) * OMR_N0]);
                c.b.copy_from_slice(&b[m * OMR_CLUE_COUNT..(m + 1) * OMR_CLUE_COUNT]);
                c
            })
            .collect())
    }
    pub fn raw(&self) -> *mut OmrSender {
        self.raw
    }
}

impl Drop for Sender {
    fn drop(&mut self) {
        unsafe { omr_sender_destroy(self.raw) }
    }
}

/// `DetectTimeInfo` (detector.rs:51-57): summed device time per stage of a detect batch.
#[derive(Debug, Clone, Copy, Default)]
pub struct DetectTimeInfo {
    pub total_detect_time: Duration,
    /// 7 level-1 rotations + sum + key switch + modulus switch (detector.rs:183-189)
    pub total_first_level_bootstrapping_time: Duration,
    /// level-2 blind rotation (detector.rs:193-198)
    pub total_second_level_bootstrapping_time: Duration,
    /// hom_trace + NTT (detector.rs:202-209)
    pub total_trace_time: Duration,
}

impl From<OmrDetectTiming> for DetectTimeInfo {
    fn from(t: OmrDetectTiming) -> Self {
        let ms = |v: f32| Duration::from_secs_f64(f64::from(v.max(0.0)) * 1e-3);
        Self {
            total_detect_time: ms(t.total_ms),
            total_first_level_bootstrapping_time: ms(t.first_level_ms),
            total_second_level_bootstrapping_time: ms(t.second_level_ms),
            total_trace_time: ms(t.trace_ms),
        }
    }
}

/// `Detector` on one MI355X: owns the device-resident evaluation keys.
pub struct GpuDetector {
    ctx: *mut OmrCtx,
}
// Calls on one context are serialised inside the library; contexts are independent.
unsafe impl Send for GpuDetector {}
unsafe impl Sync for GpuDetector {}

impl GpuDetector {
    /// `Detector::new` (detector.rs:85-110): uploads the keys to `device` and converts them.
    pub fn new(key: &DetectionKey, device: i32) -> Result<Self, OmrError> {
        if key.bsk1.len() != BSK1_LEN || key.ksk.len() != KSK_LEN || key.bsk2.len() != BSK2_LEN
            || key.trace_key.len() != TRACE_KEY_LEN
        {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "detection key sizes".into() });
        }
        let view = OmrDetectionKeyView { bsk1: key.bsk1.as_ptr(), ksk: key.ksk.as_ptr(), bsk2: key.bsk2.as_ptr(),
                                         trace_key: key.trace_key.as_ptr() };
        let mut ctx = std::ptr::null_mut();
        check(unsafe { omr_ctx_create(&view, device, &mut ctx) })?;
        Ok(Self { ctx })
    }

    /// The same detector from a seeded key (`omr_ctx_create_seeded`): the key is expanded on `device`
    /// and the expanded copy freed before this returns.
    pub fn from_seeded_key(key: &SeededKey, device: i32) -> Result<Self, OmrError> {
        let view = key.view()?;
        let mut ctx = std::ptr::null_mut();
        check(unsafe { omr_ctx_create_seeded(&view, device, &mut ctx) })?;
        Ok(Self { ctx })
    }

    /// `Detector::detect` (detector.rs:135-138): one clue set, a batch of one.
    pub fn detect(&self, clue: &Clue) -> Result<NttRlwe, OmrError> {
        // omr_detect coalesces concurrent callers (e.g. rayon's par_iter over a shared &Detector,
        // examples/omr.rs:160-164) into batched launches
        let mut out = vec![0u64; 2 * OMR_N2];
        check(unsafe { omr_detect(self.ctx, clue.a.as_ptr(), clue.b.as_ptr(), out.as_mut_ptr()) })?;
        Ok(NttRlwe::from_flat(&out))
    }

    /// `clues.par_iter().map(|c| detector.detect(c))` (examples/omr.rs:160-164) in one call.
    pub fn detect_batch(&self, clues: &[Clue]) -> Result<Vec<NttRlwe>, OmrError> {
        let d = clues.len();
        let mut a = Vec::with_capacity(d * OMR_N0);
        let mut b = Vec::with_capacity(d * OMR_CLUE_COUNT);
        for c in clues {
            a.extend_from_slice(&c.a);
            b.extend_from_slice(&c.b);
        }
        let mut out = vec![0u64; d * 2 * OMR_N2];
        check(unsafe { omr_detect_batch(self.ctx, a.as_ptr(), b.as_ptr(), d, out.as_mut_ptr()) })?;
        Ok(out.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect())
    }

    /// `Detector::detect_with_time_info` (detector.rs:169-221) over a batch: detect and the stage
    /// times in one call under the context's lock (safe with concurrent callers).
    pub fn detect_with_time_info(&self, clues: &[Clue]) -> Result<(Vec<NttRlwe>, DetectTimeInfo), OmrError> {
        let d = clues.len();
        let mut a = Vec::with_capacity(d * OMR_N0);
        let mut b = Vec::with_capacity(d * OMR_CLUE_COUNT);
        for c in clues {
            a.extend_from_slice(&c.a);
            b.extend_from_slice(&c.b);
        }
        let mut out = vec![0u64; d * 2 * OMR_N2];
        let mut t = OmrDetectTiming::default();
        check(unsafe { omr_detect_with_time_info(self.ctx, a.as_ptr(), b.as_ptr(), d, out.as_mut_ptr(), &mut t) })?;
        Ok((out.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect(), t.into()))
    }

    /// Waits for `hip_stream` (null = the whole device) and reports a failed earlier device
    /// call on this context (`omr_ctx_check`); callers of the device entry points use it.
    pub fn check(&self, hip_stream: *mut c_void) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_check(self.ctx, hip_stream) })
    }

    /// `Detector::encode_pertinent_indices` (detector.rs:223-227) for index ciphertext `ct` of the
    /// board; the buckets come from `seed` (the reference draws them from thread_rng, :262).
    pub fn encode_pertinent_indices(&self, rp: &RetrievalParams, pertinency_vector: &[NttRlwe], seed: u64,
                                    ct: u32) -> Result<NttRlwe, OmrError> {
        self.encode_pertinent_indices_shard(rp, pertinency_vector, 0, seed, ct)
    }

    /// The same over the board's messages `global_offset..global_offset + pv.len()` (one shard of
    /// a multi-GPU job; the partial digests are summed mod q2).
    pub fn encode_pertinent_indices_shard(&self, rp: &RetrievalParams, pertinency_vector: &[NttRlwe],
                                          global_offset: usize, seed: u64, ct: u32) -> Result<NttRlwe, OmrError> {
        let pv = NttRlwe::flatten(pertinency_vector);
        let mut out = vec![0u64; 2 * OMR_N2];
        check(unsafe {
            omr_encode_indices(self.ctx, pv.as_ptr(), pertinency_vector.len(), global_offset, rp.all_payloads_count,
                               seed, ct, out.as_mut_ptr())
        })?;
        Ok(NttRlwe::from_flat(&out))
    }

    /// The board's bitmap digest (`omr_encode_bitmap`, none in the reference) over the messages
    /// `global_offset..global_offset + pv.len()`: `bitmap_ct_count(all)` ciphertexts from which
    /// `Retriever::decode_bitmap` reads every pertinent index without knowing their number. Partial
    /// digests of shards are summed mod q2.
    pub fn encode_bitmap(&self, pertinency_vector: &[NttRlwe], global_offset: usize,
                         all_payloads_count: usize) -> Result<Vec<NttRlwe>, OmrError> {
        let pv = NttRlwe::flatten(pertinency_vector);
        let mut out = vec![0u64; bitmap_ct_count(all_payloads_count)? * 2 * OMR_N2];
        check(unsafe {
            omr_encode_bitmap(self.ctx, pv.as_ptr(), pertinency_vector.len(), global_offset, all_payloads_count,
                              out.as_mut_ptr())
        })?;
        Ok(out.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect())
    }

    /// Ciphertexts in compact form through the device (`omr_compact_cts`): `512 * bits` bytes each, the
    /// bits of `compact_cts_cpu`.
    pub fn compact_cts(&self, cts: &[NttRlwe], bits: i32) -> Result<Vec<u8>, OmrError> {
        let flat = NttRlwe::flatten(cts);
        let mut out = vec![0u8; cts.len() * compact_ct_bytes(bits)?];
        check(unsafe { omr_compact_cts(self.ctx, flat.as_ptr(), cts.len(), bits as c_int, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }

    /// The same on device buffers (`omr_compact_cts_device`), enqueued on `hip_stream`.
    ///
    /// # Safety
    /// `d_cts` must be device memory of `n` ciphertexts and `d_out` of `n * 512 * bits` bytes, both
    /// 16-byte aligned and valid until the stream has run the work.
    pub unsafe fn compact_cts_device(&self, d_cts: *const u64, n: usize, bits: i32, d_out: *mut c_void,
                                     hip_stream: *mut c_void) -> Result<(), OmrError> {
        check(omr_compact_cts_device(self.ctx, d_cts, n, bits as c_int, d_out, hip_stream))
    }

    /// Knobs of the compact kernel (`omr_ctx_set_compact_grid`, `omr_ctx_set_compact_staging`; 0 =
    /// default); the results do not depend on them.
    pub fn set_compact_knobs(&self, workgroups: u32, max_ciphertexts: usize) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_set_compact_grid(self.ctx, workgroups as c_uint) })?;
        check(unsafe { omr_ctx_set_compact_staging(self.ctx, max_ciphertexts) })
    }

    /// `encode_bitmap` on device buffers (`omr_encode_bitmap_device`), enqueued on `hip_stream`.
    ///
    /// # Safety
    /// `d_pv` must be device memory of `d` pertinency ciphertexts (16-byte aligned) and `d_out` of
    /// `bitmap_ct_count(all)` ciphertexts, both valid until the stream has run the call.
    pub unsafe fn encode_bitmap_device(&self, d_pv: *const u64, d: usize, global_offset: usize,
                                       all_payloads_count: usize, d_out: *mut u64,
                                       hip_stream: *mut c_void) -> Result<(), OmrError> {
        check(omr_encode_bitmap_device(self.ctx, d_pv, d, global_offset, all_payloads_count, d_out, hip_stream))
    }

    /// `Detector::encode_pertinent_payloads` (detector.rs:341-350) with the 32-byte seed of
    /// `StdRng::from_seed` (same weights; the retriever regenerates them, retriever.rs:215-240).
    pub fn encode_pertinent_payloads(&self, pertinency_vector: &[NttRlwe], payloads: &[Payload],
                                     rp: &RetrievalParams, seed: &[u8; 32]) -> Result<Vec<NttRlwe>, OmrError> {
        if payloads.len() != pertinency_vector.len() {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "one payload per message".into() });
        }
        let w = payload_weights(seed, rp)?;
        let pv = NttRlwe::flatten(pertinency_vector);
        let pay: Vec<u16> = payloads.iter().flat_map(|p| p.iter().copied()).collect();
        let n_ct = rp.layout.cmb_cipher_count;
        let mut out = vec![0u64; n_ct as usize * 2 * OMR_N2];
        check(unsafe {
            omr_encode_payloads(self.ctx, pv.as_ptr(), pay.as_ptr(), pertinency_vector.len(), 0,
                                rp.all_payloads_count, w.as_ptr(), n_ct, rp.layout.cmb_count_per_cipher,
                                out.as_mut_ptr())
        })?;
        Ok(out.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect())
    }

    /// `encode_pertinent_payloads` with indexed weights (`omr_encode_payloads_indexed`): the weights are
    /// computed in the kernel from `seed`, no board-wide table is drawn or uploaded. The pertinency vector
    /// covers the messages `global_offset..` of the board.
    pub fn encode_pertinent_payloads_indexed(&self, pertinency_vector: &[NttRlwe], payloads: &[Payload],
                                             rp: &RetrievalParams, seed: &[u8; 32],
                                             global_offset: usize) -> Result<Vec<NttRlwe>, OmrError> {
        if payloads.len() != pertinency_vector.len() {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "one payload per message".into() });
        }
        let pv = NttRlwe::flatten(pertinency_vector);
        let pay: Vec<u16> = payloads.iter().flat_map(|p| p.iter().copied()).collect();
        let n_ct = rp.layout.cmb_cipher_count;
        let mut out = vec![0u64; n_ct as usize * 2 * OMR_N2];
        check(unsafe {
            omr_encode_payloads_indexed(self.ctx, pv.as_ptr(), pay.as_ptr(), pertinency_vector.len(), global_offset,
                                        rp.all_payloads_count, seed.as_ptr(), rp.layout.combination_count, 0, n_ct,
                                        rp.layout.cmb_count_per_cipher, out.as_mut_ptr())
        })?;
        Ok(out.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect())
    }

    /// The same on device buffers for the ciphertexts `first_ct..first_ct + n_ct`
    /// (`omr_encode_payloads_indexed_device`): returns once enqueued.
    ///
    /// # Safety
    /// The pointers must be device memory of the detector's GPU in the ABI layouts (`d_out` of
    /// `n_ct` ciphertexts) and stay valid until the stream has finished.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn encode_payloads_indexed_device(&self, d_pv: *const u64, d_payloads: *const u16, d: usize,
                                                 global_offset: usize, rp: &RetrievalParams, seed: &[u8; 32],
                                                 first_ct: u32, n_ct: u32, d_out: *mut u64,
                                                 hip_stream: *mut c_void) -> Result<(), OmrError> {
        check(omr_encode_payloads_indexed_device(self.ctx, d_pv, d_payloads, d, global_offset, rp.all_payloads_count,
                                                 seed.as_ptr(), rp.layout.combination_count, first_ct, n_ct,
                                                 rp.layout.cmb_count_per_cipher, d_out, hip_stream))
    }

    /// Messages per internal detect chunk (0 = default).
    pub fn set_batch(&self, batch: usize) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_set_batch(self.ctx, batch) })
    }

    /// At most `max_chunks` partial digests per encode ciphertext (0 = default 4,096).
    pub fn set_encode_chunks(&self, max_chunks: usize) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_set_encode_chunks(self.ctx, max_chunks) })
    }

    /// Coalescing of concurrent `detect` callers (`omr_ctx_set_coalescing`): at most
    /// `max_messages` per combined launch (0 = 65,536), launching after `window_us` microseconds.
    pub fn set_coalescing(&self, max_messages: usize, window_us: i64) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_set_coalescing(self.ctx, max_messages, window_us as c_long) })
    }

    /// Rounding-margin guard of the FFT external products (`omr_ctx_set_rounding_guard`).
    pub fn set_rounding_guard(&self, enable: bool) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_set_rounding_guard(self.ctx, enable as c_int) })
    }

    /// (observed margins, a priori bounds) per level (`omr_ctx_rounding_margin`): a guarded run is
    /// exact when observed < 1 - apriori (and every run when apriori < 0.5).
    pub fn rounding_margin(&self, reset: bool) -> Result<([f64; 2], [f64; 2]), OmrError> {
        let (mut obs, mut apr) = ([0f64; 2], [0f64; 2]);
        check(unsafe {
            omr_ctx_rounding_margin(self.ctx, obs.as_mut_ptr(), apr.as_mut_ptr(), std::ptr::null_mut(), reset as c_int)
        })?;
        Ok((obs, apr))
    }

    /// The exactness contract (`omr_ctx_exactness`): (guarded on every launch, breaching launches)
    /// per level. A level whose a priori bound is >= 0.5 is guarded automatically; a breach on
    /// either level was re-run on the exact NTT (level 1: br1n_fallback_kernel; level 2:
    /// br2l_fallback_kernel + trace_fallback_kernel).
    pub fn exactness(&self) -> Result<([bool; 2], [u64; 2]), OmrError> {
        let (mut g, mut b) = ([0 as c_int; 2], [0u64; 2]);
        check(unsafe { omr_ctx_exactness(self.ctx, g.as_mut_ptr(), b.as_mut_ptr()) })?;
        Ok(([g[0] != 0, g[1] != 0], b))
    }

    /// The launch record (`omr_ctx_launch_record`): cumulative launches per level-2 rotation / trace
    /// kernel since creation, indexed by the `OMR_LAUNCH_*` constants. Host counters.
    pub fn launch_record(&self) -> Result<[u64; OMR_LAUNCH_COUNT], OmrError> {
        let mut counts = [0u64; OMR_LAUNCH_COUNT];
        check(unsafe { omr_ctx_launch_record(self.ctx, counts.as_mut_ptr()) })?;
        Ok(counts)
    }

    /// Chunks of at most `max_messages` messages run the latency kernels (0 = never).
    pub fn set_latency_threshold(&self, max_messages: usize) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_set_latency_threshold(self.ctx, max_messages) })
    }

    /// Level 1 on the exact modular NTT for every launch (`omr_ctx_set_exact_level1`): the
    /// reference's arithmetic, bit-identical outputs, slower.
    pub fn set_exact_level1(&self, enable: bool) -> Result<(), OmrError> {
        check(unsafe { omr_ctx_set_exact_level1(self.ctx, enable as c_int) })
    }
}

impl Drop for GpuDetector {
    fn drop(&mut self) {
        unsafe { omr_ctx_destroy(self.ctx) }
    }
}

/// The digest of a board: the index ciphertexts and the payload ciphertexts that
/// `Retriever::decode_digest` takes (retriever.rs:188-260).
pub struct Digest {
    pub indices: Vec<NttRlwe>,
    pub payloads: Vec<NttRlwe>,
}

/// A digest session (`omr_digest_*`): the board flow of `examples/omr.rs:160-203`, detect every
/// message, `encode_pertinent_indices` per index ciphertext, `encode_pertinent_payloads`, run piece
/// by piece inside the library with the running digest on the device. No pertinency vector crosses
/// the boundary, and the library never holds more than one detect chunk of it. Message ranges may
/// arrive in any order and any sizes; every partition gives the same digest. The borrow keeps the
/// detector (the context) alive for as long as the session.
pub struct DigestSession<'a> {
    raw: *mut OmrDigest,
    _detector: &'a GpuDetector,
}
// Calls on one session are serialised inside the library.
unsafe impl Send for DigestSession<'_> {}
unsafe impl Sync for DigestSession<'_> {}

impl GpuDetector {
    /// `omr_digest_begin` for a board of `rp.all_payloads_count` messages: `index_seed` as in
    /// `encode_pertinent_indices`, `weight_seed` as in `encode_pertinent_payloads`; the work runs on
    /// HIP's null stream.
    pub fn digest_session(&self, rp: &RetrievalParams, index_seed: u64,
                          weight_seed: &[u8; 32]) -> Result<DigestSession<'_>, OmrError> {
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            omr_digest_begin(self.ctx, rp.all_payloads_count, rp.pertinent_count, index_seed, weight_seed.as_ptr(),
                             std::ptr::null_mut(), &mut raw)
        })?;
        Ok(DigestSession { raw, _detector: self })
    }

    /// `omr_digest_begin_indexed`: the same session with indexed payload weights. It draws and holds no
    /// weight table; its digest is retrieved with `Retriever::decode_digest_indexed`.
    pub fn digest_session_indexed(&self, rp: &RetrievalParams, index_seed: u64,
                                  weight_seed: &[u8; 32]) -> Result<DigestSession<'_>, OmrError> {
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            omr_digest_begin_indexed(self.ctx, rp.all_payloads_count, rp.pertinent_count, index_seed,
                                     weight_seed.as_ptr(), std::ptr::null_mut(), &mut raw)
        })?;
        Ok(DigestSession { raw, _detector: self })
    }

    /// `omr_digest_begin_seek`: the default session's digest without its weight table. The session scans the
    /// reference's stream for its rejections on the device at begin; `Retriever::decode_digest` or
    /// `decode_digest_seek` retrieves it.
    pub fn digest_session_seek(&self, rp: &RetrievalParams, index_seed: u64,
                               weight_seed: &[u8; 32]) -> Result<DigestSession<'_>, OmrError> {
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            omr_digest_begin_seek(self.ctx, rp.all_payloads_count, rp.pertinent_count, index_seed,
                                  weight_seed.as_ptr(), std::ptr::null_mut(), &mut raw)
        })?;
        Ok(DigestSession { raw, _detector: self })
    }
}

impl DigestSession<'_> {
    /// Folds the messages `global_offset..global_offset + clues.len()` in (`omr_digest_update`);
    /// returns when the device has finished with them.
    pub fn update(&self, clues: &[Clue], payloads: &[Payload], global_offset: usize) -> Result<(), OmrError> {
        if payloads.len() != clues.len() {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "one payload per message".into() });
        }
        let d = clues.len();
        let mut a = Vec::with_capacity(d * OMR_N0);
        let mut b = Vec::with_capacity(d * OMR_CLUE_COUNT);
        for c in clues {
            a.extend_from_slice(&c.a);
            b.extend_from_slice(&c.b);
        }
        let pay: Vec<u16> = payloads.iter().flat_map(|p| p.iter().copied()).collect();
        check(unsafe { omr_digest_update(self.raw, a.as_ptr(), b.as_ptr(), pay.as_ptr(), d, global_offset) })
    }

    /// The same on device buffers of the detector's GPU (`omr_digest_update_device`): returns once
    /// enqueued.
    ///
    /// # Safety
    /// The pointers must be device memory of `d` messages in the ABI layouts and stay valid until
    /// `read` or `GpuDetector::check` has returned.
    pub unsafe fn update_device(&self, d_clue_a: *const u16, d_clue_b: *const u16, d_payloads: *const u16, d: usize,
                                global_offset: usize) -> Result<(), OmrError> {
        check(omr_digest_update_device(self.raw, d_clue_a, d_clue_b, d_payloads, d, global_offset))
    }

    /// Adds another session's digest (e.g. another GPU's shard of the board) mod q2.
    pub fn merge(&self, other: &Digest) -> Result<(), OmrError> {
        let info = self.info()?;
        if other.indices.len() != info.index_ct as usize || other.payloads.len() != info.payload_ct as usize {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "digest of another layout".into() });
        }
        let (idx, pay) = (NttRlwe::flatten(&other.indices), NttRlwe::flatten(&other.payloads));
        check(unsafe { omr_digest_merge(self.raw, idx.as_ptr(), pay.as_ptr()) })
    }

    /// Waits for the session's work and returns the digest so far (`omr_digest_read`).
    pub fn read(&self) -> Result<Digest, OmrError> {
        let info = self.info()?;
        let mut idx = vec![0u64; info.index_ct as usize * 2 * OMR_N2];
        let mut pay = vec![0u64; info.payload_ct as usize * 2 * OMR_N2];
        check(unsafe { omr_digest_read(self.raw, idx.as_mut_ptr(), pay.as_mut_ptr()) })?;
        Ok(Digest { indices: idx.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect(),
                    payloads: pay.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect() })
    }

    /// (bytes of device memory the session owns now, the weight table's share of them)
    /// (`omr_digest_device_bytes`); the share of an indexed session is 0.
    pub fn device_bytes(&self) -> Result<(usize, usize), OmrError> {
        let (mut total, mut weights) = (0usize, 0usize);
        check(unsafe { omr_digest_device_bytes(self.raw, &mut total, &mut weights) })?;
        Ok((total, weights))
    }

    /// Also keep the board's bitmap digest (`omr_digest_enable_bitmap`); before the first update or
    /// merge, a second call is a no-op.
    pub fn enable_bitmap(&self) -> Result<(), OmrError> {
        check(unsafe { omr_digest_enable_bitmap(self.raw) })
    }

    /// Waits for the session's work and returns the bitmap digest so far (`omr_digest_read_bitmap`).
    pub fn read_bitmap(&self) -> Result<Vec<NttRlwe>, OmrError> {
        let mut out = vec![0u64; bitmap_ct_count(self.info()?.all_payloads_count)? * 2 * OMR_N2];
        check(unsafe { omr_digest_read_bitmap(self.raw, out.as_mut_ptr()) })?;
        Ok(out.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect())
    }

    /// Adds another session's `read_bitmap` output mod q2 (`omr_digest_merge_bitmap`).
    pub fn merge_bitmap(&self, other: &[NttRlwe]) -> Result<(), OmrError> {
        if other.len() != bitmap_ct_count(self.info()?.all_payloads_count)? {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "bitmap of another board".into() });
        }
        let cts = NttRlwe::flatten(other);
        check(unsafe { omr_digest_merge_bitmap(self.raw, cts.as_ptr()) })
    }

    /// The digest at `bits` bits per coefficient (`omr_digest_read_compact`): the index and payload
    /// ciphertexts, and the bitmap's when `bitmap` is set, `512 * bits` bytes each. The running digest is
    /// not modified.
    pub fn read_compact(&self, bits: i32, bitmap: bool) -> Result<CompactDigest, OmrError> {
        let info = self.info()?;
        let ctb = compact_ct_bytes(bits)?;
        let mut indices = vec![0u8; info.index_ct as usize * ctb];
        let mut payloads = vec![0u8; info.payload_ct as usize * ctb];
        let mut bmp = vec![0u8; if bitmap { bitmap_ct_count(info.all_payloads_count)? * ctb } else { 0 }];
        let p_bmp = if bitmap { bmp.as_mut_ptr() as *mut c_void } else { std::ptr::null_mut() };
        check(unsafe {
            omr_digest_read_compact(self.raw, bits as c_int, indices.as_mut_ptr() as *mut c_void,
                                    payloads.as_mut_ptr() as *mut c_void, p_bmp)
        })?;
        Ok(CompactDigest { bits, indices, payloads, bitmap: bmp })
    }

    pub fn info(&self) -> Result<OmrDigestInfo, OmrError> {
        let mut info = OmrDigestInfo::default();
        check(unsafe { omr_digest_get_info(self.raw, &mut info) })?;
        Ok(info)
    }
}

impl Drop for DigestSession<'_> {
    fn drop(&mut self) {
        unsafe { omr_digest_destroy(self.raw) }
    }
}

/// A digest in compact form (`omr_digest_read_compact`): `512 * bits` bytes per ciphertext; `bitmap` is
/// empty when it was not asked for.
pub struct CompactDigest {
    pub bits: i32,
    pub indices: Vec<u8>,
    pub payloads: Vec<u8>,
    pub bitmap: Vec<u8>,
}

/// Bytes of one compact ciphertext, `512 * bits` (`omr_compact_ct_bytes`); `bits` in 16..=32.
pub fn compact_ct_bytes(bits: i32) -> Result<usize, OmrError> {
    let mut n = 0usize;
    check(unsafe { omr_compact_ct_bytes(bits as c_int, &mut n) })?;
    Ok(n)
}

/// Compact ciphertexts on the CPU (`omr_compact_cts_cpu`): `512 * bits` bytes per ciphertext.
pub fn compact_cts_cpu(cts: &[NttRlwe], bits: i32, nthreads: i32) -> Result<Vec<u8>, OmrError> {
    let flat = NttRlwe::flatten(cts);
    let mut out = vec![0u8; cts.len() * compact_ct_bytes(bits)?];
    check(unsafe { omr_compact_cts_cpu(flat.as_ptr(), cts.len(), bits as c_int, out.as_mut_ptr() as *mut c_void, nthreads) })?;
    Ok(out)
}

/// Compact ciphertexts back to `NttRlwe` on the CPU (`omr_compact_expand_cpu`).
pub fn compact_expand_cpu(packed: &[u8], bits: i32, nthreads: i32) -> Result<Vec<NttRlwe>, OmrError> {
    let ctb = compact_ct_bytes(bits)?;
    if packed.len() % ctb != 0 {
        return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "512 * bits bytes per compact ciphertext".into() });
    }
    let n = packed.len() / ctb;
    let mut out = vec![0u64; n * 2 * OMR_N2];
    check(unsafe { omr_compact_expand_cpu(packed.as_ptr() as *const c_void, n, bits as c_int, out.as_mut_ptr(), nthreads) })?;
    Ok(out.chunks_exact(2 * OMR_N2).map(NttRlwe::from_flat).collect())
}

/// R(bits) for the pack's second-level key (`omr_compact_residual_bound`): decoding a compacted
/// ciphertext is proven correct when its largest residual before compaction plus R is at most (q2 - 1) / 2.
pub fn compact_residual_bound(secret: &SecretKeyPack, bits: i32) -> Result<u64, OmrError> {
    let mut r = 0u64;
    check(unsafe { omr_compact_residual_bound(secret.raw, bits as c_int, &mut r) })?;
    Ok(r)
}

/// Bitmap ciphertexts of a board, `ceil(all / 16384)` (`omr_bitmap_ct_count`).
pub fn bitmap_ct_count(all_payloads_count: usize) -> Result<usize, OmrError> {
    let mut n = 0u32;
    check(unsafe { omr_bitmap_ct_count(all_payloads_count, &mut n) })?;
    Ok(n as usize)
}

/// Runs `call(indices, cap, found)`, and once more with room for `found` if `cap` was too small.
fn collect_indices(mut call: impl FnMut(*mut usize, usize, *mut usize) -> OmrStatus) -> Result<Vec<usize>, OmrError> {
    let mut buf = vec![0usize; 1024];
    loop {
        let mut found = 0usize;
        check(call(buf.as_mut_ptr(), buf.len(), &mut found))?;
        if found <= buf.len() {
            buf.truncate(found);
            return Ok(buf);
        }
        buf.resize(found, 0);
    }
}

/// The global indices of the set bits of decoded bitmap ciphertexts (`omr_bitmap_indices`):
/// `decoded` holds 2,048 values < 256 per ciphertext, e.g. `Audit::decoded`; increasing order.
pub fn bitmap_indices(decoded: &[u16], all_payloads_count: usize) -> Result<Vec<usize>, OmrError> {
    if decoded.len() % OMR_N2 != 0 {
        return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "2,048 decoded values per ciphertext".into() });
    }
    let n_ct = (decoded.len() / OMR_N2) as u32;
    collect_indices(|i, cap, found| unsafe { omr_bitmap_indices(decoded.as_ptr(), n_ct, all_payloads_count, i, cap, found) })
}

/// `Retriever::decode_digest` (retriever.rs:188-260) under the pack's second-level key.
pub struct Retriever<'a> {
    pub params: RetrievalParams,
    pub secret: &'a SecretKeyPack,
}

impl<'a> Retriever<'a> {
    /// Every pertinent index of the board, increasing, from its bitmap digest (`omr_retrieve_bitmap`):
    /// needs no pertinent count.
    pub fn decode_bitmap(&self, bitmap_digest: &[NttRlwe]) -> Result<Vec<usize>, OmrError> {
        let cts = NttRlwe::flatten(bitmap_digest);
        let (sk, n_ct, all) = (self.secret.raw, bitmap_digest.len() as u32, self.params.all_payloads_count);
        collect_indices(|i, cap, found| unsafe { omr_retrieve_bitmap(sk, cts.as_ptr(), n_ct, all, i, cap, found) })
    }

    /// Sorted pertinent indices and their payloads; `seed` is the payload-weight seed.
    pub fn decode_digest(&self, indices_digest: &[NttRlwe], payloads_digest: &[NttRlwe],
                         seed: &[u8; 32]) -> Result<(Vec<usize>, Vec<Payload>), OmrError> {
        let rp = self.params;
        let idx = NttRlwe::flatten(indices_digest);
        let mut found_buf = vec![0usize; rp.pertinent_count.max(1) * 4 + 64];
        let mut found = 0usize;
        check(unsafe {
            omr_retrieve_indices(self.secret.raw, idx.as_ptr(), indices_digest.len() as u32, rp.all_payloads_count,
                                 rp.pertinent_count, found_buf.as_mut_ptr(), found_buf.len(), &mut found)
        })?;
        found_buf.truncate(found.min(found_buf.len()));
        // the board's weights and combination count, whatever the number of indices found
        // (retriever.rs:196, :215-239)
        let w = payload_weights(seed, &rp)?;
        let pay = NttRlwe::flatten(payloads_digest);
        let mut out = vec![0u16; found_buf.len() * OMR_PAYLOAD_LEN];
        check(unsafe {
            omr_retrieve_payloads(self.secret.raw, pay.as_ptr(), payloads_digest.len() as u32, rp.all_payloads_count,
                                  rp.layout.combination_count, w.as_ptr(), found_buf.as_ptr(), found_buf.len(), out.as_mut_ptr())
        })?;
        let payloads = out
            .chunks_exact(OMR_PAYLOAD_LEN)
            .map(|c| {
                let mut p = [0u16; OMR_PAYLOAD_LEN];
                p.copy_from_slice(c);
                p
            })
            .collect();
        Ok((found_buf, payloads))
    }

    /// `decode_digest` for a digest encoded with indexed weights (`omr_retrieve_payloads_indexed`): the
    /// system's combination_count x found matrix is computed from `seed`, no board-wide table.
    pub fn decode_digest_indexed(&self, indices_digest: &[NttRlwe], payloads_digest: &[NttRlwe],
                                 seed: &[u8; 32]) -> Result<(Vec<usize>, Vec<Payload>), OmrError> {
        let rp = self.params;
        let idx = NttRlwe::flatten(indices_digest);
        let mut found_buf = vec![0usize; rp.pertinent_count.max(1) * 4 + 64];
        let mut found = 0usize;
        check(unsafe {
            omr_retrieve_indices(self.secret.raw, idx.as_ptr(), indices_digest.len() as u32, rp.all_payloads_count,
                                 rp.pertinent_count, found_buf.as_mut_ptr(), found_buf.len(), &mut found)
        })?;
        found_buf.truncate(found.min(found_buf.len()));
        let pay = NttRlwe::flatten(payloads_digest);
        let mut out = vec![0u16; found_buf.len() * OMR_PAYLOAD_LEN];
        check(unsafe {
            omr_retrieve_payloads_indexed(self.secret.raw, pay.as_ptr(), payloads_digest.len() as u32,
                                          rp.all_payloads_count, rp.layout.combination_count, seed.as_ptr(),
                                          found_buf.as_ptr(), found_buf.len(), out.as_mut_ptr())
        })?;
        let payloads = out
            .chunks_exact(OMR_PAYLOAD_LEN)
            .map(|c| {
                let mut p = [0u16; OMR_PAYLOAD_LEN];
                p.copy_from_slice(c);
                p
            })
            .collect();
        Ok((found_buf, payloads))
    }

    /// `decode_digest` without the weight table (`omr_retrieve_payloads_seek`): the reference's weights of
    /// the indices found, through `seek` or, with `None`, a seek built inside the call.
    pub fn decode_digest_seek(&self, indices_digest: &[NttRlwe], payloads_digest: &[NttRlwe], seed: &[u8; 32],
                              seek: Option<&OmrWeightSeek>) -> Result<(Vec<usize>, Vec<Payload>), OmrError> {
        let rp = self.params;
        let idx = NttRlwe::flatten(indices_digest);
        let mut found_buf = vec![0usize; rp.pertinent_count.max(1) * 4 + 64];
        let mut found = 0usize;
        check(unsafe {
            omr_retrieve_indices(self.secret.raw, idx.as_ptr(), indices_digest.len() as u32, rp.all_payloads_count,
                                 rp.pertinent_count, found_buf.as_mut_ptr(), found_buf.len(), &mut found)
        })?;
        found_buf.truncate(found.min(found_buf.len()));
        let pay = NttRlwe::flatten(payloads_digest);
        let mut out = vec![0u16; found_buf.len() * OMR_PAYLOAD_LEN];
        check(unsafe {
            omr_retrieve_payloads_seek(self.secret.raw, pay.as_ptr(), payloads_digest.len() as u32,
                                       rp.all_payloads_count, rp.layout.combination_count, seed.as_ptr(),
                                       seek.map_or(std::ptr::null(), |s| s as *const OmrWeightSeek),
                                       found_buf.as_ptr(), found_buf.len(), out.as_mut_ptr())
        })?;
        let payloads = out
            .chunks_exact(OMR_PAYLOAD_LEN)
            .map(|c| {
                let mut p = [0u16; OMR_PAYLOAD_LEN];
                p.copy_from_slice(c);
                p
            })
            .collect();
        Ok((found_buf, payloads))
    }
}

/// Class of an audited ciphertext (`omr_ct_audit`): all zeros, `[1, 0, .., 0]` (the omd KAT of a
/// pertinent message, omd.rs:48-58), or anything else.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum AuditClass {
    Zero,
    OneHot,
    Other,
}

impl OmrCtAudit {
    pub fn class(&self) -> AuditClass {
        match (self.nonzero, self.first) {
            (0, _) => AuditClass::Zero,
            (1, 1) => AuditClass::OneHot,
            _ => AuditClass::Other,
        }
    }
    /// Distance of the worst coefficient from its decode point in plaintext steps (0.5: a failure).
    pub fn max_residual(&self) -> f64 {
        self.max_abs_residual as f64 / OMR_Q2 as f64
    }
}

/// What an audit returns: one record and 2,048 decoded values mod 257 per ciphertext, and the
/// summary the call added into.
pub struct Audit {
    pub records: Vec<OmrCtAudit>,
    pub decoded: Vec<u16>,
    pub summary: OmrAuditSummary,
}

/// The auditor (`omr_auditor`): the level-2 secret on one device. Decrypts, classifies and
/// noise-audits `NttRlwe` ciphertexts (pertinency vectors, digests) on the GPU: the counterpart of
/// the reference's `NoiseSigmaInfo` (retriever.rs:390-560) in exact integers. The borrow keeps the
/// pack alive for `audit_cpu`.
pub struct Auditor<'a> {
    raw: *mut OmrAuditor,
    secret: &'a SecretKeyPack,
}
// Calls on one auditor are serialised inside the library.
unsafe impl Send for Auditor<'_> {}
unsafe impl Sync for Auditor<'_> {}

impl<'a> Auditor<'a> {
    pub fn new(secret: &'a SecretKeyPack, device: i32) -> Result<Self, OmrError> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { omr_auditor_create(secret.raw, device, &mut raw) })?;
        Ok(Self { raw, secret })
    }

    /// Workgroups of the kernel's grid (0 = default); the results do not depend on it.
    pub fn set_grid(&self, workgroups: u32) -> Result<(), OmrError> {
        check(unsafe { omr_auditor_set_grid(self.raw, workgroups as c_uint) })
    }

    /// Ciphertexts staged per piece by `audit` (0 = default 2,048); the results do not depend on it.
    pub fn set_staging(&self, max_ciphertexts: usize) -> Result<(), OmrError> {
        check(unsafe { omr_auditor_set_staging(self.raw, max_ciphertexts) })
    }

    /// Host ciphertexts through the device (`omr_audit`), added into `summary`.
    pub fn audit(&self, cts: &[NttRlwe], summary: &mut OmrAuditSummary) -> Result<Audit, OmrError> {
        let flat = NttRlwe::flatten(cts);
        let mut records = vec![OmrCtAudit::default(); cts.len()];
        let mut decoded = vec![0u16; cts.len() * OMR_N2];
        check(unsafe {
            omr_audit(self.raw, flat.as_ptr(), cts.len(), records.as_mut_ptr(), decoded.as_mut_ptr(), summary)
        })?;
        Ok(Audit { records, decoded, summary: *summary })
    }

    /// The same results on the CPU (`omr_audit_cpu`), on `nthreads` host threads (0: all, at most 16).
    pub fn audit_cpu(&self, cts: &[NttRlwe], summary: &mut OmrAuditSummary, nthreads: i32) -> Result<Audit, OmrError> {
        let flat = NttRlwe::flatten(cts);
        let mut records = vec![OmrCtAudit::default(); cts.len()];
        let mut decoded = vec![0u16; cts.len() * OMR_N2];
        check(unsafe {
            omr_audit_cpu(self.secret.raw, flat.as_ptr(), cts.len(), records.as_mut_ptr(), decoded.as_mut_ptr(),
                          summary, nthreads)
        })?;
        Ok(Audit { records, decoded, summary: *summary })
    }

    /// Compact ciphertexts in host memory, expanded and audited on the device (`omr_audit_compact`):
    /// the results of `audit` over their expansion, added into `summary`.
    pub fn audit_compact(&self, packed: &[u8], bits: i32, summary: &mut OmrAuditSummary) -> Result<Audit, OmrError> {
        let ctb = compact_ct_bytes(bits)?;
        if packed.len() % ctb != 0 {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "512 * bits bytes per compact ciphertext".into() });
        }
        let n = packed.len() / ctb;
        let mut records = vec![OmrCtAudit::default(); n];
        let mut decoded = vec![0u16; n * OMR_N2];
        check(unsafe {
            omr_audit_compact(self.raw, packed.as_ptr() as *const c_void, n, bits as c_int, records.as_mut_ptr(),
                              decoded.as_mut_ptr(), summary)
        })?;
        Ok(Audit { records, decoded, summary: *summary })
    }

    /// `omr_audit_key`: a detection key in host memory against the auditor's secret, staged through the
    /// device in pieces. One summary per component (`omr_key_component` order), started from
    /// `Default`; `limit` `None` is the generators' noise support. A key that passes has
    /// `rows_over == 0` in all four.
    pub fn audit_key(&self, key: &DetectionKey, limit: Option<[u64; 4]>) -> Result<[OmrKeyAuditSummary; 4], OmrError> {
        if key.bsk1.len() != BSK1_LEN || key.ksk.len() != KSK_LEN || key.bsk2.len() != BSK2_LEN
            || key.trace_key.len() != TRACE_KEY_LEN
        {
            return Err(OmrError { status: OMR_ERR_INVALID_ARGUMENT, message: "detection key sizes".into() });
        }
        let view = OmrDetectionKeyView { bsk1: key.bsk1.as_ptr(), ksk: key.ksk.as_ptr(), bsk2: key.bsk2.as_ptr(),
                                         trace_key: key.trace_key.as_ptr() };
        let mut out = [OmrKeyAuditSummary::default(); 4];
        let lim = limit.as_ref().map_or(std::ptr::null(), |l| l.as_ptr());
        check(unsafe { omr_audit_key(self.raw, &view, lim, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// `omr_audit_key_seeded`: the same for a seeded key, expanded on the device into temporaries.
    pub fn audit_seeded_key(&self, key: &SeededKey, limit: Option<[u64; 4]>) -> Result<[OmrKeyAuditSummary; 4], OmrError> {
        let view = key.view()?;
        let mut out = [OmrKeyAuditSummary::default(); 4];
        let lim = limit.as_ref().map_or(std::ptr::null(), |l| l.as_ptr());
        check(unsafe { omr_audit_key_seeded(self.raw, &view, lim, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// Device buffers of the auditor's GPU (`omr_compact_expand_device`): returns once enqueued.
    ///
    /// # Safety
    /// `d_packed` must be device memory of `n * 512 * bits` bytes and `d_cts` of `n` ciphertexts, both
    /// 16-byte aligned and valid until the stream has run the work.
    pub unsafe fn expand_device(&self, d_packed: *const c_void, n: usize, bits: i32, d_cts: *mut u64,
                                hip_stream: *mut c_void) -> Result<(), OmrError> {
        check(omr_compact_expand_device(self.raw, d_packed, n, bits as c_int, d_cts, hip_stream))
    }

    /// Device buffers of the auditor's GPU (`omr_audit_device`): returns once enqueued on `hip_stream`.
    ///
    /// # Safety
    /// `d_cts` must be device memory of `n` ciphertexts (u64 `[n][2][2048]`, 16-byte aligned); each
    /// output pointer is null or device memory of `n` records, `n * 2048` values, one summary (zeroed
    /// by the caller); not all three null. All must stay valid until the stream has run the work.
    pub unsafe fn audit_device(&self, d_cts: *const u64, n: usize, d_records: *mut OmrCtAudit, d_decoded: *mut u16,
                               d_summary: *mut OmrAuditSummary, hip_stream: *mut c_void) -> Result<(), OmrError> {
        check(omr_audit_device(self.raw, d_cts, n, d_records, d_decoded, d_summary, hip_stream))
    }
}

impl Drop for Auditor<'_> {
    fn drop(&mut self) {
        unsafe { omr_auditor_destroy(self.raw) }
    }
}

/// Library identification, e.g. "omr_gpu 0.1 gfx950".
pub fn version() -> String {
    unsafe { CStr::from_ptr(omr_version()) }.to_string_lossy().into_owned()
}
