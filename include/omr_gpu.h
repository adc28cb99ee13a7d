/*
 * omr_gpu.h — C ABI of the MI355X-native InstantOMR detector (libomr_gpu.so).
 *
 * This is the drop-in boundary for the detect path of xiangxiecrypto/tfhe-omr. Each entry
 * point names the reference interface it replaces (file:line under omr_core/src/). A Rust
 * caller binds these with `extern "C"` declarations; Python tests and
 * bench.py bind them with ctypes. Plain C: no exceptions cross the boundary, every call
 * returns an omr_status and omr_last_error() returns the thread-local message of the last
 * failure.
 *
 * Data conventions (identical to the parity oracle, oracle/omr_oracle.h):
 *  - RLWE (a, b), b = a*s + e + m over Z_q[X]/(X^N+1). LWE (a, b), b = <a,s> + e + m.
 *  - NTT domain: index j holds p(psi^(2*brv(j)+1)), psi = g^((q-1)/2N), g = 7 (q1), 22 (q2).
 *  - Keys cross the boundary in the COEFFICIENT domain, canonical residues in [0, q):
 *      bsk1      u32 [512][8][2][1024]   GGSW_{s1}(s0_i), rows 0..3 a-gadget, 4..7 b-gadget
 *      ksk       u32 [1024][27][671]     LWE_{s_int}(s1_i * 2^j): a[670], b
 *      bsk2      u64 [670][12][2][2048]  GGSW_{s2}(s_int_i), rows 0..5 a-gadget, 6..11 b-gadget
 *      trace_key u64 [11][25][2][2048]   step k (g = 2048/2^k + 1), digit j:
 *                                        (alpha, alpha*s2 + e - sigma_g(s2) * 4^j)
 *    GGSW(m) row k = (alpha_k + m*g_k, alpha_k*s + e_k); row d+k = (alpha', alpha'*s + e' + m*g_k),
 *    gadget g_k = 2^(drop + k*logB): BR1 (logB 5, d 4, drop 7), BR2 (logB 7, d 6, drop 8).
 *  - A clue (CmLweCiphertext<u16>) is mask a[512] and bodies b[7], values mod 2048.
 *  - A pertinency ciphertext (NttRlweCiphertext<SecondLevelField>) is u64 [2][2048] (a then b),
 *    NTT domain, canonical residues mod q2.
 */
#ifndef OMR_GPU_H
#define OMR_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter set: omr_core/src/parameters/mod.rs:39-105 */
#define OMR_N0 512
#define OMR_Q0 2048
#define OMR_CLUE_COUNT 7
#define OMR_Q1 134215681u
#define OMR_N1 1024
#define OMR_KS_DIGITS 27
#define OMR_NI 670
#define OMR_QI 4096
#define OMR_Q2 1125899906826241ull
#define OMR_N2 2048
#define OMR_TRACE_STEPS 11
#define OMR_TRACE_DIGITS 25
#define OMR_P 257
#define OMR_PAYLOAD_LEN 612

typedef enum {
  OMR_OK = 0,
  OMR_ERR_INVALID_ARGUMENT = 1,
  OMR_ERR_DEVICE = 2,
  OMR_ERR_OUT_OF_MEMORY = 3,
  OMR_ERR_NOT_INVERTIBLE = 4 /* OmrError::InvertibleMatrix, error.rs:5-8 */
} omr_status;

/* Message of the last failing call on this thread ("" if none). */
const char *omr_last_error(void);
/* Library / build identification, e.g. "omr_gpu 0.1 gfx950". */
const char *omr_version(void);

/* ---------------------------------------------------------------------------------------
 * Key generation (CPU) — KeyGen::generate_secret_key (key_gen/mod.rs:21-27),
 * SecretKeyPack::new (key_gen/secret.rs:46-95), generate_sender (:110), generate_detection_key
 * (:118-178). Deterministic from a 64-bit seed (counter-based ChaCha12 streams per key row),
 * so every rank of a multi-GPU job derives identical keys.
 * ------------------------------------------------------------------------------------- */
typedef struct omr_secret_key_pack omr_secret_key_pack;

omr_status omr_keygen_secret(uint64_t seed, omr_secret_key_pack **out);
void omr_secret_destroy(omr_secret_key_pack *sk);
/* Secret material for client-side checks: s0 (512 bits), s1 (1024 ternary), s_int (670 bits),
 * s2 (2048 ternary). Any pointer may be NULL. */
omr_status omr_secret_export(const omr_secret_key_pack *sk, uint8_t *s0, int8_t *s1,
                             uint8_t *s_int, int8_t *s2);
/* DetectionKey in the coefficient-domain layout above. nthreads <= 0: all host cores. */
omr_status omr_keygen_detection_key(const omr_secret_key_pack *sk, uint64_t seed, uint32_t *bsk1,
                                    uint32_t *ksk, uint64_t *bsk2, uint64_t *trace_key,
                                    int nthreads);
/* Sender::gen_clues (sender.rs:27-32, key_gen/clue.rs:27-34): `count` clues (7 encryptions of 0
 * under the pack's RLWE-mode public key) for global message indices [first, first+count).
 * clue_a u16 [count][512], clue_b u16 [count][7]. */
omr_status omr_gen_clues(const omr_secret_key_pack *sk, uint64_t seed, uint64_t first,
                         size_t count, uint16_t *clue_a, uint16_t *clue_b, int nthreads);
/* Device generators: the same streams as omr_gen_clues /
 * omr_keygen_detection_key, bit-identical output, written to device buffers of the current HIP
 * device on `stream` (a hipStream_t; NULL = default stream). Both return after the stream has
 * completed the work. */
omr_status omr_gen_clues_device(const omr_secret_key_pack *sk, uint64_t seed, uint64_t first,
                                size_t count, uint16_t *d_clue_a, uint16_t *d_clue_b, void *stream);
omr_status omr_keygen_detection_key_device(const omr_secret_key_pack *sk, uint64_t seed,
                                           uint32_t *d_bsk1, uint32_t *d_ksk, uint64_t *d_bsk2,
                                           uint64_t *d_trace_key, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sender — SecretKeyPack::generate_clue_key (key_gen/secret.rs:99-107), Sender::new(clue_key, 7) and
 * Sender::gen_clues (sender.rs:27-32, key_gen/clue.rs:27-34), and the recipient's
 * SecretKeyPack::decrypt_clue (secret.rs:267-270). A sender holds public clue keys only; the generators
 * above take the recipient's pack and stay as they are.
 *
 * Generation. The clue of message m of a call is LwePublicKeyRlweMode::encrypt_multi_messages(&[0;7])
 * under key recipient[m]: u = A r + e1, v = B r + e2 over Z_2048[X]/(X^512 + 1), clue = (u, v[0..7]). Its
 * randomness is Stream(seed, DOM_CLUE = 20, first + m), the stream omr_gen_clues uses: r (16 words, bit b
 * of word k is r[32 k + b]), then the 512 Gaussians of e1, then the 7 of e2. So a sender over the one key
 * omr_secret_clue_key(sk) returns the bits of omr_gen_clues(sk, ..). The clue of a global index does not
 * depend on the range it is generated in, on the other messages' recipients or on nthreads. count = 0
 * does nothing. On the CPU an id >= n_keys returns OMR_ERR_INVALID_ARGUMENT before anything is written.
 * The device entry returns after the stream has finished the work, as omr_gen_clues_device does; if an
 * id was out of range it returns OMR_ERR_INVALID_ARGUMENT naming the smallest offending message index of
 * the call, that message's clue (and that of every other offending message) is not written, all other
 * clues are written, and the sender stays usable.
 *
 * Opening. Clue words are reduced mod 2048 first. For clue i of a message, phase_i = b_i - <a^(i), s0>
 * mod 2048 with a^(i) the extraction of detector.rs:514 (a^(i)[j] = a[i - j] for j <= i, -a[512 + i - j]
 * otherwise), value_i = ((8 phase_i + 1024) >> 11) & 7, noise_i = phase_i - 256 value_i centred into
 * [-128, 127], pertinent = (all seven value_i == 0), the window the first-level LUT accepts, and
 * max_abs_noise = max_i |noise_i|.
 * ------------------------------------------------------------------------------------- */
/* LwePublicKeyRlweMode (A, B = A s0 + E) over Z_2048[X]/(X^512 + 1): 2,048 bytes, the wire form */
typedef struct {
  uint16_t a[512];
  uint16_t b[512];
} omr_clue_key;

omr_status omr_secret_clue_key(const omr_secret_key_pack *sk, omr_clue_key *out);
/* The words >= 2048 over n_keys keys; reports, does not reject. */
omr_status omr_clue_key_validate(const omr_clue_key *keys, size_t n_keys, uint64_t *noncanonical);
/* K: the largest |e| the generators' sampler can draw for a clue key or a clue (the last index of its
 * cumulative table, csrc/rng.hpp). */
omr_status omr_clue_key_noise_support(uint64_t *K);
/* The key's noise e = B - A s0 mod 2048, centred into [-1024, 1023]; words are reduced mod 2048 first and
 * a word >= 2048 counts as non-canonical; coeffs_over counts the coefficients with |e| > limit
 * (UINT64_MAX = K). Any output may be NULL. CPU. */
omr_status omr_clue_key_audit(const omr_secret_key_pack *sk, const omr_clue_key *key, uint64_t limit,
                              uint64_t *max_abs_noise, uint32_t *coeffs_over, uint32_t *noncanonical);

typedef struct omr_sender omr_sender;
/* Copies the table of n_keys keys. device >= 0 also uploads it, the Gaussian table and the error word to
 * that device, once; device < 0: CPU only (omr_sender_gen_clues_device then returns
 * OMR_ERR_INVALID_ARGUMENT). OMR_ERR_INVALID_ARGUMENT for n_keys = 0, n_keys > UINT32_MAX, or a word
 * >= 2048 (the message names the first such key). Calls on one sender are serialised. */
omr_status omr_sender_create(const omr_clue_key *keys, size_t n_keys, int device, omr_sender **out);
void       omr_sender_destroy(omr_sender *s);
/* The clue of global index first + m under key recipient[m] (recipient NULL: key 0 for every message):
 * clue_a u16 [count][512], clue_b u16 [count][7]. nthreads <= 0: the host's cores, at most 16. */
omr_status omr_sender_gen_clues(const omr_sender *s, const uint32_t *recipient, uint64_t seed, uint64_t first,
                                size_t count, uint16_t *clue_a, uint16_t *clue_b, int nthreads);
/* The same bits into device buffers of the sender's device on hip_stream (NULL = null stream);
 * d_recipient u32 [count] in device memory, or NULL. */
omr_status omr_sender_gen_clues_device(omr_sender *s, const uint32_t *d_recipient, uint64_t seed,
                                       uint64_t first, size_t count, uint16_t *d_clue_a, uint16_t *d_clue_b,
                                       void *hip_stream);

/* decrypt_clue for all 7 clues of each of count messages: values u8 [count][7], pertinent u8 [count],
 * max_abs_noise u8 [count]; any output may be NULL, not all three. count = 0 does nothing. */
omr_status omr_clue_open(const omr_secret_key_pack *sk, const uint16_t *clue_a, const uint16_t *clue_b,
                         size_t count, uint8_t *values, uint8_t *pertinent, uint8_t *max_abs_noise,
                         int nthreads);
/* The same on device buffers of the current HIP device (d_clue_a 16-byte aligned) on hip_stream; the
 * call hands s0 to the kernel itself and returns after the stream has finished the work. */
omr_status omr_clue_open_device(const omr_secret_key_pack *sk, const uint16_t *d_clue_a,
                                const uint16_t *d_clue_b, size_t count, uint8_t *d_values,
                                uint8_t *d_pertinent, uint8_t *d_max_abs_noise, void *hip_stream);

/* ---------------------------------------------------------------------------------------
 * Seeded detection key (none in the reference): the form a recipient sends and a server stores.
 * More than half of a detection key is uniform masks that carry no secret (the `a` half of every
 * RLWE row, 670 of the 671 words of every key-switching row). A seeded key carries a public 64-bit
 * mask_seed instead and only the bodies:
 *      bsk1_b      u32 [512][8][1024]    16,777,216 B
 *      ksk_b       u32 [1024][27]           110,592 B
 *      bsk2_b      u64 [670][12][2048]  131,727,360 B
 *      trace_key_b u64 [11][25][2048]     4,505,600 B
 *      mask_seed   u64                            8 B    153,120,776 B against 380,227,584 B
 *
 * Definition. Stream(seed, domain, row) is the ChaCha12 row stream of the generators above (key
 * words seed lo, seed hi, "keyg", domain, 0, 0, 0, 0; block counter from 0; stream id = the row of the
 * component); uniform(q) takes 64 bits, keeps the bit length of q and rejects values >= q.
 *  - The mask of row r of a component is the first N accepted draws of
 *    Stream(mask_seed, DOM_*_MASK, r).uniform(q), N = 1024 / 670 / 2048 / 2048; mask domains
 *    30 (bsk1), 31 (ksk), 32 (bsk2), 33 (trace_key).
 *  - The noise of row r is Gaussian draws (the generators' tables) from Stream(seed, DOM_*_NOISE, r),
 *    starting at the stream's first word; noise domains 40, 41, 42, 43. They are domains of their own
 *    on purpose: omr_keygen_detection_key(seed) draws a row's mask and then its noise from one stream
 *    and publishes the mask, so a seeded key whose noise came from that stream's first words would
 *    have its noise published by a plain key generated from the same seed.
 *  - Rows, with mg, the component of the gadget, sigma_g and the gadget values exactly those of
 *    omr_keygen_detection_key, products in Z_q[X]/(X^N+1):
 *      BSK a-gadget row:  a = mask, b = a*s + e - mg*s      (s ternary, mg*s coefficient-wise)
 *      BSK b-gadget row:  a = mask, b = a*s + e, plus mg at coefficient 0
 *      trace-key row:     a = mask, b = a*s2 + e - sigma_g(s2) * 4^j
 *      KSK row:           a[670] = mask, b = <a, s_int> + e + s1_i * 2^j
 *    The a-gadget row is the layout's (alpha + m g, alpha s + e) with alpha = a - mg: same phase
 *    e - mg*s, same distribution. The expanded key is therefore an ordinary detection key for every
 *    entry point below, and its `a` words are a function of the public seed alone. It is a new key:
 *    it does not equal omr_keygen_detection_key(seed), whose output is unchanged.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const uint32_t *bsk1_b;
  const uint32_t *ksk_b;
  const uint64_t *bsk2_b;
  const uint64_t *trace_key_b;
  uint64_t mask_seed;
} omr_seeded_key_view;

typedef enum { OMR_KEY_BSK1 = 0, OMR_KEY_KSK = 1, OMR_KEY_BSK2 = 2, OMR_KEY_TRACE = 3 } omr_key_component;

/* The bodies of the seeded key of (sk, seed, mask_seed), on the host; nthreads <= 0: all host cores. */
omr_status omr_keygen_seeded_key(const omr_secret_key_pack *sk, uint64_t seed, uint64_t mask_seed,
                                 uint32_t *bsk1_b, uint32_t *ksk_b, uint64_t *bsk2_b,
                                 uint64_t *trace_key_b, int nthreads);
/* The same bits into device buffers of the current HIP device on `stream`; returns after the stream has
 * completed the work. */
omr_status omr_keygen_seeded_key_device(const omr_secret_key_pack *sk, uint64_t seed, uint64_t mask_seed,
                                        uint32_t *d_bsk1_b, uint32_t *d_ksk_b, uint64_t *d_bsk2_b,
                                        uint64_t *d_trace_key_b, void *stream);
/* Seeded key -> the full key in the coefficient-domain layout (host buffers). */
omr_status omr_expand_detection_key(const omr_seeded_key_view *key, uint32_t *bsk1, uint32_t *ksk,
                                    uint64_t *bsk2, uint64_t *trace_key, int nthreads);
/* The same bits into device buffers of the current HIP device (16-byte aligned) on `stream`. Each body
 * may lie in host memory or in device memory of that device (16-byte aligned); a host body is staged
 * through a device buffer of at most 64 MiB. Returns after the stream has completed the work;
 * OMR_ERR_DEVICE ("uniform stream overrun") if a mask row rejects more than 32 draws. */
omr_status omr_expand_detection_key_device(const omr_seeded_key_view *key, uint32_t *d_bsk1, uint32_t *d_ksk,
                                           uint64_t *d_bsk2, uint64_t *d_trace_key, void *stream);
/* Stage entry points (tests): the masks of rows [first_row, first_row + rows) of one component and
 * nothing else, out [rows][N], u32 for OMR_KEY_BSK1 and OMR_KEY_KSK (N = 1024, 670), u64 for
 * OMR_KEY_BSK2 and OMR_KEY_TRACE (N = 2048). OMR_ERR_INVALID_ARGUMENT for a component that does not
 * exist or a range beyond the component (4096, 27648, 8040, 275 rows). The device call writes a
 * device buffer (16-byte aligned) on `stream` and returns after the stream has completed the work. */
omr_status omr_key_masks(uint64_t mask_seed, int component, size_t first_row, size_t rows, void *out);
omr_status omr_key_masks_device(uint64_t mask_seed, int component, size_t first_row, size_t rows,
                                void *d_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Retrieval layout — RetrievalParams::new(257, 2048, all, pertinent, 130, 25, 2)
 * (parameters/retrieval_params.rs:50-106; arguments as in key_gen/secret.rs:189-209).
 * ------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t index_slots_per_bucket, slots_per_bucket, slots_per_segment, segment_per_cipher,
      max_encode_indices_cipher_count, combination_count, cmb_count_per_cipher, cmb_cipher_count;
} omr_retrieval_params;
omr_status omr_get_retrieval_params(size_t all_payloads_count, size_t pertinent_count,
                                    omr_retrieval_params *out);
/* Payload weights: StdRng::from_seed(seed) + Uniform<u16>(0,257), drawn in the reference's
 * order (detector.rs:376-387): out[j*all + i] for combination j < combination_count, the rest
 * zero; out has cmb_cipher_count*cmb_count_per_cipher*all entries. */
omr_status omr_payload_weights(const uint8_t seed[32], size_t all_payloads_count,
                               uint32_t combination_count, uint32_t cmb_cipher_count,
                               uint32_t cmb_count_per_cipher, uint16_t *out);

/* ---------------------------------------------------------------------------------------
 * Retriever (client side, CPU): Retriever::decode_digest (retriever.rs:188-260).
 * ------------------------------------------------------------------------------------- */
/* Decrypt + decode n NttRlweCiphertexts (u64 [n][2][2048], NTT domain) under the pack's s2:
 * out[m][j] = round_half_up(phase_j * 257 / q2) mod 257 (retriever.rs:84-96). */
omr_status omr_decrypt_decode(const omr_secret_key_pack *sk, const uint64_t *ct, size_t n,
                              uint32_t *out);
/* decode_pertinent_indices over the index digest ciphertexts in order, stopping once
 * pertinent_count distinct indices are known (retriever.rs:63-130, :197-201). Writes up to cap
 * indices in increasing order and the number found (the caller compares it with the count). */
omr_status omr_retrieve_indices(const omr_secret_key_pack *sk, const uint64_t *idx_cts,
                                uint32_t n_ct, size_t all_payloads_count, size_t pertinent_count,
                                size_t *indices, size_t cap, size_t *found);
/* decode_combined_payloads + solve_matrix_mod_257 (retriever.rs:203-258, matrix.rs:164-247):
 * payloads u16 [n_indices][612] of the sorted retrieved indices, from the payload digest
 * ciphertexts and the board's weights (omr_payload_weights, same seed as the detector).
 * `combination_count` is the board's RetrievalParams::combination_count (the reference's matrix
 * has that many rows whatever the number of indices found, retriever.rs:196, :215-239); 0 takes
 * the count of a board whose pertinent count is n_indices. OMR_ERR_NOT_INVERTIBLE when the system
 * is singular. */
omr_status omr_retrieve_payloads(const omr_secret_key_pack *sk, const uint64_t *pay_cts,
                                 uint32_t n_ct, size_t all_payloads_count, uint32_t combination_count,
                                 const uint16_t *weights, const size_t *indices, size_t n_indices,
                                 uint16_t *payloads);

/* ---------------------------------------------------------------------------------------
 * Auditor (client side, GPU or CPU): decrypt, classify and noise-audit NttRlweCiphertexts
 * (pertinency vectors or digests) under the pack's s2. The decoded plaintexts are those of
 * omr_decrypt_decode (retriever.rs:84-96); the class per ciphertext is the omd KAT (omd.rs:48-58:
 * a pertinent message decrypts to [1, 0, .., 0], any other to zeros); the residual summary is the
 * exact-integer counterpart of NoiseSigmaInfo (retriever.rs:390-560).
 *
 * Arithmetic, exact integers throughout. Input words are reduced mod q2 first. For one ciphertext
 * (a, b) the phase is c = N2^-1 * INTT(b - a (.) NTT(s2)) mod q2, canonical in [0, q2). Per
 * coefficient, with p = 257:
 *   t' = floor((2 p c + q2) / (2 q2)) in [0, 257]; the decoded value is t = 0 if t' = 257, else t';
 *   the residual is r = p c - t' q2, |r| <= (q2 - 1) / 2 < 2^49.
 * |r| / q2 is the distance of the phase from its decode point in plaintext steps: 0.5 would be a
 * decode failure. An encoder places plaintext m at m * Delta2, Delta2 = round_half_up(q2 / 257), and
 * 257 * Delta2 - q2 = -69, so a noiseless encryption of m has r = -69 m (at most 69 * 256 in
 * magnitude): that systematic term is part of r by definition.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  uint64_t max_abs_residual; /* largest |r| over the 2,048 coefficients */
  uint32_t nonzero;          /* decoded coefficients != 0 */
  uint32_t first;            /* decoded coefficient 0 */
} omr_ct_audit;
/* Class of a record: zero (nonzero == 0), one-hot (nonzero == 1 && first == 1: the omd KAT's
 * [1, 0, .., 0]), other (anything else). */
#define OMR_AUDIT_RESIDUAL_BINS 50
/* Accumulated into by every audit call that is given one, never reset by the library (the caller
 * zeroes it). Only integer counts and a maximum, so it does not depend on grid, staging or call
 * order. residual_bits[k] counts the coefficients whose |r| has bit length k (k = 0 for r = 0; k <= 49);
 * their sum is 2048 * ciphertexts. */
typedef struct {
  uint64_t ciphertexts, zero, one_hot, other, max_abs_residual;
  uint64_t residual_bits[OMR_AUDIT_RESIDUAL_BINS];
} omr_audit_summary;

/* An auditor holds the pack's level-2 secret (NTT(s2)) and the inverse twiddles on `device`; it needs
 * no detector context: the party that holds the secret is not the detector. Calls on one auditor are
 * serialised. */
typedef struct omr_auditor omr_auditor;
omr_status omr_auditor_create(const omr_secret_key_pack *sk, int device, omr_auditor **out);
void       omr_auditor_destroy(omr_auditor *aud);
/* knobs, results identical for every setting: workgroups of the grid (0 = default, two per compute
 * unit) and the ciphertexts staged per piece by the host entry point (0 = default 2,048 = 64 MiB) */
omr_status omr_auditor_set_grid(omr_auditor *aud, unsigned workgroups);
omr_status omr_auditor_set_staging(omr_auditor *aud, size_t max_ciphertexts);
/* device buffers of the auditor's device, enqueued on hip_stream (NULL = null stream), returns once
 * enqueued; d_cts u64 [n][2][2048] (16-byte aligned), d_records [n], d_decoded u16 [n][2048],
 * d_summary (added into; the caller zeroes it): any may be NULL, not all three; n = 0 does nothing */
omr_status omr_audit_device(omr_auditor *aud, const uint64_t *d_cts, size_t n, omr_ct_audit *d_records,
                            uint16_t *d_decoded, omr_audit_summary *d_summary, void *hip_stream);
/* host buffers, staged in pieces; returns when done; summary is added into */
omr_status omr_audit(omr_auditor *aud, const uint64_t *cts, size_t n, omr_ct_audit *records,
                     uint16_t *decoded, omr_audit_summary *summary);
/* the same results on the CPU (no GPU, no auditor): the statement the kernel is checked against and
 * the path of a client without a device. nthreads <= 0: the host's cores, at most 16. */
omr_status omr_audit_cpu(const omr_secret_key_pack *sk, const uint64_t *cts, size_t n,
                         omr_ct_audit *records, uint16_t *decoded, omr_audit_summary *summary,
                         int nthreads);

/* ---------------------------------------------------------------------------------------
 * Detector — one context per GPU; calls on one context are serialised; contexts are
 * independent. Detector::new (detector.rs:85-110) uploads the keys and converts them to the
 * device layout; the LUTs (:457-503) are built inside. The key view may point to host memory
 * or to device memory of `device` (e.g. from omr_keygen_detection_key_device). The context
 * keeps a 32 MB host copy of BSK1 until level 1's exact-NTT key is first needed
 * (omr_ctx_set_rounding_guard / omr_ctx_set_exact_level1, or at creation when level 1 is guarded
 * by the exactness contract); the copy is dropped once that key is built.
 * ------------------------------------------------------------------------------------- */
typedef struct omr_ctx omr_ctx;

typedef struct {
  const uint32_t *bsk1;
  const uint32_t *ksk;
  const uint64_t *bsk2;
  const uint64_t *trace_key;
} omr_detection_key_view;

omr_status omr_ctx_create(const omr_detection_key_view *key, int device, omr_ctx **out);
/* The same context from a seeded key (bodies in host memory or in device memory of `device`): expands
 * it on the device (omr_expand_detection_key_device) into temporary buffers, runs exactly the creation
 * path of omr_ctx_create on them and frees them before it returns. The temporaries are the full key,
 * 380,227,584 B (362.6 MiB), plus at most 64 MiB of staging while a host body is expanded. */
omr_status omr_ctx_create_seeded(const omr_seeded_key_view *key, int device, omr_ctx **out);
void omr_ctx_destroy(omr_ctx *ctx);
/* Kernel names of this build's detect pipeline: "br1=<name> ks=<name> br2=<name>". */
const char *omr_detect_kernels(void);
/* Messages per internal detect chunk (memory/latency knob: 36 KiB of scratch per message);
 * 0 = the default 16,384. */
omr_status omr_ctx_set_batch(omr_ctx *ctx, size_t batch);
/* Chunks of at most `max_messages` messages run the latency kernels (each level-1 rotation
 * spread over more waves, each level-2 message over two CUs that exchange partial products
 * through global memory every step, or over two wave groups of one CU when the cooperative
 * launch of the two-CU grid is refused, and each message's trace over five CUs that all-reduce
 * their digit partials, or one CU when that launch is refused: lower single-message latency,
 * bit-identical output); larger chunks run the throughput kernels. Default 64; 0 = always
 * throughput. The multi-CU grids are launched with hipLaunchCooperativeKernel, so their
 * workgroups are co-resident; if a hand-off still does not complete, the kernel ends, its output
 * is invalid and the error is reported by omr_ctx_check (after the caller's stream sync), by the
 * host entry points, and by the next detect call on the context (which then returns
 * OMR_ERR_DEVICE without running). */
omr_status omr_ctx_set_latency_threshold(omr_ctx *ctx, size_t max_messages);
/* Synchronises `hip_stream` (NULL: the whole device) and reports a pending device-side
 * failure of an earlier call on the context (the two-CU hand-off timeout above) as
 * OMR_ERR_DEVICE, clearing it; OMR_OK when every call completed correctly. Callers of the
 * device entry points use it where they would otherwise only synchronise. */
omr_status omr_ctx_check(omr_ctx *ctx, void *hip_stream);
/* Exactness of the FFT external products. The level-1 rotations and the throughput
 * level-2 rotation compute each external product with FP64 FFTs and round every coefficient to the
 * integer it equals (the reference computes it with an exact NTT: detector.rs:553-557, :623 via
 * concrete-ntt, omr_core/Cargo.toml:38-45). With the guard on, the detect kernels run guarded
 * variants (same output, slower) that record the largest |y - rint(y)| over every rounded
 * coefficient: observed[0] level 1, observed[1] level 2, since context creation or the last reset.
 * apriori[l] is the proven bound E on |computed - exact| of every such coefficient for this key
 * (from kappa[l], the largest stored key-spectrum magnitude, computed at context creation): if
 * E < 0.5 the rounding is exact for every input; a run with observed < 1 - E is exact (an error
 * |e| in [0.5, E] would show a margin >= 1 - E). Any pointer may be NULL; reset != 0 zeroes the
 * observed margins after reading them. The read synchronises the device.
 * The first enable on a context (of this or of omr_ctx_set_exact_level1) builds level 1's exact-NTT
 * key: it allocates 64 MB of device memory and runs a blocking conversion under the context mutex
 * (other calls on the context wait), and can fail with OMR_ERR_DEVICE or OMR_ERR_OUT_OF_MEMORY;
 * the setting is then unchanged. */
omr_status omr_ctx_set_rounding_guard(omr_ctx *ctx, int enable);
omr_status omr_ctx_rounding_margin(omr_ctx *ctx, double observed[2], double apriori[2],
                                   double kappa[2], int reset);
/* The exactness contract. A level whose a priori bound E >= 0.5 runs its guarded
 * kernels on EVERY launch of the context, whatever omr_ctx_set_rounding_guard says; after each
 * such launch the observed margin m of that launch is compared with 1 - E on the device:
 *  - level 2: a launch with m >= 1 - E2 is re-run on the exact modular NTT (the latency family's
 *    br2l_kernel + trace), in the same stream order, so its outputs are exact;
 *  - level 1: a launch with m >= 1 - E1 is re-run on the exact modular NTT (br1n_fallback_kernel,
 *    br1_ntt.hpp) in the same stream order, so its outputs are exact.
 * guarded[l] != 0 when level l + 1 is guarded on every launch (automatically or by the user);
 * breaches[l] counts the launches of level l + 1 whose margin reached the threshold. Any pointer
 * may be NULL. Reading breaches synchronises the device. */
omr_status omr_ctx_exactness(omr_ctx *ctx, int guarded[2], uint64_t breaches[2]);
/* The launch record: which level-2 rotation and trace kernel the context's calls ran. Every entry point
 * that reaches level 2 (detect, omr_second_level, omr_blind_rotate_level2[_from], omr_trace) chooses its
 * kernels on the host -- by size, guard, a priori bounds, and whether the cooperative two-CU launch fits
 * and the runtime accepts it, falling back silently otherwise. counts[k] is the cumulative number of
 * launches of kind k since the context was created (the counters are never reset: compare two reads).
 * Host integers only, incremented under the context's mutex where the choice is made: the record adds no
 * kernel argument, device memory or synchronisation. */
typedef enum {
  /* the level-2 rotation of one launch: exactly one of these five */
  OMR_LAUNCH_BR2F = 0,       /* throughput, FFT (br2f_kernel) */
  OMR_LAUNCH_BR2F_GUARD = 1, /* throughput, guarded FFT (br2f_guard_kernel) */
  OMR_LAUNCH_BR2L = 2,       /* latency, one workgroup per message, NTT (br2l_kernel) */
  OMR_LAUNCH_BR2X = 3,       /* latency, two CUs per message, NTT (br2x_kernel), cooperative */
  OMR_LAUNCH_BR2Y = 4,       /* latency, two CUs per message, FFT (br2y_kernel), cooperative */
  OMR_LAUNCH_BR2Y_HELPERS = 5, /* of the BR2Y launches, those that carried the key-prefetch helper rows */
  OMR_LAUNCH_BR2_FROM = 6,   /* of the five, those on the kernel's _from instantiation (a supplied acc0) */
  OMR_LAUNCH_GUARD_FALLBACK = 7, /* guarded level-2 launches (rotation, or omr_trace's trace) followed by
                                  * the conditional exact fallback kernels */
  /* the trace of one launch: exactly one of these four */
  OMR_LAUNCH_TRACE_FFT = 8,       /* throughput, FFT (trace_fft_kernel) */
  OMR_LAUNCH_TRACE_FFT_GUARD = 9, /* throughput, guarded FFT (trace_fft_guard_kernel) */
  OMR_LAUNCH_TRACE_X = 10,        /* latency, TRACE_X CUs per message (trace_x_kernel), cooperative */
  OMR_LAUNCH_TRACE_KERNEL = 11,   /* one workgroup per message, NTT (trace_kernel) */
  OMR_LAUNCH_COUNT = 12
} omr_launch_kind;
omr_status omr_ctx_launch_record(omr_ctx *ctx, uint64_t counts[OMR_LAUNCH_COUNT]);
/* Level 1 on the exact modular NTT for every launch of the context (br1n_kernel: the reference's
 * own arithmetic, concrete-ntt in BlindRotationKey::blind_rotate, detector.rs:553-557), instead of the
 * FFT kernels; enable = 0 restores them. Outputs are bit-identical either way -- a cross-check of
 * the FFT path at any size, about 3x slower at level 1.
 * The first enable on a context (of this or of omr_ctx_set_rounding_guard) builds the exact-NTT
 * key: it allocates 64 MB of device memory and runs a blocking conversion under the context mutex,
 * and can fail with OMR_ERR_DEVICE or OMR_ERR_OUT_OF_MEMORY; the setting is then unchanged. */
omr_status omr_ctx_set_exact_level1(omr_ctx *ctx, int enable);
/* Diagnostics: `count` stored key-spectrum values (complex, re/im pairs) starting at value `first`
 * of level 1 (BSK1, [512][8][2][512], /512) or level 2 (BSK2 limbs, [670][12][2][2][1024], /1024),
 * in the kernels' storage order (register-major slots). */
omr_status omr_ctx_key_spectrum(omr_ctx *ctx, int level, size_t first, size_t count, double *out);
/* Diagnostics (host only, no GPU): the double-double twiddles of the key transform of `level`
 * (n - 1 entries, stage s node i at (1 << s) - 1 + i; per entry re.hi, re.lo, im.hi, im.lo). */
omr_status omr_fft_twiddles_dd(int level, double *out);
/* Encode workgroups fold ceil(D / max_chunks) messages each (at least 32, or 128 from D = 16,384),
 * so a call keeps at most `max_chunks` partial digests per ciphertext (32 KiB each); 0 = the
 * default 4,096. A memory knob: the digests are identical for every setting. */
omr_status omr_ctx_set_encode_chunks(omr_ctx *ctx, size_t max_chunks);

/* Detector::detect (detector.rs:135-166), batched like `par_iter().map(detect)` in
 * examples/omr.rs:160-164. Host buffers: clue_a u16 [D][512], clue_b u16 [D][7],
 * out u64 [D][2][2048] (NTT domain). */
omr_status omr_detect_batch(omr_ctx *ctx, const uint16_t *clue_a, const uint16_t *clue_b,
                            size_t D, uint64_t *out);
/* Detector::detect (detector.rs:135-138) for one message: clue_a u16 [512], clue_b u16 [7],
 * out u64 [2][2048]. Safe to call from many host threads at once on one context, as the
 * reference's `clues.par_iter().map(|c| detector.detect(c))` does on a shared &Detector
 * (examples/omr.rs:160-164): concurrent calls are coalesced into batched launches (whichever
 * caller finds no launch in progress takes every queued request, up to max_messages, as one
 * omr_detect_batch), so many callers reach batch throughput; a lone caller gets single-message
 * latency. Each caller returns when its own output is written. */
omr_status omr_detect(omr_ctx *ctx, const uint16_t *clue_a, const uint16_t *clue_b, uint64_t *out);
/* Coalescing knobs of omr_detect: at most max_messages per combined launch (0 = 65,536), and a
 * window (microseconds, default 0) a launching caller waits for more requests first. */
omr_status omr_ctx_set_coalescing(omr_ctx *ctx, size_t max_messages, long window_us);
/* omr_detect calls served and combined launches run so far on the context. */
omr_status omr_ctx_coalescing_stats(omr_ctx *ctx, size_t *calls, size_t *launches);
/* Same on device buffers, enqueued on `hip_stream` (NULL = HIP's null stream, which orders with
 * the other blocking streams, as in every HIP API); returns once enqueued. Calls on one context may use different streams: they share the
 * context's scratch, so a call's kernels wait (hipStreamWaitEvent) for those of the previous
 * call on another stream; the caller orders its own buffers. */
omr_status omr_detect_batch_device(omr_ctx *ctx, const uint16_t *d_clue_a,
                                   const uint16_t *d_clue_b, size_t D, uint64_t *d_out,
                                   void *hip_stream);

/* Detector::detect_with_time_info (detector.rs:169-221): device time per stage of the last detect
 * call, milliseconds, summed over its messages like DetectTimeInfo (detector.rs:51-57):
 *   total_ms        total_detect_time                      = first_level + second_level + trace
 *   first_level_ms  total_first_level_bootstrapping_time   7 rotations + sum + key switch + mod switch
 *   second_level_ms total_second_level_bootstrapping_time  level-2 blind rotation
 *   trace_ms        total_trace_time                       hom_trace + NTT
 *   key_switch_ms   the sum + key-switch + mod-switch part of first_level_ms (two_level_bs.rs:62-73)
 * Timing modes (omr_ctx_enable_timing): 0 off; 1 and 2 are the same, stage events around the
 * production kernels. Both kernel families run the trace as its own launch after the level-2
 * rotation, so trace_ms is always the reference's split. trace_separate is always 1; the field
 * and the two mode numbers are kept for ABI compatibility. */
typedef struct {
  float total_ms, first_level_ms, second_level_ms, trace_ms, key_switch_ms;
  size_t messages;
  int trace_separate;
} omr_detect_timing;
omr_status omr_ctx_enable_timing(omr_ctx *ctx, int mode);
omr_status omr_last_timing(omr_ctx *ctx, omr_detect_timing *t);
/* omr_detect_batch with timing on and omr_last_timing as one call under the context's lock
 * (concurrent callers cannot switch timing off under each other or read another call's times);
 * the context's timing mode is left as it was. */
omr_status omr_detect_with_time_info(omr_ctx *ctx, const uint16_t *clue_a, const uint16_t *clue_b,
                                     size_t D, uint64_t *out, omr_detect_timing *t);

/* Detector::encode_pertinent_indices (detector.rs:223-339) for index ciphertext `ct` over the
 * messages with global indices [global_offset, global_offset+D) of an all_payloads_count board.
 * Buckets come from a seeded counter-based stream (the reference uses thread_rng, :262) so
 * that shards agree. out u64 [2][2048] (NTT domain), a partial digest summed mod q2 across
 * shards. The device entry returns OMR_ERR_INVALID_ARGUMENT before anything is enqueued for n_ct = 0
 * or n_ct > 65,535, a range [global_offset, global_offset + D) that does not lie on the board
 * (checked without the sum, which may wrap), D > INT32_MAX, or a NULL d_pv with D > 0; the host entry
 * inherits the checks. */
omr_status omr_encode_indices(omr_ctx *ctx, const uint64_t *pv, size_t D, size_t global_offset,
                              size_t all_payloads_count, uint64_t seed, uint32_t ct,
                              uint64_t *out);
omr_status omr_encode_indices_device(omr_ctx *ctx, const uint64_t *d_pv, size_t D,
                                     size_t global_offset, size_t all_payloads_count,
                                     uint64_t seed, uint32_t first_ct, uint32_t n_ct,
                                     uint64_t *d_out /* [n_ct][2][2048] */, void *hip_stream);
/* Detector::encode_pertinent_payloads (detector.rs:341-453). weights: omr_payload_weights()
 * output for the whole board; payloads u16 [D][612]; out u64 [n_ct][2][2048]. The device entry returns
 * OMR_ERR_INVALID_ARGUMENT before anything is enqueued on the conditions of
 * omr_encode_payloads_indexed_device: n_ct above 65,535 and a range beyond the board among them. */
omr_status omr_encode_payloads(omr_ctx *ctx, const uint64_t *pv, const uint16_t *payloads,
                               size_t D, size_t global_offset, size_t all_payloads_count,
                               const uint16_t *weights, uint32_t n_ct, uint32_t cmb_per_ct,
                               uint64_t *out);
omr_status omr_encode_payloads_device(omr_ctx *ctx, const uint64_t *d_pv,
                                      const uint16_t *d_payloads, size_t D, size_t global_offset,
                                      size_t all_payloads_count, const uint16_t *d_weights,
                                      uint32_t n_ct, uint32_t cmb_per_ct, uint64_t *d_out,
                                      void *hip_stream);

/* ---------------------------------------------------------------------------------------
 * Bitmap digest (none in the reference): the detection-only digest from which a recipient learns
 * exactly which messages of a board are pertinent and how many, with no bound on the count known in
 * advance and no bucket collisions. Retriever::decode_pertinent_indices (retriever.rs:63-130,
 * :197-204) needs pertinent_count to know when it is done; this digest needs only the board size.
 *
 * Layout. A pertinent pv_g decrypts to [1, 0, .., 0] and any other to zeros (omd.rs:48-58), so
 * pv_g * 2^t * X^j decrypts to 2^t at coefficient j. The message with global index g goes to
 *   ciphertext c = g / 16384,  l = g % 16384,  coefficient j = l % 2048,  bit t = l / 2048,
 * and a board of `all` messages has ceil(all / 16384) bitmap ciphertexts (omr_bitmap_ct_count):
 *   out[c][h][i] = sum_g pv_g[h][i] * 2^t * psi^((2 brv11(i) + 1) j mod 4096)  mod q2,  h in {a, b},
 * the second factor being NTT(X^j)[i] in the convention above. Outputs are canonical residues in the
 * NTT domain like every digest; messages that are not folded in contribute nothing; the sum is exact,
 * so every partition of a board into calls, added mod q2, gives the same bits. Coefficient j of
 * ciphertext c decodes to sum_t 2^t [message 16384 c + 2048 t + j is pertinent] <= 255 < p.
 *
 * Noise condition. In the auditor's terms decoding is correct while |r| / q2 < 0.5 at every
 * coefficient. Multiplying by 2^t X^j permutes and negates a ciphertext's noise coefficients and
 * scales them by 2^t, so a full bitmap ciphertext's |r| / q2 is at most (sum_t 2^t) * 2048 * E =
 * 522,240 E (plus the systematic term, at most 69 * 255 / q2), E being the largest |r| / q2 over the
 * pertinency ciphertexts folded in: E < 9.5e-7 suffices (measured E and bitmap noise: DESIGN.md §1).
 * ------------------------------------------------------------------------------------- */
#define OMR_BITMAP_BITS 8
#define OMR_BITMAP_MESSAGES_PER_CT 16384
/* ceil(all_payloads_count / 16384); all_payloads_count = 0 (or a count beyond uint32_t) is invalid */
omr_status omr_bitmap_ct_count(size_t all_payloads_count, uint32_t *n_ct);
/* The bitmap ciphertexts of the whole board over the messages [global_offset, global_offset + D):
 * d_out u64 [n_ct][2][2048], every ciphertext written (those the range does not touch are zero; D = 0
 * writes zeros). d_pv u64 [D][2][2048], canonical (not validated), 16-byte aligned. Enqueued on
 * hip_stream (NULL = null stream), returns once enqueued. A workgroup folds slices of 128 messages;
 * omr_ctx_set_encode_chunks bounds the partials kept per ciphertext here too (identical bits). */
omr_status omr_encode_bitmap_device(omr_ctx *ctx, const uint64_t *d_pv, size_t D, size_t global_offset,
                                    size_t all_payloads_count, uint64_t *d_out /* [n_ct][2][2048] */,
                                    void *hip_stream);
/* The same on host buffers; returns when done. */
omr_status omr_encode_bitmap(omr_ctx *ctx, const uint64_t *pv, size_t D, size_t global_offset,
                             size_t all_payloads_count, uint64_t *out);
/* Client side, host only: the global indices of the set bits of decoded bitmap ciphertexts (decoded
 * u16 [n_ct][2048]: omr_decrypt_decode's values narrowed to u16, or the `decoded` output of omr_audit /
 * omr_audit_cpu; a client with a GPU decodes the bitmap with the auditor), in increasing order. Writes
 * at most cap indices and the full count to *found. OMR_ERR_INVALID_ARGUMENT ("not a bitmap digest of
 * this board") for n_ct != omr_bitmap_ct_count(all), a value >= 256, or a set bit at or beyond all. */
omr_status omr_bitmap_indices(const uint16_t *decoded /* [n_ct][2048] */, uint32_t n_ct,
                              size_t all_payloads_count, size_t *indices, size_t cap, size_t *found);
/* omr_decrypt_decode of the bitmap ciphertexts u64 [n_ct][2][2048] + omr_bitmap_indices (CPU). */
omr_status omr_retrieve_bitmap(const omr_secret_key_pack *sk, const uint64_t *bitmap_cts, uint32_t n_ct,
                               size_t all_payloads_count, size_t *indices, size_t cap, size_t *found);

/* ---------------------------------------------------------------------------------------
 * Digest session — the detector's whole board flow (examples/omr.rs:160-203: detect every message,
 * encode_pertinent_indices per index ciphertext, encode_pertinent_payloads once; detector.rs:223-453)
 * behind one handle that never holds the board's pertinency vector. The caller feeds message
 * ranges in any order and any sizes; the library detects and encodes them in pieces of at most the
 * context's detect batch (omr_ctx_set_batch) and keeps the running digest, the ciphertexts that
 * Retriever::decode_digest (retriever.rs:188-260) consumes, on the device. The digest is an exact
 * sum mod q2 of per-message terms, so every partition of a board into updates, and every split of
 * it over sessions joined by omr_digest_merge, gives the same bits as omr_detect_batch followed by
 * omr_encode_indices for each ciphertext and omr_encode_payloads.
 *
 * Calls on one session are serialised. Several sessions may live on one context and interleave
 * with any other call on it: each session owns its buffers and shares the context's detect / encode
 * scratch in stream order like every device entry point. Destroying the context before its
 * sessions is a caller error (a session uses the context until omr_digest_destroy returns).
 * ------------------------------------------------------------------------------------- */
typedef struct omr_digest omr_digest;

typedef struct {
  uint32_t index_ct, payload_ct;      /* rp.max_encode_indices_cipher_count, rp.cmb_cipher_count */
  uint32_t combination_count, cmb_count_per_cipher;
  size_t   all_payloads_count;
  size_t   messages;                  /* global indices folded in by update calls of THIS session */
  size_t   pv_capacity_messages;      /* pertinency ciphertexts the session currently has room for */
} omr_digest_info;

/* A session for an all_payloads_count board: the layout is omr_get_retrieval_params(all, pertinent),
 * the buckets of the index ciphertexts come from index_seed as in omr_encode_indices, and the weights
 * are omr_payload_weights(weight_seed, all, combination_count, cmb_cipher_count,
 * cmb_count_per_cipher), generated on the host and uploaded once: the call blocks while it does so.
 * All device work of the session is enqueued on `hip_stream` (NULL = HIP's null stream). Device
 * footprint: payload_ct * cmb_count_per_cipher * all * 2 bytes of weights, the running digest
 * ([index_ct + payload_ct][2][2048] u64, zeroed), at most one detect chunk of pertinency
 * ciphertexts (32 KiB per message, allocated by the first update) and, for host updates, the
 * staging of one chunk of clues and payloads (2.3 KiB per message). */
omr_status omr_digest_begin(omr_ctx *ctx, size_t all_payloads_count, size_t pertinent_count,
                            uint64_t index_seed, const uint8_t weight_seed[32],
                            void *hip_stream, omr_digest **out);
/* Folds the messages with global indices [global_offset, global_offset + D) into the digest:
 * clue_a u16 [D][512], clue_b u16 [D][7], payloads u16 [D][612]. Per piece of at most the context's
 * detect batch: Detector::detect into the session's pertinency buffer, then every index ciphertext
 * (detector.rs:223-339) and every payload ciphertext (:341-453) over it, added to the running digest
 * mod q2. The pertinency buffer grows to min(largest piece seen, batch) messages and no further
 * (omr_digest_info.pv_capacity_messages). OMR_ERR_INVALID_ARGUMENT, before anything is enqueued and
 * with the session still usable, for a range that reaches beyond the board or overlaps one already
 * folded in, or a NULL pointer with D > 0; D = 0 does nothing. Host and device updates may be mixed.
 * Host buffers: returns once the stream has finished the update (the buffers may be reused) and
 * reports a failed hand-off as omr_detect_batch does. Device buffers (of the context's device):
 * returns once enqueued; the caller keeps the inputs alive and synchronises through omr_ctx_check or
 * omr_digest_read. A device failure reported to any call on the session poisons it (see
 * omr_digest_read). */
omr_status omr_digest_update(omr_digest *dg, const uint16_t *clue_a, const uint16_t *clue_b,
                             const uint16_t *payloads, size_t D, size_t global_offset);
omr_status omr_digest_update_device(omr_digest *dg, const uint16_t *d_clue_a, const uint16_t *d_clue_b,
                                    const uint16_t *d_payloads, size_t D, size_t global_offset);
/* Adds another session's omr_digest_read output (host arrays; e.g. the shard of another GPU for the
 * same board, seeds and layout) into this one mod q2, the sum the reference takes with
 * add_element_wise (detector.rs:333-336, :445-448). Either pointer may be NULL, not both. Every value
 * must be canonical: OMR_ERR_INVALID_ARGUMENT for one >= q2, the digest unchanged. `messages` counts
 * this session's own updates and is not touched. Returns once the stream has taken the arrays. */
omr_status omr_digest_merge(omr_digest *dg, const uint64_t *idx_cts, const uint64_t *pay_cts);
/* Synchronises the session's stream and copies the canonical digest to the host: idx_cts u64
 * [index_ct][2][2048], pay_cts u64 [payload_ct][2][2048], the inputs of omr_retrieve_indices and
 * omr_retrieve_payloads (retriever.rs:188-260). Either pointer may be NULL. Nothing is reset, so the
 * digest can be read between updates. A pending hand-off error of the context (omr_ctx_check) is
 * taken here: the call then returns OMR_ERR_DEVICE and the session is poisoned, every later call on
 * it returns OMR_ERR_DEVICE. */
omr_status omr_digest_read(omr_digest *dg, uint64_t *idx_cts, uint64_t *pay_cts);
omr_status omr_digest_get_info(omr_digest *dg, omr_digest_info *info);
/* The session's bitmap digest ("Bitmap digest" above). omr_digest_enable_bitmap allocates a zeroed
 * running bitmap u64 [omr_bitmap_ct_count(all)][2][2048] on the device; every later piece then also folds
 * its pertinency ciphertexts into it, in the same stream order and under the same poisoning rules as
 * the index and payload digests, which are not affected. It must come before the session's first
 * non-empty update and before any merge: later it returns OMR_ERR_INVALID_ARGUMENT and the session
 * stays usable, without a bitmap. A second call is a no-op. A session that never enables the bitmap
 * does exactly what it did before, and omr_digest_read_bitmap / omr_digest_merge_bitmap on it return
 * OMR_ERR_INVALID_ARGUMENT. omr_digest_info does not describe the bitmap: its ciphertext count comes
 * from omr_bitmap_ct_count. */
omr_status omr_digest_enable_bitmap(omr_digest *dg);
/* As omr_digest_read, for the bitmap: synchronises, takes a pending hand-off error (poisoning the
 * session), then copies bitmap_cts u64 [n_ct][2][2048] to the host. */
omr_status omr_digest_read_bitmap(omr_digest *dg, uint64_t *bitmap_cts);
/* As omr_digest_merge, for the bitmap: adds another session's omr_digest_read_bitmap output mod q2;
 * OMR_ERR_INVALID_ARGUMENT for a value >= q2, the bitmap unchanged. */
omr_status omr_digest_merge_bitmap(omr_digest *dg, const uint64_t *bitmap_cts);
/* Synchronises the session's stream and frees its buffers; NULL is ignored. */
void omr_digest_destroy(omr_digest *dg);

/* ---------------------------------------------------------------------------------------
 * Compact ciphertexts (none in the reference): the form in which a digest travels to the recipient. A
 * digest ciphertext leaves the detector with far more precision than decoding needs (max |r| / q2 of
 * 2.2e-5 for a 7-ciphertext digest and 2.4e-5 for a full bitmap ciphertext; decoding fails
 * at 0.5), so it is modulus-switched from q2 to Q = 2^bits and sent at `bits` bits per coefficient:
 * 512 * bits bytes instead of 32,768 (12,288 at 24 bits, 10,240 at 20). `bits` is any integer in
 * [OMR_COMPACT_MIN_BITS, OMR_COMPACT_MAX_BITS]; p = 257.
 *
 * Compact. The input is an NttRlweCiphertext u64 [2][2048]; words are reduced mod q2 first, as the
 * auditor does. For h in {a, b} let x_h be the coefficient form: the polynomial whose NTT in the
 * convention above is the input row, canonical in [0, q2), in natural coefficient order. Per coefficient
 *   y = floor((2 x Q + q2) / (2 q2)) mod Q.
 * q2 is odd, so there are no ties; x close to q2 rounds to Q and wraps to 0.
 *
 * Packing. One compact ciphertext is 512 * bits bytes: the 2,048 values of a, then those of b, as one
 * little-endian bit stream per polynomial (256 * bits bytes each). Value i occupies stream bits
 * [i bits, (i + 1) bits); stream bit k is bit (k mod 8) of byte k / 8. 512 * bits is a multiple of 16, so
 * every ciphertext of an array starts on a 16-byte boundary when the array does.
 *
 * Expand. Per value x' = (y q2 + Q / 2) >> bits, which lies in [0, q2); then the forward NTT. The result
 * is an ordinary NttRlweCiphertext under the same key, canonical, and every client entry point takes it
 * unchanged: omr_retrieve_indices, omr_retrieve_payloads, omr_retrieve_bitmap, omr_decrypt_decode, the
 * auditor.
 *
 * Bound. Write the compacted phase in units of Q. Each of the 4,096 roundings errs by at most 1/2; the
 * a-side errors reach the phase through a negacyclic product with the ternary s2, so compaction adds
 * delta with |delta_j| <= (1 + ||s2||_1) / 2 in units of Q. Expansion rounds once more per value and adds
 * at most the same amount in units of q2. In the auditor's residual units (r = p c - t' q2), as long as
 * the decoded value does not change,
 *   |r_expanded| <= |r_original| + R(bits),  R(bits) = ceil(p (1 + ||s2||_1) (q2 + Q) / (2 Q))
 * (omr_compact_residual_bound). Decoding of a compacted ciphertext is therefore proven correct when
 * max |r_original| + R(bits) <= (q2 - 1) / 2. With ||s2||_1 <= 2048, R / q2 is 0.0157 at 24 bits, 0.0628
 * at 22, 0.2511 at 20 and 0.502 at 19: 19 bits is not provable for a worst-case key. A real key has
 * ||s2||_1 near 1,365, and the recipient knows its own. The server cannot evaluate the bound (it has no
 * secret); it compacts to the width the recipient asked for.
 *
 * A compacted ciphertext is for decoding only: it no longer has the headroom of a pertinency ciphertext,
 * so it must not be fed to omr_encode_* or merged into a digest (merging stays in the full form).
 * ------------------------------------------------------------------------------------- */
#define OMR_COMPACT_MIN_BITS 16
#define OMR_COMPACT_MAX_BITS 32
/* 512 * bits; OMR_ERR_INVALID_ARGUMENT for bits out of range (as in every call below, before anything
 * else is looked at or enqueued) */
omr_status omr_compact_ct_bytes(int bits, size_t *bytes);
/* R(bits) for the pack's s2 (a 128-bit product on the host) */
omr_status omr_compact_residual_bound(const omr_secret_key_pack *sk, int bits, uint64_t *R);
/* The CPU statement of both directions (no GPU): out is n x 512 bits bytes, cts_out u64 [n][2][2048].
 * nthreads <= 0: the host's cores, at most 16. n = 0 does nothing; NULL with n > 0 is invalid. */
omr_status omr_compact_cts_cpu(const uint64_t *cts, size_t n, int bits, void *out, int nthreads);
omr_status omr_compact_expand_cpu(const void *packed, size_t n, int bits, uint64_t *cts_out, int nthreads);
/* Server side, on the context's device: needs the context's level-2 inverse twiddles and nothing else
 * (no key, no scratch lease), so it runs beside any other call on the context. Device buffers, 16-byte
 * aligned (OMR_ERR_INVALID_ARGUMENT otherwise, and for NULL with n > 0), enqueued on hip_stream
 * (NULL = null stream); returns once enqueued; n = 0 does nothing. The same bits as omr_compact_cts_cpu. */
omr_status omr_compact_cts_device(omr_ctx *ctx, const uint64_t *d_cts, size_t n, int bits, void *d_out,
                                  void *hip_stream);
/* the same on host buffers, staged in pieces on the context's own stream; returns when done */
omr_status omr_compact_cts(omr_ctx *ctx, const uint64_t *cts, size_t n, int bits, void *out);
/* knobs, results identical for every setting: workgroups of compact_kernel's grid, which strides over the
 * ciphertexts (0 = default, six per compute unit; also used by omr_digest_read_compact), and the
 * ciphertexts staged per piece by omr_compact_cts (0 = default 2,048 = 64 MiB) */
omr_status omr_ctx_set_compact_grid(omr_ctx *ctx, unsigned workgroups);
omr_status omr_ctx_set_compact_staging(omr_ctx *ctx, size_t max_ciphertexts);
/* Client side, on an auditor, which holds the level-2 forward twiddles for this. Device buffers of the
 * auditor's device, 16-byte aligned, enqueued on hip_stream; returns once enqueued; n = 0 does nothing.
 * The same bits as omr_compact_expand_cpu. omr_auditor_set_grid sets expand_kernel's grid too (0 = six
 * per compute unit). */
omr_status omr_compact_expand_device(omr_auditor *aud, const void *d_packed, size_t n, int bits,
                                     uint64_t *d_cts, void *hip_stream);
/* omr_audit over compact ciphertexts in host memory: staged in pieces (omr_auditor_set_staging), each
 * expanded on the device and audited there. Results identical to omr_audit over omr_compact_expand_cpu's
 * output; summary is added into. */
omr_status omr_audit_compact(omr_auditor *aud, const void *packed, size_t n, int bits, omr_ct_audit *records,
                             uint16_t *decoded, omr_audit_summary *summary);
/* The session's digest in compact form: idx_packed index_ct x 512 bits bytes, pay_packed payload_ct x,
 * bitmap_packed omr_bitmap_ct_count(all) x; any pointer may be NULL. bitmap_packed non-NULL on a session
 * without a bitmap is OMR_ERR_INVALID_ARGUMENT. Synchronises, takes a pending hand-off error and follows
 * the poisoning rules exactly as omr_digest_read does; then compacts the running digest on the device and
 * copies only the packed bytes: the same bits as omr_compact_cts_cpu of omr_digest_read /
 * omr_digest_read_bitmap. The running digest is not modified: later updates, reads and merges behave as
 * before. */
omr_status omr_digest_read_compact(omr_digest *dg, int bits, void *idx_packed, void *pay_packed,
                                   void *bitmap_packed);

/* ---------------------------------------------------------------------------------------
 * Indexed payload weights (none in the reference): payload weights that are a function of (seed,
 * combination, global message index) alone, so that no party draws or holds a board-wide table.
 * omr_payload_weights restates the reference's one sequential StdRng stream with rejection
 * (detector.rs:376-387): weight (j, i) is known only after j * all + i draws, and the detector, every
 * shard and the recipient each build the whole [combinations][all] table. Here, with key[0..7] the
 * little-endian words of the 32-byte weight seed exactly as in omr_payload_weights, for combination
 * j < 2^32 and global message index g:
 *   B      = chacha_block(12, key, counter = g >> 4, stream = (0x70617977 << 32) | j)      ("payw")
 *   w(j,g) = (uint64_t)B[g & 15] * 257 >> 32     for j <  combination_count, in [0, 256]
 *   w(j,g) = 0                                   for j >= combination_count (a padding combination)
 * One block holds one combination's weights for 16 consecutive messages.
 *
 * Stream separation. The reference stream (omr_payload_weights) uses stream id 0 and the index buckets
 * "bukt"; the stream id here is never 0, so the streams never share a block.
 * No rejection step, so the index is random-access. Each residue receives 16,711,935 or 16,711,936 of
 * the 2^32 words: a relative bias below 6.1e-8. The solve's invertibility argument (i.i.d. near-uniform
 * entries mod 257) is untouched.
 *
 * Everything else of the payload digest is unchanged: the slot layout, the centred lift, the NTT, the
 * sum mod q2, cmb_count_per_cipher and omr_get_retrieval_params. An indexed digest is an ordinary payload
 * digest: any partition of a board, any shard and any merge give the same bits, and it is compacted,
 * audited and merged like any other. The two conventions do not mix: a digest encoded with indexed
 * weights is solved with omr_retrieve_payloads_indexed (or omr_retrieve_payloads given the indexed table).
 * ------------------------------------------------------------------------------------- */
/* Host, parallel (nthreads <= 0: the host's cores, at most 16): out u16 [n_combos][n_indices], out[r][k] =
 * w(first_combo + r, indices[k]); rows at or beyond combination_count are zero. The recipient's matrix is
 * (combination_count, 0, combination_count, its indices); any index of size_t is valid (no board size
 * enters). Sorted indices reuse a block. n_combos = 0 or n_indices = 0 does nothing. */
omr_status omr_indexed_weights_at(const uint8_t seed[32], uint32_t combination_count, uint32_t first_combo,
                                  uint32_t n_combos, const size_t *indices, size_t n_indices, uint16_t *out,
                                  int nthreads);
/* The indexed weights in omr_payload_weights's layout, out u16 [cmb_cipher_count * cmb_count_per_cipher][all]
 * (padding rows zero), for cross-checks and for callers that keep the table path: on the host, and into a
 * device buffer of the current HIP device on hip_stream (NULL = null stream; returns once enqueued).
 * OMR_ERR_INVALID_ARGUMENT for NULL, all = 0, or fewer rows than combinations. */
omr_status omr_indexed_weights_table(const uint8_t seed[32], size_t all_payloads_count, uint32_t combination_count,
                                     uint32_t cmb_cipher_count, uint32_t cmb_count_per_cipher, uint16_t *out,
                                     int nthreads);
omr_status omr_indexed_weights_table_device(const uint8_t seed[32], size_t all_payloads_count,
                                            uint32_t combination_count, uint32_t cmb_cipher_count,
                                            uint32_t cmb_count_per_cipher, uint16_t *d_out, void *hip_stream);
/* omr_encode_payloads_device with indexed weights computed in the kernel: no table. Covers the payload
 * ciphertexts [first_ct, first_ct + n_ct), which hold the combinations first_ct * cmb_per_ct ..; a caller
 * can therefore encode a large digest in groups of ciphertexts. Combinations at or beyond
 * combination_count are padding: a ciphertext that holds only padding is all zeros. d_out u64
 * [n_ct][2][2048]; the same bits as omr_encode_payloads_device fed omr_indexed_weights_table_device's
 * table. OMR_ERR_INVALID_ARGUMENT, before anything is enqueued, for NULL (seed included), n_ct = 0 or above
 * 65,535, cmb_per_ct = 0 or cmb_per_ct * 612 > 2048, or global_offset + D > all_payloads_count. */
omr_status omr_encode_payloads_indexed_device(omr_ctx *ctx, const uint64_t *d_pv, const uint16_t *d_payloads,
                                              size_t D, size_t global_offset, size_t all_payloads_count,
                                              const uint8_t seed[32], uint32_t combination_count,
                                              uint32_t first_ct, uint32_t n_ct, uint32_t cmb_per_ct,
                                              uint64_t *d_out /* [n_ct][2][2048] */, void *hip_stream);
/* The same on host buffers; returns when done. */
omr_status omr_encode_payloads_indexed(omr_ctx *ctx, const uint64_t *pv, const uint16_t *payloads, size_t D,
                                       size_t global_offset, size_t all_payloads_count, const uint8_t seed[32],
                                       uint32_t combination_count, uint32_t first_ct, uint32_t n_ct,
                                       uint32_t cmb_per_ct, uint64_t *out);
/* omr_digest_begin for a session whose payload digest uses indexed weights: it draws, uploads and holds no
 * weights (the call does not block on a table) and runs the indexed kernel per piece. Device footprint: the
 * running digest, one detect chunk of pertinency ciphertexts and the host updates' staging, none of which
 * grows with all_payloads_count. Every other session call behaves as documented above; the index digest
 * and the bitmap are those of an omr_digest_begin session on the same inputs. */
omr_status omr_digest_begin_indexed(omr_ctx *ctx, size_t all_payloads_count, size_t pertinent_count,
                                    uint64_t index_seed, const uint8_t weight_seed[32], void *hip_stream,
                                    omr_digest **out);
/* The bytes of device memory a session owns now (*total: weights, running digest, pertinency chunk, host
 * staging, merge staging, bitmap, compact buffer) and the weights' share of them (*weights: 0 for an
 * indexed session, always). Not poisoned-sensitive; touches no stream. */
omr_status omr_digest_device_bytes(omr_digest *dg, size_t *total, size_t *weights);
/* omr_retrieve_payloads for an indexed digest: the same decode and the same elimination, the matrix
 * taken from omr_indexed_weights_at (combination_count x n_indices values; no table). The same status
 * codes, OMR_ERR_NOT_INVERTIBLE included. */
omr_status omr_retrieve_payloads_indexed(const omr_secret_key_pack *sk, const uint64_t *pay_cts, uint32_t n_ct,
                                         size_t all_payloads_count, uint32_t combination_count,
                                         const uint8_t weight_seed[32], const size_t *indices, size_t n_indices,
                                         uint16_t *payloads);

/* ---------------------------------------------------------------------------------------
 * Payload length as a board parameter (none in the reference): indexed payload digests whose payloads are
 * L words long, 1 <= L <= OMR_PAYLOAD_LEN_MAX, instead of the 612 of OMR_PAYLOAD_LEN. The reference's own
 * recipient can only read 612-word payloads, so the table and seek conventions stay at 612; the length
 * belongs to the indexed convention, the one for parties not bound to the reference.
 *
 * Layout of a board with payload length L and pertinent_count pertinent messages:
 *   stripes           = ceil(L / 2048), at most 8
 *   per               = min(2048 / L, OMR_PAYLOAD_PER_CT_MAX) combinations per ciphertext for L <= 2048,
 *                       1 for L > 2048
 *   combination_count = pertinent_count + 5, as in omr_get_retrieval_params
 *   groups            = ceil(combination_count / per),  payload_ct = groups * stripes
 * Ciphertext c is stripe s = c % stripes of group c / stripes, which holds the combinations
 * (c / stripes) * per + j for j < per. A combination at or beyond combination_count is padding, with
 * weight 0. With one stripe, slot j * L + l holds centred_lift(payload[l] * w(combo, g) mod 257) for l < L
 * and every other slot is 0. With several stripes (per = 1), slot i of stripe s holds that value for word
 * l = 2048 * s + i when l < L, and 0 otherwise. w is omr_indexed_weights_at's weight, unchanged, and so are
 * the centred lift, the NTT and the sum mod q2. L = 612 at 3 combinations per ciphertext fills a ciphertext
 * that omr_get_retrieval_params fills with 2. The cap of 16 combinations keeps the weights a workgroup
 * stages at 16 x 144 u16 of LDS: below L = 128 a ciphertext is not full (16 L < 2048 slots are used).
 * ------------------------------------------------------------------------------------- */
#define OMR_PAYLOAD_LEN_MAX 16384
#define OMR_PAYLOAD_PER_CT_MAX 16
typedef struct {
  uint32_t payload_len, combination_count, cmb_count_per_cipher, stripes, payload_ct;
} omr_payload_layout;
/* The layout above. OMR_ERR_INVALID_ARGUMENT for NULL, payload_len = 0 or above OMR_PAYLOAD_LEN_MAX, or a
 * pertinent_count whose combination count does not fit 32 bits. */
omr_status omr_get_payload_layout(size_t pertinent_count, size_t payload_len, omr_payload_layout *out);
/* omr_encode_payloads_indexed_device for payloads u16 [D][payload_len]. first_ct and n_ct count ciphertexts,
 * stripes included: the call covers the ciphertexts [first_ct, first_ct + n_ct) of the layout with cmb_per_ct
 * combinations per group, so it may start or end in the middle of a stripe group. cmb_per_ct is explicit, as
 * in omr_encode_payloads_indexed_device: any value in [1, per] (a digest is decoded with the value it was
 * encoded with). A ciphertext that holds only padding is all zeros. payload_len = 612 with cmb_per_ct <= 3
 * gives the bits of omr_encode_payloads_indexed_device. OMR_ERR_INVALID_ARGUMENT, before anything is
 * enqueued, for NULL (seed included), n_ct = 0 or above 65,535, payload_len = 0 or above
 * OMR_PAYLOAD_LEN_MAX, cmb_per_ct = 0 or above the layout's per for that length, D above INT32_MAX, or
 * global_offset + D > all_payloads_count. */
omr_status omr_encode_payloads_indexed_len_device(omr_ctx *ctx, const uint64_t *d_pv,
                                                  const uint16_t *d_payloads /* [D][payload_len] */, size_t D,
                                                  size_t global_offset, size_t all_payloads_count,
                                                  const uint8_t seed[32], uint32_t combination_count,
                                                  uint32_t payload_len, uint32_t cmb_per_ct, uint32_t first_ct,
                                                  uint32_t n_ct, uint64_t *d_out /* [n_ct][2][2048] */,
                                                  void *hip_stream);
/* The same on host buffers; returns when done. */
omr_status omr_encode_payloads_indexed_len(omr_ctx *ctx, const uint64_t *pv, const uint16_t *payloads, size_t D,
                                           size_t global_offset, size_t all_payloads_count, const uint8_t seed[32],
                                           uint32_t combination_count, uint32_t payload_len, uint32_t cmb_per_ct,
                                           uint32_t first_ct, uint32_t n_ct, uint64_t *out);
/* omr_digest_begin_indexed for a board whose payloads are payload_len words long: the session's updates take
 * payloads u16 [D][payload_len], its payload digest has omr_get_payload_layout(pertinent_count, payload_len)'s
 * payload_ct ciphertexts, and omr_digest_get_info reports that payload_ct and cmb_count_per_cipher. Merge,
 * read, compact read, bitmap and omr_digest_device_bytes work unchanged on it; the index digest and the
 * bitmap do not depend on the length. OMR_ERR_INVALID_ARGUMENT for a length out of range, or a layout of more
 * than 65,535 payload ciphertexts (a session encodes them in one launch; such a board is encoded in groups
 * with omr_encode_payloads_indexed_len_device). */
omr_status omr_digest_begin_indexed_len(omr_ctx *ctx, size_t all_payloads_count, size_t pertinent_count,
                                        uint64_t index_seed, const uint8_t weight_seed[32], size_t payload_len,
                                        void *hip_stream, omr_digest **out);
/* The payload layout of any session: of a 612-word session, payload_len 612, one stripe and
 * omr_get_retrieval_params' counts. */
omr_status omr_digest_get_payload_layout(omr_digest *dg, omr_payload_layout *layout);
/* omr_retrieve_payloads_indexed for a digest of the layout given: payloads u16 [n_indices][payload_len]. The
 * system has layout->combination_count rows; combination j's payload_len words are gathered across its
 * stripes, and the solve is the same one with width = payload_len. Of the layout, payload_len,
 * combination_count and cmb_count_per_cipher are read (stripes and payload_ct follow from them; n_ct must be at
 * least ceil(combination_count / cmb_count_per_cipher) * stripes). The status codes of
 * omr_retrieve_payloads_indexed, OMR_ERR_NOT_INVERTIBLE included; OMR_ERR_INVALID_ARGUMENT also for a NULL
 * layout, a length out of range or a cmb_count_per_cipher the length does not allow. */
omr_status omr_retrieve_payloads_indexed_len(const omr_secret_key_pack *sk, const uint64_t *pay_cts, uint32_t n_ct,
                                             size_t all_payloads_count, const omr_payload_layout *layout,
                                             const uint8_t weight_seed[32], const size_t *indices,
                                             size_t n_indices, uint16_t *payloads);

/* ---------------------------------------------------------------------------------------
 * Solve mod 257 — solve_matrix_mod_257 (matrix.rs:164-247), the elimination behind
 * Retriever::decode_digest, as an operation of its own: on the CPU, and on an auditor's device.
 *
 * Definition. Every input word is reduced mod 257 first. The system is [matrix | rhs] with rows >= cols.
 * For column i = 0 .. cols - 1:
 *   - the pivot is the FIRST row j >= i whose current entry (j, i) is non-zero;
 *   - rows i and j are swapped, in the matrix and in the rhs;
 *   - row i is scaled by the inverse of its pivot;
 *   - every row below i is reduced by its entry in column i times row i.
 * After the last column back substitution clears the entries above the diagonal, and the solution is rows
 * 0 .. cols - 1 of the rhs. If a column has no pivot the call reports OMR_ERR_NOT_INVERTIBLE ("Matrix is
 * not invertible") and the column, and writes no solution.
 *
 * The arithmetic is exact and the pivot rule is fixed, so the result is a function of the inputs alone,
 * also for an inconsistent system (rows > cols, e.g. a garbage digest), where the pivot rule decides which
 * equations are solved. Any schedule that makes the same pivot choices gives the same bits;
 * the device solver is a blocked one.
 * ------------------------------------------------------------------------------------- */
#define OMR_SOLVE_MAX_ROWS 8192
/* matrix u16 [rows][cols], rhs u16 [rows][width], solution u16 [cols][width]; every input word is reduced
 * mod 257 first. cols >= 1, rows >= cols, rows <= OMR_SOLVE_MAX_ROWS, width >= 1, else
 * OMR_ERR_INVALID_ARGUMENT. OMR_ERR_NOT_INVERTIBLE sets *singular_col (it may be NULL) and leaves solution
 * untouched. nthreads parallelises the row updates (<= 0: the host's cores, at most 16). */
omr_status omr_solve_mod257_cpu(const uint16_t *matrix, const uint16_t *rhs, size_t rows, size_t cols,
                                size_t width, uint16_t *solution, size_t *singular_col, int nthreads);
/* Tile sizes of this build, so tests can place their shapes on the edges: the columns factorised per panel
 * step, and the rows and columns of one tile of the trailing update. Any pointer may be NULL. */
omr_status omr_solve_geometry(unsigned *panel_cols, unsigned *tile_rows, unsigned *tile_width);
/* Device buffers of the auditor's device, 16-byte aligned. Inputs are not modified. d_status u32:
 * 0 = solved, 1 + i = no pivot in column i (d_solution then not written). Enqueued on hip_stream
 * (NULL = null stream), returns once enqueued. Works in scratch owned by the auditor (grown on
 * demand: rows * (cols + width) words, each row padded to a multiple of 8 words); a call on another
 * stream waits by event for the previous call's kernels, as detect does for the context's scratch. */
omr_status omr_solve_mod257_device(omr_auditor *aud, const uint16_t *d_matrix, const uint16_t *d_rhs,
                                   size_t rows, size_t cols, size_t width, uint16_t *d_solution,
                                   uint32_t *d_status, void *hip_stream);
/* Diagnostics for tools/retrieve_bench.py, not part of the stable interface (it may change or go with the
 * solver's schedule; an auditor that never enables it records nothing): with enable != 0 every later
 * omr_solve_mod257_device on the auditor records events around its steps; the call synchronises the auditor's last solve and writes the
 * device time of that solve per step, milliseconds: step_ms[0] panel, [1] row swaps and pivot block,
 * [2] trailing update, [3] back substitution (zeros if none was profiled). step_ms may be NULL. */
omr_status omr_solve_profile(omr_auditor *aud, int enable, float step_ms[4]);

/* Retrieval on the auditor: the CPU entry points above with the decode (audit_kernel), the system's
 * right-hand side, the indexed matrix and the solve on the device. Ciphertexts come from host memory, full
 * (bits = 0, u64 [n_ct][2][2048]) or compact (bits in [16, 32], n_ct x 512 bits bytes, expanded on the
 * device), staged as omr_audit stages them; the decoded values stay on the device. Each call returns the
 * same bits and the same status codes as its CPU twin (for bits != 0: the CPU call over
 * omr_compact_expand_cpu's output), and OMR_ERR_INVALID_ARGUMENT ("more than OMR_SOLVE_MAX_ROWS
 * combinations") for a system of more than OMR_SOLVE_MAX_ROWS rows. They return when done. */
omr_status omr_auditor_retrieve_indices(omr_auditor *aud, const void *idx_cts, uint32_t n_ct, int bits,
                                        size_t all_payloads_count, size_t pertinent_count, size_t *indices,
                                        size_t cap, size_t *found);
omr_status omr_auditor_retrieve_payloads(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits,
                                         size_t all_payloads_count, uint32_t combination_count,
                                         const uint16_t *weights, const size_t *indices, size_t n_indices,
                                         uint16_t *payloads);
omr_status omr_auditor_retrieve_payloads_indexed(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits,
                                                 size_t all_payloads_count, uint32_t combination_count,
                                                 const uint8_t weight_seed[32], const size_t *indices,
                                                 size_t n_indices, uint16_t *payloads);
/* omr_retrieve_payloads_indexed_len's device twin ("Payload length as a board parameter" above), for full and
 * compact ciphertexts: the right-hand side is gathered across the stripes on the device and the solver runs
 * with width = layout->payload_len. The same bits and status codes as the CPU entry. */
omr_status omr_auditor_retrieve_payloads_indexed_len(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits,
                                                     size_t all_payloads_count, const omr_payload_layout *layout,
                                                     const uint8_t weight_seed[32], const size_t *indices,
                                                     size_t n_indices, uint16_t *payloads);
/* decode_digest in one call, indexed weights: indices, then payloads of the indices found. The system
 * has the board's rp.combination_count rows. cap < found is OMR_ERR_INVALID_ARGUMENT with *found set.
 * summary (may be NULL) is added into with the audit of every ciphertext the call decoded (all of
 * idx_cts and pay_cts). payloads u16 [found][612]. */
omr_status omr_auditor_decode_digest_indexed(omr_auditor *aud, const void *idx_cts, uint32_t n_idx_ct,
                                             const void *pay_cts, uint32_t n_pay_ct, int bits,
                                             size_t all_payloads_count, size_t pertinent_count,
                                             const uint8_t weight_seed[32], size_t *indices, size_t cap,
                                             size_t *found, uint16_t *payloads, omr_audit_summary *summary);

/* ---------------------------------------------------------------------------------------
 * Reference payload weights by seek (none in the reference): omr_payload_weights' own values, weight by
 * weight, without the table. The reference draws one StdRng stream through Uniform<u16>(0, 257)
 * (detector.rs:376-387), which rejects a 32-bit word v when the low half of v * 257 exceeds the zone
 * 0xFFFFFFFE. Since 2^32 = 1 (mod 257), v * 257 = 0xFFFFFFFF (mod 2^32) has the single solution
 * v = 0x00FF00FF: one word in 2^32 is rejected, and accepted draw n sits at raw stream position
 * n + (rejections met so far). A 2^20 x 1,005 board (1.05e9 draws) meets at least one rejection with
 * probability 0.22, so the list of rejections is short but cannot be assumed empty.
 *
 * Definition. The stream is ChaCha12 with key[0..7] the little-endian words of the 32-byte seed, stream
 * id 0: word(r) = chacha_block(12, key, counter = r >> 4, stream = 0)[r & 15] for raw position r. A raw word
 * is rejected when (uint32_t)(word * 257) > zone. With r_0 < r_1 < .. the rejected raw positions:
 *   at[k]  = r_k - k                        draws accepted when rejection k is met (nondecreasing)
 *   pos(n) = n + #{k : at[k] <= n}          raw position of accepted draw n
 *   w(n)   = (uint64_t)word(pos(n)) * 257 >> 32
 * and weight (j, i) of a board is w(j * all + i) for j < combination_count, 0 for a padding combination.
 * Two adjacent rejected words give two equal entries of at[]. A seek lists the rejections that matter for
 * the draws n < draws: those with at[k] < draws, a prefix of the list. A board needs
 * draws >= combination_count * all; every consumer returns OMR_ERR_INVALID_ARGUMENT otherwise. Only the
 * builders read `zone`; consumers read draws, n and at[] alone. At most OMR_WEIGHT_SEEK_MAX rejections
 * fit: a stream with more is OMR_ERR_INVALID_ARGUMENT ("more than 32 rejections: use the table") from the
 * builders, which then leave *out untouched; with the reference's zone a board expects draws / 2^32 rejections, 0.24 at
 * 2^20 x 1,005 (33 of them: below 1e-50), and the cap is reached around 2^37 draws. The indexed convention above stays: it needs no scan and has no cap, where nobody is bound
 * to the reference's stream.
 * ------------------------------------------------------------------------------------- */
#define OMR_WEIGHT_SEEK_MAX 32
#define OMR_WEIGHT_ZONE 0xFFFFFFFEu
typedef struct {
  uint64_t draws;                   /* valid for accepted draws n < draws */
  uint32_t n;                       /* rejections that matter for those draws */
  uint32_t zone;                    /* 0xFFFFFFFE for every public builder */
  uint64_t at[OMR_WEIGHT_SEEK_MAX]; /* at[k] = r_k - k, nondecreasing */
} omr_weight_seek;
/* Host builder, parallel over ChaCha blocks (nthreads <= 0: the host's cores, at most 16): scans the raw
 * words [0, draws + OMR_WEIGHT_SEEK_MAX], which hold every rejection that can shift a draw below `draws`.
 * OMR_ERR_INVALID_ARGUMENT for NULL or draws >= 2^62. */
omr_status omr_weight_seek_build_cpu(const uint8_t seed[32], uint64_t draws, int nthreads, omr_weight_seek *out);
/* The same scan on the current HIP device, on hip_stream (NULL = null stream); returns after the stream
 * has completed the scan, as omr_gen_clues_device does. The same result and the same errors. */
omr_status omr_weight_seek_build_device(const uint8_t seed[32], uint64_t draws, omr_weight_seek *out,
                                        void *hip_stream);
/* Stage entries for tests: the builders with an explicit zone (a smaller zone makes rejections frequent).
 * The public builders are these with OMR_WEIGHT_ZONE. */
omr_status omr_weight_seek_build_zone_cpu(const uint8_t seed[32], uint64_t draws, uint32_t zone, int nthreads,
                                          omr_weight_seek *out);
omr_status omr_weight_seek_build_zone_device(const uint8_t seed[32], uint64_t draws, uint32_t zone,
                                             omr_weight_seek *out, void *hip_stream);
/* The recipient's matrix in the reference's convention, host, parallel: out u16 [n_combos][n_indices],
 * out[r][k] = weight (first_combo + r, indices[k]); rows at or beyond combination_count are zero (the layout
 * and padding of omr_indexed_weights_at). OMR_ERR_INVALID_ARGUMENT for NULL, an index >= all, seek->n above
 * OMR_WEIGHT_SEEK_MAX, or combination_count * all > seek->draws. */
omr_status omr_payload_weights_at(const uint8_t seed[32], size_t all_payloads_count, uint32_t combination_count,
                                  const omr_weight_seek *seek, uint32_t first_combo, uint32_t n_combos,
                                  const size_t *indices, size_t n_indices, uint16_t *out, int nthreads);
/* omr_encode_payloads_indexed_device with the reference's weights found through the seek: the same
 * arguments, checks and padding rules, and the same bits as omr_encode_payloads_device fed
 * omr_payload_weights' table. Also OMR_ERR_INVALID_ARGUMENT for seek = NULL, seek->n above
 * OMR_WEIGHT_SEEK_MAX, or combination_count * all_payloads_count > seek->draws. */
omr_status omr_encode_payloads_seek_device(omr_ctx *ctx, const uint64_t *d_pv, const uint16_t *d_payloads, size_t D,
                                           size_t global_offset, size_t all_payloads_count, const uint8_t seed[32],
                                           const omr_weight_seek *seek, uint32_t combination_count,
                                           uint32_t first_ct, uint32_t n_ct, uint32_t cmb_per_ct,
                                           uint64_t *d_out /* [n_ct][2][2048] */, void *hip_stream);
/* The same on host buffers; returns when done. */
omr_status omr_encode_payloads_seek(omr_ctx *ctx, const uint64_t *pv, const uint16_t *payloads, size_t D,
                                    size_t global_offset, size_t all_payloads_count, const uint8_t seed[32],
                                    const omr_weight_seek *seek, uint32_t combination_count, uint32_t first_ct,
                                    uint32_t n_ct, uint32_t cmb_per_ct, uint64_t *out);
/* omr_digest_begin without the table: the session builds the seek of its board on the context's device at
 * begin (omr_weight_seek_build_device; the call returns when the scan is done), holds no weights
 * (omr_digest_device_bytes: weights = 0) and runs the seek kernel per piece. Every other session call
 * behaves as documented above, and the digest is bit-identical to that of an omr_digest_begin session on
 * the same inputs. */
omr_status omr_digest_begin_seek(omr_ctx *ctx, size_t all_payloads_count, size_t pertinent_count,
                                 uint64_t index_seed, const uint8_t weight_seed[32], void *hip_stream,
                                 omr_digest **out);
/* omr_retrieve_payloads without the table: the matrix from omr_payload_weights_at. seek = NULL builds the
 * seek inside the call (omr_weight_seek_build_cpu). The same bits and status codes as omr_retrieve_payloads
 * given omr_payload_weights' table, OMR_ERR_NOT_INVERTIBLE included. */
omr_status omr_retrieve_payloads_seek(const omr_secret_key_pack *sk, const uint64_t *pay_cts, uint32_t n_ct,
                                      size_t all_payloads_count, uint32_t combination_count,
                                      const uint8_t weight_seed[32], const omr_weight_seek *seek,
                                      const size_t *indices, size_t n_indices, uint16_t *payloads);
/* The same on the auditor (see "Retrieval on the auditor": full or compact ciphertexts, the same `bits`
 * rule): the matrix is built on the device from the same statement; seek = NULL builds the seek on the
 * auditor's device. */
omr_status omr_auditor_retrieve_payloads_seek(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits,
                                              size_t all_payloads_count, uint32_t combination_count,
                                              const uint8_t weight_seed[32], const omr_weight_seek *seek,
                                              const size_t *indices, size_t n_indices, uint16_t *payloads);

/* ---------------------------------------------------------------------------------------
 * Key audit (none in the reference): check a detection key against its secret before it is uploaded and
 * after any reload, and count non-canonical words at intake without a secret. A detector runs to
 * completion on a damaged key and returns well-formed ciphertexts that decrypt to "not pertinent"; this
 * is the check that finds the damage first.
 *
 * Arithmetic, exact integers throughout. A component c is an omr_key_component; its modulus q is q1 for
 * BSK1 and KSK and q2 for BSK2 and TRACE; rows and row layout are those of the key layout above (4096 /
 * 27648 / 8040 / 275 rows; an RLWE row is a[N] then b[N], a key-switching row a[670] then b). Every word
 * is reduced mod q first; a word >= q counts as non-canonical and is still used reduced. The noise of a row
 * is its phase minus the message the generators put there, centred into (-q/2, q/2):
 *   BSK row (i, r), k = r mod d, mg = bit_i 2^(drop + k logB) (bit = s0 for BSK1, s_int for BSK2; s = s1, s2):
 *     a-gadget (r < d):   e = (b - a s) + mg s     coefficient-wise; this holds for the plain row
 *                                                  (a = alpha + mg) and for the seeded row (b carries -mg s)
 *     b-gadget (r >= d):  e = (b - a s) - mg at coefficient 0
 *   TRACE row (k, j), g = 2048 / 2^k + 1:  e = (b - a s2) + sigma_g(s2) 4^j
 *   KSK row (i, j):                        e = b - <a, s_int> - s1_i 2^j mod q1   (one value per row)
 * Per row the audit yields row_max = max |e|; per call a summary.
 * ------------------------------------------------------------------------------------- */
/* Added into by every key-audit call that is given one and never reset by the library: counts, a maximum
 * and a minimum, so it does not depend on grid, staging or call order. The caller initialises it to zeros
 * with first_row_over = UINT64_MAX (merging is by minimum). noise_bits[k] counts the noise values whose
 * |e| has bit length k (k = 0 for e = 0); their sum is N * rows (rows for KSK: one value per row). */
typedef struct {
  uint64_t rows, noncanonical, max_abs_noise;
  uint64_t rows_over;       /* rows with row_max > limit */
  uint64_t first_row_over;  /* smallest such component row index; UINT64_MAX if none */
  uint64_t noise_bits[OMR_AUDIT_RESIDUAL_BINS];
} omr_key_audit_summary;

/* K: the largest |e| this library's generators can draw for the component (the last index of their
 * cumulative table, csrc/rng.hpp: 44 / 27,064 / 16 / 16). A `limit` of UINT64_MAX below means K. */
omr_status omr_key_noise_support(int component, uint64_t *K);

/* Row ranges (the kernels' entry, and the stage entry points of the tests). d_rows points at row
 * first_row of the component in device memory of the auditor's device (16-byte aligned; 4-byte for KSK,
 * whose rows are 2,684 bytes); d_row_max is u64 [rows]; it or d_summary may be NULL, not both. rows = 0
 * does nothing; a component that does not exist or a range beyond it is OMR_ERR_INVALID_ARGUMENT.
 * Enqueued on hip_stream (NULL = null stream), returns once enqueued. The first key-audit call on an
 * auditor uploads its level-1 tables and the secrets' coefficient forms (blocking). */
omr_status omr_audit_key_rows_device(omr_auditor *aud, int component, const void *d_rows, size_t first_row,
                                     size_t rows, uint64_t limit, uint64_t *d_row_max,
                                     omr_key_audit_summary *d_summary, void *hip_stream);
/* the same results on the CPU (host memory, no GPU): the statement the kernels are checked against.
 * nthreads <= 0: the host's cores, at most 16. */
omr_status omr_audit_key_rows_cpu(const omr_secret_key_pack *sk, int component, const void *rows_ptr,
                                  size_t first_row, size_t rows, uint64_t limit, uint64_t *row_max,
                                  omr_key_audit_summary *summary, int nthreads);
/* Whole keys: out[c] is added into for every component whose pointer is not NULL (a NULL component is
 * skipped and its entry left untouched); limit NULL = K for every component. The view's pointers may be
 * host memory or device memory of the auditor's device, as for omr_ctx_create; a host component is staged
 * in pieces of omr_auditor_set_staging x 32 KiB. Returns when done. */
omr_status omr_audit_key(omr_auditor *aud, const omr_detection_key_view *key, const uint64_t limit[4],
                         omr_key_audit_summary out[4]);
/* The same for a seeded key (all four bodies required, as for omr_expand_detection_key_device): expands it
 * on the auditor's device into temporaries (380,227,584 B), audits them and frees them. */
omr_status omr_audit_key_seeded(omr_auditor *aud, const omr_seeded_key_view *key, const uint64_t limit[4],
                                omr_key_audit_summary out[4]);
omr_status omr_audit_key_cpu(const omr_secret_key_pack *sk, const omr_detection_key_view *key,
                             const uint64_t limit[4], omr_key_audit_summary out[4], int nthreads);
/* Server side, no secret: the words >= q of its level (1: u32 against q1, 2: u64 against q2). These calls
 * report and do not reject; omr_ctx_create* take keys exactly as before. The device count is added into
 * *d_count on hip_stream of the current device and the call returns once enqueued; n = 0 does nothing. */
omr_status omr_key_count_noncanonical_device(int level, const void *d_words, size_t n, uint64_t *d_count,
                                             void *hip_stream);
/* noncanonical[c] is written for every component whose pointer is not NULL. Host memory, or device memory
 * of `device` (returns when done). The _seeded twins look at the bodies only: the masks come from the seed
 * by rejection sampling and are canonical by construction. */
omr_status omr_key_validate(const omr_detection_key_view *key, uint64_t noncanonical[4], int nthreads);
omr_status omr_key_validate_device(const omr_detection_key_view *key, int device, uint64_t noncanonical[4]);
omr_status omr_key_validate_seeded(const omr_seeded_key_view *key, uint64_t noncanonical[4], int nthreads);
omr_status omr_key_validate_seeded_device(const omr_seeded_key_view *key, int device, uint64_t noncanonical[4]);

/* ---------------------------------------------------------------------------------------
 * Stage entry points (for parity tests and per-stage benchmarks, benches/two_level_bs.rs).
 * Host buffers.
 * ------------------------------------------------------------------------------------- */
/* First level (detector.rs:533-597) for D messages: out u32 [D][671] (a[670], b mod 4096). */
omr_status omr_first_level(omr_ctx *ctx, const uint16_t *clue_a, const uint16_t *clue_b,
                           size_t D, uint32_t *lwe_int);
/* Test entry: the first level after its rotations (sum of the seven extracted LWEs mod q1, key switch,
 * modulus switch, body offset; detector.rs:556-594) on caller-supplied extracted LWEs. ext u32
 * [n][7][1025]: per message and clue the mask a[1024] then the body, in the layout the rotations write
 * (coefficient-0 extraction: a'[0] = a[0], a'[j] = -a[1024 - j]); out u32 [n][671] as omr_first_level's.
 * The same kernel selection as omr_first_level (n, the latency threshold). n <= the batch size; a word
 * >= q1 is OMR_ERR_INVALID_ARGUMENT, checked on the host before anything is enqueued. */
omr_status omr_sum_key_switch(omr_ctx *ctx, const uint32_t *ext, size_t n, uint32_t *lwe_int);
/* One level-1 blind rotation per LWE (a u16 [n][512], b u16 [n]): out u64 [n][2][1024]. */
omr_status omr_blind_rotate_level1(omr_ctx *ctx, const uint16_t *lwe_a, const uint16_t *lwe_b,
                                   size_t n, uint64_t *out);
/* Negacyclic product a * k mod (X^1024 + 1, q1) of n pairs through the level-1 FFT external-
 * product path (device_fft.hpp): a u32 [n][1024] with digit-sized centred values (|a| <= 17),
 * k u32 [n][1024] canonical; out u64 [n][1024] canonical. */
omr_status omr_fft1_mul(omr_ctx *ctx, const uint32_t *a, const uint32_t *k, size_t n,
                        uint64_t *out);
/* Second level + trace (detector.rs:599-639) on LWE(670, 4096) inputs: out u64 [n][2][2048]. */
omr_status omr_second_level(omr_ctx *ctx, const uint32_t *lwe_int, size_t n, uint64_t *out);
/* Level-2 blind rotation only (no trace): out u64 [n][2][2048] coefficient domain. */
omr_status omr_blind_rotate_level2(omr_ctx *ctx, const uint32_t *lwe_int, size_t n,
                                   uint64_t *out);
/* Test entries: the blind rotations from a caller-supplied initial accumulator acc0, u64 [n][2][N]
 * (level 1: N = 1024 mod q1; level 2: N = 2048 mod q2) of canonical residues in the coefficient
 * domain, in the layout of the matching entry's output. It replaces (0, X^-b * LUT); the LWE body
 * (lwe_b, which may then be NULL; lwe_int[670]) is ignored. With a rotation amount a = N,
 * (X^a - 1) * ACC = -2 ACC, so every decomposition input T is reachable as ACC = -T * 2^-1 mod q,
 * and an LWE with one nonzero a_i runs exactly one CMUX step on that step's key rows. acc0 == NULL
 * behaves exactly as the entry without _from. A word >= q is OMR_ERR_INVALID_ARGUMENT, checked on
 * the host before anything is enqueued. The same kernel selection, guard and fallback as the
 * matching entry, on those kernels' _from instantiations: at level 2 that includes the latency path's
 * two-CU kernels (br2y_from_kernel, or br2x_from_kernel on a guarded context or with OMR_BR2Y=0), with
 * br2l's only where the entry without _from would run br2l_kernel (the cooperative launch does not fit
 * or is refused). omr_ctx_launch_record tells which ran. */
omr_status omr_blind_rotate_level1_from(omr_ctx *ctx, const uint16_t *lwe_a, const uint16_t *lwe_b,
                                        size_t n, const uint64_t *acc0, uint64_t *out);
omr_status omr_blind_rotate_level2_from(omr_ctx *ctx, const uint32_t *lwe_int, size_t n,
                                        const uint64_t *acc0, uint64_t *out);
/* Test entry: the homomorphic trace alone (what omr_second_level runs after its rotation, with the
 * same kernel selection, guard and fallback) on n coefficient-domain RLWEs, rlwe u64 [n][2][2048]
 * canonical (a word >= q2 is OMR_ERR_INVALID_ARGUMENT): out u64 [n][2][2048], NTT domain. */
omr_status omr_trace(omr_ctx *ctx, const uint64_t *rlwe, size_t n, uint64_t *out);
/* Forward / inverse NTT of n polynomials (level 1: N=1024 mod q1, level 2: N=2048 mod q2). */
omr_status omr_ntt(int level, int inverse, uint64_t *polys, size_t n, int device);

#ifdef __cplusplus
}
#endif
#endif
