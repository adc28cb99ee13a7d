// Host-side key generation and clue generation (CPU), the sender over public clue keys with the
// recipient's clue opening and clue-key audit, and the library's error text. The payload weights and the
// digest layout are in weights.hip.
//
// Mirrors omr_core's KeyGen / SecretKeyPack / Sender (key_gen/mod.rs:16-27,
// key_gen/secret.rs:46-209, key_gen/clue.rs:27-34, sender.rs:27-32). Every random draw comes
// from a ChaCha12 stream keyed by (seed, domain) whose stream id is the key row (or the global
// message index for clues), so results do not depend on thread count or sharding.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_ring.hpp"
#include "rng.hpp"
#include "sender.hpp"

namespace omr {

static thread_local std::string g_last_error;

omr_status set_error(omr_status st, const std::string &msg) {
  g_last_error = msg;
  return st;
}

}  // namespace omr

// ==========================================================================================
// SecretKeyPack (key_gen/secret.rs:17-95)
// ==========================================================================================

using namespace omr;

extern "C" const char *omr_last_error(void) { return omr::g_last_error.c_str(); }
extern "C" const char *omr_version(void) { return "omr_gpu 0.1 gfx950"; }

extern "C" omr_status omr_keygen_secret(uint64_t seed, omr_secret_key_pack **out) {
  if (!out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_keygen_secret: out is NULL");
  auto sk = std::make_unique<omr_secret_key_pack>();
  sk->seed = seed;
  {
    Stream s(seed, DOM_S0, 0);
    for (int i = 0; i < N0; ++i) sk->s0[i] = (uint8_t)s.bit();
  }
  {
    Stream s(seed, DOM_S1, 0);
    for (int i = 0; i < N1; ++i) sk->s1[i] = (int8_t)s.ternary();
  }
  {
    Stream s(seed, DOM_SINT, 0);
    for (int i = 0; i < NI; ++i) sk->sint[i] = (uint8_t)s.bit();
  }
  {
    Stream s(seed, DOM_S2, 0);
    for (int i = 0; i < N2; ++i) sk->s2[i] = (int8_t)s.ternary();
  }
  {  // public key: B = A * s0 + E over Z_2048[X]/(X^512+1)
    Stream sa(seed, DOM_PK_A, 0), se(seed, DOM_PK_E, 0);
    Gaussian g(SIGMA_CLUE);
    int32_t b[N0];
    for (int i = 0; i < N0; ++i) sk->pk_a[i] = (uint16_t)(sa.next32() & (Q0 - 1));
    for (int i = 0; i < N0; ++i) b[i] = (int32_t)g.sample(se);
    for (int t = 0; t < N0; ++t) {
      if (!sk->s0[t]) continue;
      for (int i = 0; i < N0; ++i) {
        int e = i + t;
        if (e < N0) b[e] += sk->pk_a[i];
        else b[e - N0] -= sk->pk_a[i];
      }
    }
    for (int i = 0; i < N0; ++i) sk->pk_b[i] = (uint16_t)(((b[i] % Q0) + Q0) % Q0);
  }
  auto ntt_of = [](const int8_t *s, int N, uint64_t q, const auto &tab, std::vector<uint64_t> &v,
                   std::vector<uint64_t> &vs) {
    v.resize(N);
    vs.resize(N);
    for (int i = 0; i < N; ++i) v[i] = to_mod(s[i], q);
    tab.fwd(v.data());
    for (int i = 0; i < N; ++i) vs[i] = tab.pre(v[i]);
  };
  ntt_of(sk->s1, N1, Q1, ntt1(), sk->s1_ntt, sk->s1_ntts);
  ntt_of(sk->s2, N2, Q2, ntt2(), sk->s2_ntt, sk->s2_ntts);
  *out = sk.release();
  return OMR_OK;
}

extern "C" void omr_secret_destroy(omr_secret_key_pack *sk) { delete sk; }

extern "C" omr_status omr_secret_export(const omr_secret_key_pack *sk, uint8_t *s0, int8_t *s1,
                                        uint8_t *s_int, int8_t *s2) {
  if (!sk) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_secret_export: sk is NULL");
  if (s0) memcpy(s0, sk->s0, sizeof(sk->s0));
  if (s1) memcpy(s1, sk->s1, sizeof(sk->s1));
  if (s_int) memcpy(s_int, sk->sint, sizeof(sk->sint));
  if (s2) memcpy(s2, sk->s2, sizeof(sk->s2));
  return OMR_OK;
}

namespace omr {
namespace {
// RLWE encryption of zero with mask alpha (uniform draws of `sa`) and noise from `se` (the same stream
// for a plain key), plus m*g in component `comp` of coefficient 0:
// row = (alpha + [comp==0] m g, alpha*s + e + [comp==1] m g). Writes canonical residues.
// Seeded rows (s_fold = the ternary coefficients of s, out_a may be NULL) keep a = alpha, a function of
// the public mask seed alone, and put the a-gadget into the body: b = alpha*s + e - m g s, the same
// phase e - m g s as the row above.
template <typename T>
void ggsw_row(Stream &sa, Stream &se, const Gaussian &gauss, const HostNtt &tab,
              const std::vector<uint64_t> &s_ntt, const std::vector<uint64_t> &s_ntts, uint64_t mg, int comp,
              T *out_a, T *out_b, const int8_t *sigma_s = nullptr, uint64_t sigma_scale = 0,
              const int8_t *s_fold = nullptr) {
  const int N = tab.N;
  const uint64_t q = tab.q;
  std::vector<uint64_t> a(N), t(N);
  for (int j = 0; j < N; ++j) a[j] = sa.uniform(q);
  for (int j = 0; j < N; ++j) t[j] = a[j];
  tab.fwd(t.data());
  for (int j = 0; j < N; ++j) t[j] = tab.mul(t[j], s_ntt[j], s_ntts[j]);
  tab.inv(t.data());  // alpha * s
  for (int j = 0; j < N; ++j) {
    uint64_t b = t[j] + to_mod(gauss.sample(se), q);
    b = b >= q ? b - q : b;
    if (sigma_s && sigma_s[j]) {  // - sigma_g(s) * scale
      uint64_t c = mulmod(sigma_scale, (uint64_t)(sigma_s[j] < 0 ? q - 1 : 1), q);
      b = b >= c ? b - c : b + q - c;
    }
    if (s_fold && comp == 0 && mg && s_fold[j]) {  // - m g s
      const uint64_t c = s_fold[j] < 0 ? q - mg : mg;
      b = b >= c ? b - c : b + q - c;
    }
    t[j] = b;
  }
  if (mg) {
    if (comp == 1) t[0] = (t[0] + mg) % q;
    else if (!s_fold) a[0] = (a[0] + mg) % q;
  }
  for (int j = 0; j < N; ++j) {
    if (out_a) out_a[j] = (T)a[j];
    out_b[j] = (T)t[j];
  }
}

// The first `n` accepted draws of Stream(mask_seed, dom, row).uniform(q): the mask of a seeded row.
template <typename T>
void mask_row(uint64_t mask_seed, uint32_t dom, uint64_t row, uint64_t q, int n, T *out) {
  Stream st(mask_seed, dom, row);
  for (int j = 0; j < n; ++j) out[j] = (T)st.uniform(q);
}

// Every row of a detection key. Plain (mask_seed NULL): one stream per row draws the mask and then the
// noise, rows (a, b) in the layout of include/omr_gpu.h. Seeded: the mask from the public stream, the
// noise from word 0 of the noise stream, and only the bodies are written (bsk1 [4096][1024],
// ksk [27648], bsk2 [8040][2048], tk [275][2048]).
omr_status keygen_rows(const omr_secret_key_pack *sk, uint64_t seed, const uint64_t *mask_seed, uint32_t *bsk1,
                       uint32_t *ksk, uint64_t *bsk2, uint64_t *tk, int nthreads) {
  const bool sd = mask_seed != nullptr;
  const uint64_t ms = sd ? *mask_seed : 0;
  const Gaussian g1(SIGMA_BR1), gks(SIGMA_KS), g2(SIGMA_BR2), gt(SIGMA_TRACE);
  // BSK1: BlindRotationKey::generate(s0, NTT(s1), basis(q1,5,4), sigma 3.1859), :124-131
  parallel_for((size_t)N0 * 2 * D1, nthreads, [&](size_t row) {
    const size_t i = row / (2 * D1);
    const int r = (int)(row % (2 * D1));
    Stream st(seed, sd ? DOM_BSK1_NOISE : DOM_BSK1, row), sm(ms, DOM_BSK1_MASK, row);
    const int k = r < D1 ? r : r - D1;
    const uint64_t mg = sk->s0[i] ? (1ull << (DROP1 + k * LOGB1)) : 0;
    uint32_t *oa = sd ? nullptr : bsk1 + row * 2 * N1, *ob = sd ? bsk1 + row * N1 : oa + N1;
    ggsw_row<uint32_t>(sd ? sm : st, st, g1, ntt1(), sk->s1_ntt, sk->s1_ntts, mg, r < D1 ? 0 : 1, oa, ob, nullptr, 0,
                       sd ? sk->s1 : nullptr);
  });
  // KSK: NonPowOf2LweKeySwitchingKey::generate(s1 (-1 -> q1-1), s_int, ...), :133-147
  parallel_for((size_t)N1 * KS_DIGITS, nthreads, [&](size_t row) {
    const size_t i = row / KS_DIGITS;
    const int j = (int)(row % KS_DIGITS);
    Stream st(seed, sd ? DOM_KSK_NOISE : DOM_KSK, row), sm(ms, DOM_KSK_MASK, row);
    Stream &sa = sd ? sm : st;
    uint32_t *o = sd ? nullptr : ksk + row * (NI + 1);
    uint64_t b = 0;
    for (int c = 0; c < NI; ++c) {
      uint64_t a = sa.uniform(Q1);
      if (o) o[c] = (uint32_t)a;
      if (sk->sint[c]) b += a;
    }
    b %= Q1;
    b = (b + to_mod(gks.sample(st), Q1)) % Q1;
    const uint64_t m = mulmod(to_mod(sk->s1[i], Q1), (1ull << j) % Q1, Q1);
    (sd ? ksk[row] : o[NI]) = (uint32_t)((b + m) % Q1);
  });
  // BSK2: BlindRotationKey::generate(s_int, NTT(s2), basis(q2,7,6), sigma 0.3908), :149-156
  parallel_for((size_t)NI * 2 * D2, nthreads, [&](size_t row) {
    const size_t i = row / (2 * D2);
    const int r = (int)(row % (2 * D2));
    Stream st(seed, sd ? DOM_BSK2_NOISE : DOM_BSK2, row), sm(ms, DOM_BSK2_MASK, row);
    const int k = r < D2 ? r : r - D2;
    const uint64_t mg = sk->sint[i] ? (1ull << (DROP2 + k * LOGB2)) : 0;
    uint64_t *oa = sd ? nullptr : bsk2 + row * 2 * N2, *ob = sd ? bsk2 + row * N2 : oa + N2;
    ggsw_row<uint64_t>(sd ? sm : st, st, g2, ntt2(), sk->s2_ntt, sk->s2_ntts, mg, r < D2 ? 0 : 1, oa, ob, nullptr, 0,
                       sd ? sk->s2 : nullptr);
  });
  // TraceKey::new(s2, NTT(s2), basis(q2,2,None), sigma 0.3908), :158-165
  parallel_for((size_t)TRACE_STEPS * DT, nthreads, [&](size_t row) {
    const int k = (int)(row / DT), j = (int)(row % DT);
    const uint32_t g = (uint32_t)(N2 >> k) + 1;
    int8_t sg[N2];
    for (int i = 0; i < N2; ++i) {
      uint32_t e = (uint32_t)(((uint64_t)i * g) % (2 * N2));
      if (e < (uint32_t)N2) sg[e] = sk->s2[i];
      else sg[e - N2] = (int8_t)-sk->s2[i];
    }
    Stream st(seed, sd ? DOM_TK_NOISE : DOM_TK, row), sm(ms, DOM_TK_MASK, row);
    uint64_t *oa = sd ? nullptr : tk + row * 2 * N2, *ob = sd ? tk + row * N2 : oa + N2;
    ggsw_row<uint64_t>(sd ? sm : st, st, gt, ntt2(), sk->s2_ntt, sk->s2_ntts, 0, 1, oa, ob, sg, (1ull << (2 * j)) % Q2);
  });
  return OMR_OK;
}

// Masks of rows [first, first + rows) of component c into out + i * stride (elements of the component).
template <typename T>
void mask_rows(const KeyComponent &c, uint64_t mask_seed, size_t first, size_t rows, T *out, size_t stride,
               int nthreads) {
  const uint64_t q = c.level == 1 ? Q1 : Q2;
  parallel_for(rows, nthreads, [&](size_t i) { mask_row<T>(mask_seed, c.mask_dom, first + i, q, c.masks, out + i * stride); });
}

// One component of a seeded key -> rows (mask, body) in the standard layout.
template <typename T>
void expand_component(int comp, uint64_t mask_seed, const T *body, T *out, int nthreads) {
  const KeyComponent &c = *key_component(comp);
  mask_rows<T>(c, mask_seed, 0, c.rows, out, (size_t)c.row_elems, nthreads);
  parallel_for(c.rows, nthreads, [&](size_t r) {
    memcpy(out + r * c.row_elems + c.masks, body + r * c.body(), c.body() * sizeof(T));
  });
}
}  // namespace
}  // namespace omr

// DetectionKey (key_gen/secret.rs:118-178).
extern "C" omr_status omr_keygen_detection_key(const omr_secret_key_pack *sk, uint64_t seed,
                                               uint32_t *bsk1, uint32_t *ksk, uint64_t *bsk2,
                                               uint64_t *tk, int nthreads) {
  if (!sk || !bsk1 || !ksk || !bsk2 || !tk)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_keygen_detection_key: NULL argument");
  return keygen_rows(sk, seed, nullptr, bsk1, ksk, bsk2, tk, nthreads);
}

// Seeded detection key (include/omr_gpu.h): the bodies of a key whose masks come from mask_seed.
extern "C" omr_status omr_keygen_seeded_key(const omr_secret_key_pack *sk, uint64_t seed, uint64_t mask_seed,
                                            uint32_t *bsk1_b, uint32_t *ksk_b, uint64_t *bsk2_b,
                                            uint64_t *tk_b, int nthreads) {
  if (!sk || !bsk1_b || !ksk_b || !bsk2_b || !tk_b)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_keygen_seeded_key: NULL argument");
  return keygen_rows(sk, seed, &mask_seed, bsk1_b, ksk_b, bsk2_b, tk_b, nthreads);
}

extern "C" omr_status omr_expand_detection_key(const omr_seeded_key_view *key, uint32_t *bsk1, uint32_t *ksk,
                                               uint64_t *bsk2, uint64_t *tk, int nthreads) {
  if (!key || !key->bsk1_b || !key->ksk_b || !key->bsk2_b || !key->trace_key_b || !bsk1 || !ksk || !bsk2 || !tk)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_expand_detection_key: NULL argument");
  expand_component<uint32_t>(OMR_KEY_BSK1, key->mask_seed, key->bsk1_b, bsk1, nthreads);
  expand_component<uint32_t>(OMR_KEY_KSK, key->mask_seed, key->ksk_b, ksk, nthreads);
  expand_component<uint64_t>(OMR_KEY_BSK2, key->mask_seed, key->bsk2_b, bsk2, nthreads);
  expand_component<uint64_t>(OMR_KEY_TRACE, key->mask_seed, key->trace_key_b, tk, nthreads);
  return OMR_OK;
}

extern "C" omr_status omr_key_masks(uint64_t mask_seed, int component, size_t first_row, size_t rows, void *out) {
  const KeyComponent *c = key_component(component);
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_masks: no such component");
  if (first_row > c->rows || rows > c->rows - first_row)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_masks: row range beyond the component");
  if (rows && !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_masks: out is NULL");
  if (c->level == 1) mask_rows<uint32_t>(*c, mask_seed, first_row, rows, (uint32_t *)out, (size_t)c->masks, 0);
  else mask_rows<uint64_t>(*c, mask_seed, first_row, rows, (uint64_t *)out, (size_t)c->masks, 0);
  return OMR_OK;
}

// Sender::gen_clues: ClueKey::gen_clues -> LwePublicKeyRlweMode::encrypt_multi_messages(&[0;7]).
// u = A*r + e1, v = B*r + e2 (+ Delta*m = 0), r binary; clue = (u, v[0..7]). One body over a key (A, B)
// for the pack's own key (omr_gen_clues) and a sender's table (omr_sender_gen_clues): the clue of global
// message index g from Stream(seed, DOM_CLUE, g).
namespace omr {
namespace {
void clue_body(const uint16_t *A, const uint16_t *B, const Gaussian &g, uint64_t seed, uint64_t index, uint16_t *ca,
               uint16_t *cb) {
  Stream st(seed, DOM_CLUE, index);
  uint8_t r[N0];
  for (int w = 0; w < N0 / 32; ++w) {
    uint32_t v = st.next32();
    for (int b = 0; b < 32; ++b) r[w * 32 + b] = (uint8_t)((v >> b) & 1u);
  }
  int32_t u[N0];
  for (int i = 0; i < N0; ++i) u[i] = (int32_t)g.sample(st);
  for (int t = 0; t < N0; ++t) {
    if (!r[t]) continue;
    for (int i = 0; i < N0 - t; ++i) u[i + t] += A[i];
    for (int i = N0 - t; i < N0; ++i) u[i + t - N0] -= A[i];
  }
  for (int i = 0; i < N0; ++i) ca[i] = (uint16_t)(((u[i] % Q0) + Q0) % Q0);
  for (int i = 0; i < CLUES; ++i) {
    int32_t v = (int32_t)g.sample(st);
    for (int t = 0; t <= i; ++t)
      if (r[t]) v += B[i - t];
    for (int t = i + 1; t < N0; ++t)
      if (r[t]) v -= B[N0 + i - t];
    cb[i] = (uint16_t)(((v % Q0) + Q0) % Q0);
  }
}

// (c * s0)[i] of the negacyclic product, i < 7, words of c reduced mod 2048: <a^(i), s0> of the extraction.
inline int32_t clue_dot(const uint16_t *c, const uint8_t *s0, int i) {
  int32_t acc = 0;
  for (int k = 0; k <= i; ++k) acc += (c[k] & (Q0 - 1)) * s0[i - k];
  for (int k = i + 1; k < N0; ++k) acc -= (c[k] & (Q0 - 1)) * s0[N0 + i - k];
  return acc;
}

uint64_t clue_noise_support() {
  static const uint64_t k = (uint64_t)(Gaussian(SIGMA_CLUE).table().size() - 1);
  return k;
}
}  // namespace
}  // namespace omr

extern "C" omr_status omr_gen_clues(const omr_secret_key_pack *sk, uint64_t seed, uint64_t first,
                                    size_t count, uint16_t *clue_a, uint16_t *clue_b,
                                    int nthreads) {
  if (!sk || !clue_a || !clue_b)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_gen_clues: NULL argument");
  const Gaussian g(SIGMA_CLUE);
  parallel_for(count, nthreads, [&](size_t m) {
    clue_body(sk->pk_a, sk->pk_b, g, seed, first + m, clue_a + m * N0, clue_b + m * CLUES);
  });
  return OMR_OK;
}

// ==========================================================================================
// Sender (include/omr_gpu.h "Sender"): the clue key as a value, its checks, the sender handle and the
// recipient's clue opening on the CPU. The device entries are in keygen_gpu.hip.
// ==========================================================================================
extern "C" omr_status omr_secret_clue_key(const omr_secret_key_pack *sk, omr_clue_key *out) {
  if (!sk || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_secret_clue_key: NULL argument");
  memcpy(out->a, sk->pk_a, sizeof(out->a));
  memcpy(out->b, sk->pk_b, sizeof(out->b));
  return OMR_OK;
}

extern "C" omr_status omr_clue_key_validate(const omr_clue_key *keys, size_t n_keys, uint64_t *noncanonical) {
  if (!noncanonical || (n_keys && !keys))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_key_validate: NULL argument");
  uint64_t n = 0;
  for (size_t k = 0; k < n_keys; ++k)
    for (int i = 0; i < N0; ++i) n += (keys[k].a[i] >= Q0) + (keys[k].b[i] >= Q0);
  *noncanonical = n;
  return OMR_OK;
}

extern "C" omr_status omr_clue_key_noise_support(uint64_t *K) {
  if (!K) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_key_noise_support: K is NULL");
  *K = clue_noise_support();
  return OMR_OK;
}

extern "C" omr_status omr_clue_key_audit(const omr_secret_key_pack *sk, const omr_clue_key *key, uint64_t limit,
                                         uint64_t *max_abs_noise, uint32_t *coeffs_over, uint32_t *noncanonical) {
  if (!sk || !key) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_key_audit: NULL argument");
  if (limit == UINT64_MAX) limit = clue_noise_support();
  int32_t as[N0] = {0};  // A * s0, negacyclic, words reduced mod 2048
  uint32_t nc = 0, over = 0;
  uint64_t mx = 0;
  for (int i = 0; i < N0; ++i) nc += (key->a[i] >= Q0) + (key->b[i] >= Q0);
  for (int t = 0; t < N0; ++t) {
    if (!sk->s0[t]) continue;
    for (int i = 0; i < N0 - t; ++i) as[i + t] += key->a[i] & (Q0 - 1);
    for (int i = N0 - t; i < N0; ++i) as[i + t - N0] -= key->a[i] & (Q0 - 1);
  }
  for (int i = 0; i < N0; ++i) {
    const int32_t e = ((((key->b[i] & (Q0 - 1)) - as[i]) % Q0 + Q0 + Q0 / 2) % Q0) - Q0 / 2;  // [-1024, 1023]
    const uint64_t ab = (uint64_t)(e < 0 ? -e : e);
    mx = std::max(mx, ab);
    over += ab > limit;
  }
  if (max_abs_noise) *max_abs_noise = mx;
  if (coeffs_over) *coeffs_over = over;
  if (noncanonical) *noncanonical = nc;
  return OMR_OK;
}

extern "C" omr_status omr_sender_create(const omr_clue_key *keys, size_t n_keys, int device, omr_sender **out) {
  if (!keys || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_create: NULL argument");
  if (n_keys == 0 || n_keys > UINT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_create: n_keys must be in [1, 2^32)");
  for (size_t k = 0; k < n_keys; ++k)
    for (int i = 0; i < N0; ++i)
      if (keys[k].a[i] >= Q0 || keys[k].b[i] >= Q0)
        return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_create: key " + std::to_string(k) + " has a word >= 2048");
  static_assert(sizeof(omr_clue_key) == 2 * N0 * sizeof(uint16_t), "omr_clue_key is a then b, no padding");
  auto s = std::make_unique<omr_sender>();
  s->n_keys = n_keys;
  const uint16_t *words = reinterpret_cast<const uint16_t *>(keys);
  s->keys.assign(words, words + n_keys * 2 * N0);
  if (device >= 0) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device >= ndev) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_create: no such device");
    HIP_TRY(hipSetDevice(device));
    const Gaussian g(SIGMA_CLUE);
    const unsigned long long none = SENDER_NO_ERROR;
    HIP_TRY(s->d_keys.upload_sync(s->keys));
    HIP_TRY(s->d_cdt.upload_sync(g.table()));
    HIP_TRY(s->d_err.upload_sync(&none, 1));
    s->cdt_n = (int)g.table().size();
    s->device = device;
  }
  *out = s.release();
  return OMR_OK;
}

extern "C" void omr_sender_destroy(omr_sender *s) {
  if (!s) return;
  if (s->device >= 0) (void)hipSetDevice(s->device);
  delete s;
}

extern "C" omr_status omr_sender_gen_clues(const omr_sender *s, const uint32_t *recipient, uint64_t seed, uint64_t first,
                                           size_t count, uint16_t *clue_a, uint16_t *clue_b, int nthreads) {
  if (!s || (count && (!clue_a || !clue_b)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_gen_clues: NULL argument");
  if (recipient)
    for (size_t m = 0; m < count; ++m)
      if (recipient[m] >= s->n_keys)
        return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_gen_clues: recipient of message " + std::to_string(m) +
                                                       " is not a key of the table");
  const Gaussian g(SIGMA_CLUE);
  parallel_for(count, nthreads, [&](size_t m) {
    const uint16_t *key = s->keys.data() + (size_t)(recipient ? recipient[m] : 0) * 2 * N0;
    clue_body(key, key + N0, g, seed, first + m, clue_a + m * N0, clue_b + m * CLUES);
  });
  return OMR_OK;
}

extern "C" omr_status omr_clue_open(const omr_secret_key_pack *sk, const uint16_t *clue_a, const uint16_t *clue_b,
                                    size_t count, uint8_t *values, uint8_t *pertinent, uint8_t *max_abs_noise,
                                    int nthreads) {
  if (!sk || (!values && !pertinent && !max_abs_noise))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_open: NULL secret key pack or no output requested");
  if (count == 0) return OMR_OK;
  if (!clue_a || !clue_b) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_open: NULL clues");
  parallel_for(count, nthreads, [&](size_t m) {
    int any = 0, mx = 0;
    for (int i = 0; i < CLUES; ++i) {
      const int phase = (((clue_b[m * CLUES + i] & (Q0 - 1)) - clue_dot(clue_a + m * N0, sk->s0, i)) % Q0 + Q0) % Q0;
      const int value = ((8 * phase + Q0 / 2) >> 11) & 7;
      const int noise = ((phase - 256 * value + Q0 + Q0 / 2) % Q0) - Q0 / 2;  // [-128, 127]
      any |= value;
      mx = std::max(mx, noise < 0 ? -noise : noise);
      if (values) values[m * CLUES + i] = (uint8_t)value;
    }
    if (pertinent) pertinent[m] = (uint8_t)(any == 0);
    if (max_abs_noise) max_abs_noise[m] = (uint8_t)mx;
  });
  return OMR_OK;
}
