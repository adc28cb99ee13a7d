// Key audit on the CPU (include/omr_gpu.h, "Key audit"): the statement the kernels of
// key_audit_kernels.hpp are checked against and the path of a client without a device, plus the
// secret-free canonicity count over host memory. Host code only; it links against keygen.hip alone
// (tests/host/key_audit_test.cpp builds the two without a GPU).
#include <mutex>
#include <string>
#include <vector>

#include "host_ring.hpp"
#include "key_audit_math.hpp"
#include "rng.hpp"

using namespace omr;

namespace {

// The noise of one RLWE row [a[N] | b[N]]: row_max and noncanonical returned, bins added into sum.
template <typename T>
void audit_rlwe_row(const omr_secret_key_pack *sk, int comp, size_t row, const T *p, uint64_t &row_max, uint64_t &nc,
                    omr_key_audit_summary &sum) {
  const KeyAuditShape c = key_audit_shape(comp);
  const HostNtt &tab = c.level == 1 ? ntt1() : ntt2();
  const uint64_t q = tab.q;
  const int N = c.n;
  const std::vector<uint64_t> &sn = c.level == 1 ? sk->s1_ntt : sk->s2_ntt, &sns = c.level == 1 ? sk->s1_ntts : sk->s2_ntts;
  const int8_t *s = c.level == 1 ? sk->s1 : sk->s2;
  const KeyRowMessage m = key_row_message(comp, row);
  std::vector<uint64_t> t(N);
  nc = 0;
  for (int j = 0; j < N; ++j) {
    nc += (uint64_t)p[j] >= q;
    nc += (uint64_t)p[N + j] >= q;
    t[j] = (uint64_t)p[j] % q;
  }
  tab.fwd(t.data());
  for (int j = 0; j < N; ++j) t[j] = tab.mul(t[j], sn[j], sns[j]);
  tab.inv(t.data());  // a s
  std::vector<int8_t> sg;
  int bit = 0;
  if (m.kind == KA_TRACE) {  // sigma_g(s2), as keygen_rows builds it
    const uint32_t g = (uint32_t)(N >> m.index) + 1;
    sg.resize(N);
    for (int i = 0; i < N; ++i) {
      const uint32_t e = (uint32_t)(((uint64_t)i * g) % (2 * (uint64_t)N));
      if (e < (uint32_t)N) sg[e] = s[i];
      else sg[e - N] = (int8_t)-s[i];
    }
  } else {
    bit = comp == OMR_KEY_BSK1 ? sk->s0[m.index] : sk->sint[m.index];
  }
  row_max = 0;
  for (int j = 0; j < N; ++j) {
    const uint64_t b = (uint64_t)p[N + j] % q;
    const uint64_t ph = b >= t[j] ? b - t[j] : b + q - t[j];
    const int sign = m.kind == KA_TRACE ? sg[j] : m.kind == KA_A_GADGET ? bit * s[j] : (j == 0 ? -bit : 0);
    const uint64_t e = key_abs_centred(key_add_signed(ph, sign, m.mag, q), q);
    if (e > row_max) row_max = e;
    ++sum.noise_bits[key_noise_bits(e)];
  }
}

// One key-switching row [a[670] | b]: e = b - <a, s_int> - s1_i 2^j mod q1.
void audit_ksk_row(const omr_secret_key_pack *sk, size_t row, const uint32_t *p, uint64_t &row_max, uint64_t &nc,
                   omr_key_audit_summary &sum) {
  const KeyRowMessage m = key_row_message(OMR_KEY_KSK, row);
  uint64_t acc = 0;  // 670 words below q1 < 2^27
  nc = 0;
  for (int c = 0; c < NI; ++c) {
    nc += p[c] >= Q1;
    if (sk->sint[c]) acc += p[c] % Q1;
  }
  nc += p[NI] >= Q1;
  const uint64_t as = acc % Q1, b = p[NI] % Q1;
  const uint64_t ph = b >= as ? b - as : b + Q1 - as;
  row_max = key_abs_centred(key_add_signed(ph, -(int)sk->s1[m.index], m.mag % Q1, Q1), Q1);
  ++sum.noise_bits[key_noise_bits(row_max)];
}

template <typename T>
uint64_t count_words(const T *w, size_t n, uint64_t q, int nthreads) {
  const size_t piece = (size_t)1 << 20, pieces = (n + piece - 1) / piece;
  std::vector<uint64_t> part(pieces, 0);
  parallel_for(pieces, nthreads, [&](size_t p) {
    const size_t end = std::min(n, (p + 1) * piece);
    uint64_t k = 0;
    for (size_t i = p * piece; i < end; ++i) k += (uint64_t)w[i] >= q;
    part[p] = k;
  });
  uint64_t k = 0;
  for (uint64_t v : part) k += v;
  return k;
}

omr_status range_error(const char *who, int component, size_t first_row, size_t rows) {
  const KeyAuditShape c = key_audit_shape(component);
  if (!c.rows) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": no such component");
  if (first_row > c.rows || rows > c.rows - first_row)
    return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": row range beyond the component");
  return OMR_OK;
}

}  // namespace

extern "C" omr_status omr_key_noise_support(int component, uint64_t *K) {
  // built once: the key-switching table alone has 27,065 entries (a millisecond of exponentials)
  struct Support {
    uint64_t k[4];
    Support() {
      const double sigma[4] = {SIGMA_BR1, SIGMA_KS, SIGMA_BR2, SIGMA_TRACE};
      for (int c = 0; c < 4; ++c) k[c] = (uint64_t)(Gaussian(sigma[c]).table().size() - 1);
    }
  };
  static const Support support;
  if (component < 0 || component >= 4) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_noise_support: no such component");
  if (!K) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_noise_support: K is NULL");
  *K = support.k[component];
  return OMR_OK;
}

extern "C" omr_status omr_audit_key_rows_cpu(const omr_secret_key_pack *sk, int component, const void *rows_ptr,
                                             size_t first_row, size_t rows, uint64_t limit, uint64_t *row_max,
                                             omr_key_audit_summary *summary, int nthreads) {
  if (!sk) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_cpu: NULL secret key pack");
  if (const omr_status s = range_error("omr_audit_key_rows_cpu", component, first_row, rows)) return s;
  if (!row_max && !summary) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_cpu: no output requested");
  if (rows == 0) return OMR_OK;
  if (!rows_ptr) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_cpu: NULL rows");
  if (limit == UINT64_MAX) (void)omr_key_noise_support(component, &limit);
  const KeyAuditShape c = key_audit_shape(component);
  std::mutex mu;  // guards *summary: integer tallies, so the order of the merges does not matter
  parallel_for(rows, nthreads, [&](size_t i) {
    omr_key_audit_summary one = key_summary_init();
    uint64_t mx = 0, nc = 0;
    const size_t row = first_row + i;
    if (component == OMR_KEY_KSK) audit_ksk_row(sk, row, (const uint32_t *)rows_ptr + i * c.row_elems, mx, nc, one);
    else if (c.level == 1) audit_rlwe_row<uint32_t>(sk, component, row, (const uint32_t *)rows_ptr + i * c.row_elems, mx, nc, one);
    else audit_rlwe_row<uint64_t>(sk, component, row, (const uint64_t *)rows_ptr + i * c.row_elems, mx, nc, one);
    if (row_max) row_max[i] = mx;
    if (summary) {
      tally_key_row(one, row, mx, nc, limit);
      std::lock_guard<std::mutex> lk(mu);
      merge_key_summary(*summary, one);
    }
  });
  return OMR_OK;
}

extern "C" omr_status omr_audit_key_cpu(const omr_secret_key_pack *sk, const omr_detection_key_view *key,
                                        const uint64_t limit[4], omr_key_audit_summary out[4], int nthreads) {
  if (!sk || !key || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_cpu: NULL argument");
  const void *p[4] = {key->bsk1, key->ksk, key->bsk2, key->trace_key};
  for (int c = 0; c < 4; ++c) {
    if (!p[c]) continue;
    const omr_status s = omr_audit_key_rows_cpu(sk, c, p[c], 0, key_audit_shape(c).rows, limit ? limit[c] : UINT64_MAX,
                                                nullptr, &out[c], nthreads);
    if (s != OMR_OK) return s;
  }
  return OMR_OK;
}

extern "C" omr_status omr_key_validate(const omr_detection_key_view *key, uint64_t noncanonical[4], int nthreads) {
  if (!key || !noncanonical) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_validate: NULL argument");
  if (key->bsk1) noncanonical[0] = count_words(key->bsk1, BSK1_ELEMS, Q1, nthreads);
  if (key->ksk) noncanonical[1] = count_words(key->ksk, KSK_ELEMS, Q1, nthreads);
  if (key->bsk2) noncanonical[2] = count_words(key->bsk2, BSK2_ELEMS, Q2, nthreads);
  if (key->trace_key) noncanonical[3] = count_words(key->trace_key, TK_ELEMS, Q2, nthreads);
  return OMR_OK;
}

extern "C" omr_status omr_key_validate_seeded(const omr_seeded_key_view *key, uint64_t noncanonical[4], int nthreads) {
  if (!key || !noncanonical) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_validate_seeded: NULL argument");
  if (key->bsk1_b) noncanonical[0] = count_words(key->bsk1_b, BSK1_ELEMS / 2, Q1, nthreads);
  if (key->ksk_b) noncanonical[1] = count_words(key->ksk_b, (size_t)N1 * KS_DIGITS, Q1, nthreads);
  if (key->bsk2_b) noncanonical[2] = count_words(key->bsk2_b, BSK2_ELEMS / 2, Q2, nthreads);
  if (key->trace_key_b) noncanonical[3] = count_words(key->trace_key_b, TK_ELEMS / 2, Q2, nthreads);
  return OMR_OK;
}
