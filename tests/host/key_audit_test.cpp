// Stand-alone host test of the key audit's CPU statement (csrc/key_audit.hip) and its arithmetic header
// (csrc/key_audit_math.hpp), meant for a build with csrc/keygen.hip under the address and undefined-behaviour
// sanitizers (make build/key_audit_test; no GPU is touched): crafted rows with exactly known noise at the
// first and last row of every component in exactly sized buffers, a generated key, the summary rules and
// the argument errors.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "key_audit_math.hpp"
#include "omr_gpu.h"

namespace {

int fails = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

using namespace omr;

struct Secrets {
  uint8_t s0[OMR_N0], sint[OMR_NI];
  int8_t s1[OMR_N1], s2[OMR_N2];
};

// One row with a = 0 and b = message + e, e = `noise` at coefficient `at` and 0 elsewhere.
template <typename T>
std::vector<T> craft(const Secrets &s, int comp, size_t row, int64_t noise, int at) {
  const KeyAuditShape c = key_audit_shape(comp);
  const uint64_t q = key_audit_modulus(c.level);
  const KeyRowMessage m = key_row_message(comp, row);
  std::vector<T> out((size_t)c.row_elems, 0);
  const int masks = c.row_elems - c.n;
  for (int j = 0; j < c.n; ++j) {
    int sign = 0;
    if (m.kind == KA_A_GADGET) sign = -(comp == OMR_KEY_BSK1 ? s.s0[m.index] * s.s1[j] : s.sint[m.index] * s.s2[j]);
    else if (m.kind == KA_B_GADGET) sign = j == 0 ? (comp == OMR_KEY_BSK1 ? s.s0[m.index] : s.sint[m.index]) : 0;
    else if (m.kind == KA_KSK) sign = s.s1[m.index];
    else {  // -sigma_g(s2)[j]: the coefficient i with i g = j or j + N mod 2N
      const uint32_t g = (uint32_t)(OMR_N2 >> m.index) + 1;
      for (int i = 0; i < OMR_N2; ++i) {
        const uint32_t e = (uint32_t)(((uint64_t)i * g) % (2 * OMR_N2));
        if (e == (uint32_t)j) sign = -s.s2[i];
        else if (e == (uint32_t)j + OMR_N2) sign = s.s2[i];
      }
    }
    uint64_t v = key_add_signed(0, sign, m.mag % q, q);
    if (j == at) v = (v + (uint64_t)((noise % (int64_t)q + (int64_t)q) % (int64_t)q)) % q;
    out[(size_t)masks + j] = (T)v;
  }
  return out;
}

template <typename T>
void crafted(const omr_secret_key_pack *sk, const Secrets &s, int comp) {
  const KeyAuditShape c = key_audit_shape(comp);
  const uint64_t q = key_audit_modulus(c.level);
  uint64_t K = 0;
  EXPECT(omr_key_noise_support(comp, &K) == OMR_OK && K >= 16);
  const size_t rows[3] = {0, c.rows / 2 + 1, c.rows - 1};
  const int64_t noises[5] = {0, (int64_t)K, -(int64_t)K, (int64_t)K + 1, -(int64_t)((q - 1) / 2)};
  for (size_t row : rows)
    for (int64_t e : noises) {
      const std::vector<T> r = craft<T>(s, comp, row, e, (int)(row % (size_t)c.n));
      uint64_t mx = ~0ull;
      omr_key_audit_summary sum = key_summary_init();
      EXPECT(omr_audit_key_rows_cpu(sk, comp, r.data(), row, 1, UINT64_MAX, &mx, &sum, 1) == OMR_OK);
      const uint64_t want = (uint64_t)(e < 0 ? -e : e);
      EXPECT(mx == want && sum.max_abs_noise == want && sum.rows == 1 && sum.noncanonical == 0);
      EXPECT(sum.rows_over == (want > K) && sum.first_row_over == (want > K ? row : UINT64_MAX));
      EXPECT(sum.noise_bits[key_noise_bits(want)] >= 1 && sum.noise_bits[0] == (uint64_t)c.n - (want != 0));
    }
}

}  // namespace

int main() {
  // the arithmetic header
  EXPECT(key_abs_centred(0, OMR_Q1) == 0 && key_abs_centred((OMR_Q1 - 1) / 2, OMR_Q1) == (OMR_Q1 - 1) / 2);
  EXPECT(key_abs_centred((OMR_Q1 + 1) / 2, OMR_Q1) == (OMR_Q1 - 1) / 2 && key_abs_centred(OMR_Q1 - 1, OMR_Q1) == 1);
  EXPECT(key_noise_bits(0) == 0 && key_noise_bits(1) == 1 && key_noise_bits((OMR_Q2 - 1) / 2) == 49 &&
         key_noise_bits((OMR_Q1 - 1) / 2) == 26);
  EXPECT(key_add_signed(5, -1, 7, OMR_Q2) == OMR_Q2 - 2 && key_add_signed(OMR_Q2 - 1, 1, 1, OMR_Q2) == 0);
  for (int comp = 0; comp < 4; ++comp) {
    const KeyAuditShape c = key_audit_shape(comp);
    const KeyRowMessage last = key_row_message(comp, c.rows - 1);
    EXPECT(last.mag < key_audit_modulus(c.level));
    EXPECT(last.index == (comp == OMR_KEY_BSK1 ? 511u : comp == OMR_KEY_KSK ? 1023u : comp == OMR_KEY_BSK2 ? 669u : 10u));
  }
  EXPECT(key_audit_shape(4).rows == 0 && key_audit_shape(-1).rows == 0);
  EXPECT(key_row_message(OMR_KEY_BSK2, 5).kind == KA_A_GADGET && key_row_message(OMR_KEY_BSK2, 6).kind == KA_B_GADGET);
  EXPECT(key_row_message(OMR_KEY_BSK1, 7).mag == 1ull << 22 && key_row_message(OMR_KEY_TRACE, 274).mag == 1ull << 48);
  omr_key_audit_summary a = key_summary_init(), b = key_summary_init();
  tally_key_row(a, 9, 100, 1, 16);
  tally_key_row(b, 4, 7, 0, 16);
  tally_key_row(b, 3, 17, 2, 16);
  merge_key_summary(a, b);
  EXPECT(a.rows == 3 && a.noncanonical == 3 && a.max_abs_noise == 100 && a.rows_over == 2 && a.first_row_over == 3);

  omr_secret_key_pack *sk = nullptr;
  EXPECT(omr_keygen_secret(42, &sk) == OMR_OK);
  Secrets s;
  EXPECT(omr_secret_export(sk, s.s0, s.s1, s.sint, s.s2) == OMR_OK);
  crafted<uint32_t>(sk, s, OMR_KEY_BSK1);
  crafted<uint32_t>(sk, s, OMR_KEY_KSK);
  crafted<uint64_t>(sk, s, OMR_KEY_BSK2);
  crafted<uint64_t>(sk, s, OMR_KEY_TRACE);

  // a generated key, exactly sized buffers: the last rows of every component, then the whole key
  std::vector<uint32_t> bsk1(4096u * 2048), ksk(27648u * 671);
  std::vector<uint64_t> bsk2(8040u * 4096), tk(275u * 4096);
  EXPECT(omr_keygen_detection_key(sk, 7, bsk1.data(), ksk.data(), bsk2.data(), tk.data(), 16) == OMR_OK);
  const void *full[4] = {bsk1.data(), ksk.data(), bsk2.data(), tk.data()};
  for (int comp = 0; comp < 4; ++comp) {
    const KeyAuditShape c = key_audit_shape(comp);
    const size_t width = c.level == 1 ? 4 : 8, first = c.rows - 3;
    uint64_t mx[3], K = 0;
    omr_key_audit_summary sum = key_summary_init();
    EXPECT(omr_key_noise_support(comp, &K) == OMR_OK);
    EXPECT(omr_audit_key_rows_cpu(sk, comp, (const unsigned char *)full[comp] + first * c.row_elems * width, first, 3,
                                  UINT64_MAX, mx, &sum, 2) == OMR_OK);
    EXPECT(sum.rows == 3 && sum.rows_over == 0 && sum.max_abs_noise <= K && sum.noncanonical == 0);
    EXPECT(mx[0] <= K && mx[1] <= K && mx[2] <= K);
    // the argument errors
    EXPECT(omr_audit_key_rows_cpu(sk, comp, full[comp], c.rows - 1, 2, 0, mx, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_audit_key_rows_cpu(sk, comp, full[comp], c.rows + 1, 0, 0, mx, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_audit_key_rows_cpu(sk, comp, full[comp], 1, (size_t)-1, 0, mx, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_audit_key_rows_cpu(sk, comp, full[comp], 0, 1, 0, nullptr, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_audit_key_rows_cpu(sk, comp, nullptr, 0, 1, 0, mx, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_audit_key_rows_cpu(sk, comp, nullptr, c.rows, 0, 0, mx, nullptr, 1) == OMR_OK);
  }
  EXPECT(omr_audit_key_rows_cpu(sk, 4, bsk1.data(), 0, 1, 0, nullptr, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  omr_key_audit_summary out[4] = {key_summary_init(), key_summary_init(), key_summary_init(), key_summary_init()};
  const omr_detection_key_view view{bsk1.data(), ksk.data(), nullptr, tk.data()};
  EXPECT(omr_audit_key_cpu(sk, &view, nullptr, out, 16) == OMR_OK);
  EXPECT(out[0].rows == 4096 && out[1].rows == 27648 && out[2].rows == 0 && out[3].rows == 275);
  EXPECT(out[0].rows_over == 0 && out[1].rows_over == 0 && out[3].rows_over == 0);
  uint64_t nc[4] = {9, 9, 9, 9};
  tk[275u * 4096 - 1] = OMR_Q2;
  ksk[0] = 0xFFFFFFFFu;
  EXPECT(omr_key_validate(&view, nc, 3) == OMR_OK);
  EXPECT(nc[0] == 0 && nc[1] == 1 && nc[2] == 9 && nc[3] == 1);
  EXPECT(omr_key_validate(nullptr, nc, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_audit_key_cpu(sk, nullptr, nullptr, out, 1) == OMR_ERR_INVALID_ARGUMENT);
  omr_secret_destroy(sk);
  std::printf(fails ? "FAILED (%d)\n" : "key audit host test OK\n", fails);
  return fails ? 1 : 0;
}
