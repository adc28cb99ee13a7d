// The key audit's per-row arithmetic (include/omr_gpu.h, "Key audit"), shared by the CPU statement
// (key_audit.hip), the kernels (key_audit_kernels.hpp) and their launch code (audit.hip): which message
// keygen_rows (keygen.hip) puts into a row, centring, the bit length of a noise value and the merge of two
// summaries. Exact integers; plain C++ apart from the host/device marker, no HIP header.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/omr_gpu.h"

#ifdef __HIPCC__
#define OMR_KA_HD __host__ __device__ inline
#else
#define OMR_KA_HD inline
#endif

namespace omr {

// What a row encrypts besides its noise, from the component and the row index alone. With phase = b - a s:
//   KA_A_GADGET  e = phase + mag * bit[index] * s       (coefficient-wise; plain and seeded layouts alike)
//   KA_B_GADGET  e = phase - mag * bit[index] at coefficient 0
//   KA_TRACE     e = phase + mag * sigma_g(s2), g = 2048 / 2^index + 1
//   KA_KSK       e = phase - s1[index] * mag            (phase = b - <a, s_int>, one value)
enum KeyRowKind : int { KA_A_GADGET = 0, KA_B_GADGET = 1, KA_TRACE = 2, KA_KSK = 3 };
struct KeyRowMessage {
  int kind;
  uint32_t index;  // secret bit i (BSK), trace step k, s1 coefficient i (KSK)
  uint64_t mag;    // 2^(drop + k logB), 4^j (both below q / 2 of their level), 2^j (below q1)
};

// geometry of the audited components (the parameter set of include/omr_gpu.h; csrc/common.hpp)
struct KeyAuditShape {
  size_t rows;
  int n;          // noise values per row: N for an RLWE row, 1 for a key-switching row
  int row_elems;  // words per row
  int level;      // 1: u32 mod q1, 2: u64 mod q2
  int d, drop, logb;
};
OMR_KA_HD KeyAuditShape key_audit_shape(int comp) {
  switch (comp) {
    case OMR_KEY_BSK1: return {(size_t)OMR_N0 * 8, OMR_N1, 2 * OMR_N1, 1, 4, 7, 5};
    case OMR_KEY_KSK: return {(size_t)OMR_N1 * OMR_KS_DIGITS, 1, OMR_NI + 1, 1, OMR_KS_DIGITS, 0, 1};
    case OMR_KEY_BSK2: return {(size_t)OMR_NI * 12, OMR_N2, 2 * OMR_N2, 2, 6, 8, 7};
    case OMR_KEY_TRACE: return {(size_t)OMR_TRACE_STEPS * OMR_TRACE_DIGITS, OMR_N2, 2 * OMR_N2, 2, OMR_TRACE_DIGITS, 0, 2};
    default: return {0, 0, 0, 0, 0, 0, 0};
  }
}
OMR_KA_HD uint64_t key_audit_modulus(int level) { return level == 1 ? (uint64_t)OMR_Q1 : (uint64_t)OMR_Q2; }

// comp is a valid component and row < key_audit_shape(comp).rows
OMR_KA_HD KeyRowMessage key_row_message(int comp, size_t row) {
  const KeyAuditShape c = key_audit_shape(comp);
  if (comp == OMR_KEY_BSK1 || comp == OMR_KEY_BSK2) {
    const int r = (int)(row % (size_t)(2 * c.d)), k = r % c.d;
    return {r < c.d ? KA_A_GADGET : KA_B_GADGET, (uint32_t)(row / (size_t)(2 * c.d)), (uint64_t)1 << (c.drop + k * c.logb)};
  }
  const int j = (int)(row % (size_t)c.d);
  const uint32_t i = (uint32_t)(row / (size_t)c.d);
  if (comp == OMR_KEY_TRACE) return {KA_TRACE, i, (uint64_t)1 << (2 * j)};
  return {KA_KSK, i, (uint64_t)1 << j};
}

// v canonical in [0, q), sign in {-1, 0, 1}, 0 < mag < q: v + sign * mag mod q, canonical
OMR_KA_HD uint64_t key_add_signed(uint64_t v, int sign, uint64_t mag, uint64_t q) {
  if (sign == 0) return v;
  const uint64_t m = sign > 0 ? mag : q - mag;
  const uint64_t t = v + m;  // < 2 q < 2^64
  return t >= q ? t - q : t;
}
// |centred representative| of v canonical in [0, q), q odd: at most (q - 1) / 2
OMR_KA_HD uint64_t key_abs_centred(uint64_t v, uint64_t q) { return v > (q - 1) / 2 ? q - v : v; }
// bits needed to write |e|: 0 for 0, at most 49 at level 2 and 26 at level 1
OMR_KA_HD int key_noise_bits(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// a summary to add into: zeros, and no row over the limit yet
inline omr_key_audit_summary key_summary_init() {
  omr_key_audit_summary s{};
  s.first_row_over = UINT64_MAX;
  return s;
}
// adds the tallies of `from` into `into`: counts, a maximum and a minimum, so the order does not matter
inline void merge_key_summary(omr_key_audit_summary &into, const omr_key_audit_summary &from) {
  into.rows += from.rows;
  into.noncanonical += from.noncanonical;
  if (from.max_abs_noise > into.max_abs_noise) into.max_abs_noise = from.max_abs_noise;
  into.rows_over += from.rows_over;
  if (from.first_row_over < into.first_row_over) into.first_row_over = from.first_row_over;
  for (int k = 0; k < OMR_AUDIT_RESIDUAL_BINS; ++k) into.noise_bits[k] += from.noise_bits[k];
}
// one audited row into a summary: bins are added by the caller (one per noise value)
inline void tally_key_row(omr_key_audit_summary &s, uint64_t component_row, uint64_t row_max, uint64_t noncanonical,
                          uint64_t limit) {
  ++s.rows;
  s.noncanonical += noncanonical;
  if (row_max > s.max_abs_noise) s.max_abs_noise = row_max;
  if (row_max > limit) {
    ++s.rows_over;
    if (component_row < s.first_row_over) s.first_row_over = component_row;
  }
}

}  // namespace omr
