// The auditor's per-coefficient arithmetic (include/omr_gpu.h, "Auditor"), shared by the CPU statement
// (retriever.hip, omr_audit_cpu) and the device kernel (audit_kernels.hpp): exact 64-bit integers.
#pragma once

#include "common.hpp"

namespace omr {

struct DecodedCoeff {
  uint32_t t;      // decoded plaintext in [0, 257)
  uint64_t abs_r;  // |p c - t' q2|
};

// c canonical in [0, q2). t' = floor((2 p c + q2) / (2 q2)) is the round-half-up of p c / q2
// (retriever.rs:84-89); 2 p c + q2 < 515 * 2^50 < 2^60, so nothing here leaves 64 bits. r = p c - t' q2
// lies in [-q2/2, q2/2): from 2 q2 t' <= 2 p c + q2 < 2 q2 (t' + 1), and q2 is odd, so
// |r| <= (q2 - 1) / 2 < 2^49. The division is by a constant: a multiply-high and shifts on the device.
OMR_HD DecodedCoeff decode_coeff(uint64_t c) {
  const uint64_t pc = (uint64_t)P * c;
  const uint64_t tp = (2 * pc + Q2) / (2 * Q2);
  const int64_t r = (int64_t)pc - (int64_t)(tp * Q2);
  return {tp == (uint64_t)P ? 0u : (uint32_t)tp, (uint64_t)(r < 0 ? -r : r)};
}

// bits needed to write v: 0 for 0, at most 49 for a residual
OMR_HD int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// adds the tallies of `from` into `into` (omr_audit_summary is only counts and a maximum)
inline void merge_summary(omr_audit_summary &into, const omr_audit_summary &from) {
  into.ciphertexts += from.ciphertexts;
  into.zero += from.zero;
  into.one_hot += from.one_hot;
  into.other += from.other;
  if (from.max_abs_residual > into.max_abs_residual) into.max_abs_residual = from.max_abs_residual;
  for (int k = 0; k < OMR_AUDIT_RESIDUAL_BINS; ++k) into.residual_bits[k] += from.residual_bits[k];
}

}  // namespace omr
