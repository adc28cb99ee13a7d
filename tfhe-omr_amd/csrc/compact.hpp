// What compact.hip lends the other host translation units (digest.hip, audit.hip): the launches of the
// two kernels of compact_kernels.hpp, which only compact.hip includes. Both enqueue on st and return;
// the device of the buffers is current; bits is valid; n > 0; every pointer is 16-byte aligned.
#pragma once

#include "compact_math.hpp"
#include "hip_util.hpp"

namespace omr {

// workgroups of a launch over n ciphertexts: `grid` if set, else six per compute unit, never more than n
unsigned compact_grid(unsigned grid, int num_cu, size_t n);
// d_out = the n compact ciphertexts (512 bits bytes each) of d_cts u64 [n][2][2048]; itw: level-2 inverse twiddles
omr_status launch_compact(const uint64_t *d_cts, size_t n, int bits, const double *d_itw, unsigned grid,
                          void *d_out, hipStream_t st);
// d_cts = the n NttRlweCiphertexts of d_packed; tw: level-2 forward twiddles
omr_status launch_expand(const void *d_packed, size_t n, int bits, const double *d_tw, unsigned grid,
                         uint64_t *d_cts, hipStream_t st);

}  // namespace omr
