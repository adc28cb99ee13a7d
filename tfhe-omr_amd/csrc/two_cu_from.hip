// The two-CU level-2 latency kernels from a caller-supplied accumulator (the test entry
// omr_blind_rotate_level2_from): br2y_from_kernel and br2x_from_kernel, each the text of its production
// twin (br2y_kernel_body.inc, br2x_kernel_body.inc) with ACC_r loaded from polynomial r of acc0's message
// instead of (0, X^-b LUT2). Helpers, hand-off, flags, slots and grid shape are the production kernels'.
//
// A translation unit of their own: defined beside br2x_kernel in detect.hip's device code, a second kernel
// changed the code the compiler emits for br2x_kernel itself (226 instead of 220 VGPRs, another LDS access
// pattern), and the production kernels' code must not move for a test entry. detect.hip launches them
// through the pointers below.
#undef OMR_PHASE_TRACE  // the phase buffer is detect.hip's; these kernels are not traced
#define OMR_LEVEL2_PARTS_ONLY
#include "br2_fft.hpp"
#include "br2_ntt.hpp"
#include "two_cu_from.hpp"

namespace omr {

__global__ __launch_bounds__(BR2Y_T, 1) void br2y_from_kernel(const uint32_t *__restrict__ lwe_int,
                                                              const double2 *__restrict__ bskf,
                                                              const double2 *__restrict__ twg, DeviceTables tb,
                                                              double *xg, uint32_t *flags, int *err,
                                                              uint64_t *__restrict__ out, int nmsg, int w8,
                                                              int allow_fast, const uint64_t *__restrict__ acc0) {
#define OMR_BR2Y_FROM 1
#include "br2y_kernel_body.inc"
#undef OMR_BR2Y_FROM
}

__global__ __launch_bounds__(BR2L_T, 1) void br2x_from_kernel(const uint32_t *__restrict__ lwe_int,
                                                              const double *__restrict__ bsk2, DeviceTables tb,
                                                              double *xg, uint32_t *flags, int *err,
                                                              uint64_t *__restrict__ out,
                                                              const uint64_t *__restrict__ acc0) {
#define OMR_BR2X_FROM 1
#include "br2x_kernel_body.inc"
#undef OMR_BR2X_FROM
}

const void *br2y_from_kernel_ptr() { return reinterpret_cast<const void *>(&br2y_from_kernel); }
const void *br2x_from_kernel_ptr() { return reinterpret_cast<const void *>(&br2x_from_kernel); }

}  // namespace omr
