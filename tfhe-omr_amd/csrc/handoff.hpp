// Hand-offs between the workgroups of a cooperative latency kernel (br2x_kernel, br2y_kernel,
// trace_x_kernel) through global memory: the sc1 accesses, the flag protocol, and the geometry of
// the payload slots and flags, which the kernels index and the host (detect.hip) allocates from the
// same functions and constants. Also the phase timestamps of the latency kernels.
//
// Protocol (MI355X_MICROARCH.md, inter-workgroup visibility, the first row of the sc1 table): every
// storing thread stores its payload with sc1 stores (agent-scope relaxed atomics) and waits
// vmcnt(0); a workgroup barrier; one lane stores the sc1 flag (the hand-off's number + 1). The
// consumer's lane 0 polls each partner's flag with sc1 loads, a workgroup barrier follows, and
// every load of the payload is an sc1 load. The payload slot is the hand-off's parity, so
// consecutive hand-offs alternate slots, and before a workgroup rewrites slot h & 1 (at hand-off
// h + 2) it has seen every partner's flag h + 2, which a partner publishes only after its
// hand-off-h read of that slot was consumed. The poll is bounded: after BR2X_SPIN polls the
// workgroup records an error in *err and leaves its loop, so every wave exits. The grid must be
// co-resident: the host launches it with hipLaunchCooperativeKernel, which guarantees that or
// refuses the launch.
#pragma once

#include "kernels.hpp"

namespace omr {

// Phase timestamps of the latency kernels (tools/phase_trace.py; built only with
// -DOMR_PHASE_TRACE): lane 0 of each traced wave stores clock64() at the phase boundaries of
// executed steps PT_S0 .. PT_S0 + PT_STEPS - 1 (slots 0..7: br1l workgroup 0, waves 0..7; slots
// 8..23: br2x workgroups 0, 1, waves 0..7), plus clock64 / wall_clock64 pairs at kernel entry and
// exit for the clock rate.
#ifdef OMR_PHASE_TRACE
constexpr int PT_S0 = 200, PT_STEPS = 64, PT_K = 8, PT_SLOTS = 32;
__device__ unsigned long long omr_phase_buf[PT_SLOTS * PT_STEPS * PT_K + PT_SLOTS * 4];
__device__ __forceinline__ void phase_mark(int slot, int step, int k) {
  if (slot >= 0 && (threadIdx.x & 63) == 0 && step >= PT_S0 && step < PT_S0 + PT_STEPS)
    omr_phase_buf[(slot * PT_STEPS + (step - PT_S0)) * PT_K + k] = clock64();
}
__device__ __forceinline__ void phase_clock(int slot, int k) {  // k 0: entry, 1: exit
  if (slot >= 0 && (threadIdx.x & 63) == 0) {
    unsigned long long *p = omr_phase_buf + PT_SLOTS * PT_STEPS * PT_K + slot * 4 + 2 * k;
    p[0] = clock64();
    p[1] = wall_clock64();
  }
}
#define OMR_PHASE(slot, step, k) phase_mark(slot, step, k)
#define OMR_PHASE_CLOCK(slot, k) phase_clock(slot, k)
#else  // the slot stays "used", so a kernel needs no (void) of its own for it
#define OMR_PHASE(slot, step, k) ((void)(slot))
#define OMR_PHASE_CLOCK(slot, k) ((void)(slot))
#endif

constexpr int BR2X_SPIN = 1 << 24;

__device__ __forceinline__ void st_sc1(double *p, double v) {
  __hip_atomic_store(reinterpret_cast<uint64_t *>(p), __builtin_bit_cast(uint64_t, v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1(const double *p) {
  return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const uint64_t *>(p), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT));
}

// The flag half of a hand-off, for thread 0 alone, between the caller's two workgroup barriers: of
// the `count` flags of the group at fl, publish `value` in flag `self` (a plain store when `plain`:
// br2y's same-XCD form; an sc1 store otherwise) and poll every other one until it reaches `value`.
// On expiry *stop is set and *err raised.
__device__ __forceinline__ void handoff_flags(uint32_t *fl, int count, int self, uint32_t value, bool plain, int *stop,
                                              int *err) {
  if (plain)
    __hip_atomic_store(fl + self, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    __hip_atomic_store(fl + self, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
  for (int i = 1; i < count && !*stop; ++i) {  // the partners in ring order from self: one poll loop
    const int p = self + i < count ? self + i : self + i - count;
    int n = 0;
    while (__hip_atomic_load(fl + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < value) {
      if (++n == BR2X_SPIN) {
        *stop = 1;
        atomicExch(err, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
}

// ---- slots and flags: doubles / words per message, and each kernel's slot address --------------
// br2x: xg[m][r][slot][N2]; flags[m][r]
constexpr size_t BR2X_SLOT_DOUBLES = 2 * 2 * (size_t)N2, BR2X_FLAGS = 2;
__device__ __forceinline__ double *br2x_slot(double *xg, int m, int r, size_t slot) {
  return xg + (((size_t)m * 2 + r) * 2 + slot) * N2;
}
// br2y: xg[m][r][slot][g][re / im][1024]; flags[m][r], then (after every message's) the workers'
// XCD ids + 1, [m][r] too
constexpr size_t BR2Y_SLOT_DOUBLES = 2 * 2 * 2 * 2 * (size_t)(N2 / 2), BR2Y_FLAGS = 4;
__device__ __forceinline__ double *br2y_slot(double *xg, int m, int r, size_t slot, int g) {
  return xg + ((((size_t)m * 2 + r) * 2 + slot) * 2 + g) * 2 * (N2 / 2);
}
// the host allocates one pair of buffers for whichever of the two runs
static_assert(BR2Y_SLOT_DOUBLES >= BR2X_SLOT_DOUBLES && BR2Y_FLAGS >= BR2X_FLAGS, "br2y's scratch is the larger");
constexpr size_t BR2XY_SLOT_DOUBLES = BR2Y_SLOT_DOUBLES, BR2XY_FLAGS = BR2Y_FLAGS;

// trace_x: xg[m][w][slot][A / B][N2]; flags[m][w]
#ifndef OMR_TRACE_X
#define OMR_TRACE_X 5
#endif
constexpr int TRACE_X = OMR_TRACE_X;  // workgroups per message (25 digits: 5 per workgroup)
constexpr size_t TRACE_X_SLOT_DOUBLES = (size_t)TRACE_X * 2 * 2 * N2, TRACE_X_FLAGS = TRACE_X;
__device__ __forceinline__ double *trace_x_slot(double *xg, int m, int w, size_t slot) {
  return xg + (((size_t)m * TRACE_X + w) * 2 + slot) * 2 * N2;
}

}  // namespace omr
