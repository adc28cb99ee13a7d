// The LDS synchronisation vocabulary of every kernel (gfx950): the s_waitcnt immediate, and the
// wave-level and workgroup-level points at which LDS traffic becomes visible.
#pragma once

#include "common.hpp"

namespace omr {

// gfx9 s_waitcnt immediate: vmcnt in bits 3:0 and 15:14, expcnt in bits 6:4, lgkmcnt in bits 11:8.
// A counter at its maximum is not waited for.
constexpr int WAIT_VM_MAX = 63, WAIT_EXP_MAX = 7, WAIT_LGKM_MAX = 15;
constexpr int waitcnt_imm(int vmcnt, int expcnt, int lgkmcnt) {
  return (vmcnt & 0xF) | ((vmcnt >> 4) << 14) | (expcnt << 4) | (lgkmcnt << 8);
}
constexpr int waitcnt_lgkm(int n) { return waitcnt_imm(WAIT_VM_MAX, WAIT_EXP_MAX, n); }
constexpr int waitcnt_vm(int n) { return waitcnt_imm(n, WAIT_EXP_MAX, WAIT_LGKM_MAX); }
static_assert(waitcnt_lgkm(0) == 0xc07f, "s_waitcnt lgkmcnt(0)");
static_assert(waitcnt_vm(0) == 0x0f70 && waitcnt_vm(4) == 0x0f74, "s_waitcnt vmcnt(n)");

// LDS visibility within one wave: this wave's LDS writes have landed, and the compiler moves no
// memory operation across (waves of a workgroup stay independent).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_s_waitcnt(waitcnt_lgkm(0));
  __builtin_amdgcn_wave_barrier();
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}
// Compiler-only ordering of one wave's LDS accesses (its LDS operations complete in order).
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_wave_barrier();
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}
// Workgroup barrier for LDS traffic only: this wave's LDS reads / writes are done, then s_barrier.
// Unlike __syncthreads() (a workgroup-scope fence: s_waitcnt vmcnt(0) lgkmcnt(0)) it leaves the
// wave's global loads in flight across the barrier (cdna_hip_programming.md, "Pipelining across
// barriers"); callers that hand global data between waves must not use it.
__device__ __forceinline__ void wg_barrier_lds() {
  __builtin_amdgcn_s_waitcnt(waitcnt_lgkm(0));
  __builtin_amdgcn_s_barrier();
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

}  // namespace omr
