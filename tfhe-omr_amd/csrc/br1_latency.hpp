// Latency path of the detect pipeline (small chunks: a single message or a few), level 1.
//
// The throughput kernels give one wave to a level-1 rotation and one 4-wave workgroup to a
// level-2 message, so a lone message walks 512 (670) CMUX steps with 10 (14) transforms each on
// one wave (workgroup) while the rest of the chip idles: 9 + 16.6 ms of its 27 ms latency.
// The latency kernels split every CMUX step's digit transforms over more waves, whose partial
// multiply-accumulates are summed through LDS before the inverse transforms:
//   level 1 (br1l_kernel, here): one 8-wave workgroup per rotation; wave w transforms one of the 8
//     digit polynomials (1 FFT instead of 8) and adds its products into the two output sums in
//     LDS, waves 0 / 1 run the inverse FFT of output A / B and own the mask / body accumulator;
//   level 2 (br2_ntt.hpp: br2l_kernel, br2x_kernel, trace_x_kernel; br2_fft.hpp: br2y_kernel): one
//     8-wave workgroup, or two on two CUs, per message;
//   key switch (ks_mfma.hpp: ks_mfma_split_kernel + ks_combine_kernel): the 1024 input
//     coefficients split over 32 slices of workgroups.
// The arithmetic is the throughput kernels' (same digits, transforms, products and reduction
// points), so the outputs are bit-identical; tests/test_gpu_parity.py checks both paths.
#pragma once

#include "device_fft.hpp"
#include "handoff.hpp"
#include "level1_common.hpp"

namespace omr {

// Level 1 over eight waves, one workgroup per rotation. Per CMUX step wave w = p * D1 + k extracts
// digit k of polynomial p (p = 0 mask, 1 body: 16 coefficients per lane) and runs its forward FFT
// (GGSW row w's digit spectrum); the eight spectra then cross through LDS (each wave's exchange
// buffer, [e][lane]) and wave v multiplies the 8 spectra's register-slot-v points by the 8 rows'
// keys (its slice of the step, the bsk1l layout: 16 KB contiguous per wave and step), producing
// outputs A and B at those points with plain stores; waves 0 / 1 read output A / B, run its
// inverse and own the mask / body accumulator. Three LDS-only barriers per step (the key loads of
// the next executed step, issued after the multiply-accumulate, stay in flight across them).
// Round 2's form summed the eight waves' products with ds_add_f64 atomics into shared sums: their
// completion tail was ~3,600 cycles of a 17,100-cycle step (tools/phase_trace.py,
// profiles/r03q/phase_br1l_atomics.log); the products now sum in registers in a fixed row order,
// as in br1f_kernel, and the rounded FFT product is exact in either order (device_fft.hpp).
constexpr int BR1L_WAVES = 2 * D1;

// FROM: the initial accumulator is acc0's rotation instead (br1f_body's FROM).
template <bool G, bool FROM = false>
__device__ __forceinline__ void br1l_body(
    const uint16_t *__restrict__ clue_a, const uint16_t *__restrict__ clue_b,
    const uint16_t *__restrict__ lwe_a, const uint16_t *__restrict__ lwe_b,
    const double2 *__restrict__ bskl, DeviceTables tb, uint32_t *__restrict__ ext_out,
    uint64_t *__restrict__ rlwe_out, int mode, unsigned long long *margin,
    const uint64_t *__restrict__ acc0 = nullptr) {
  using F = Fft512;
  constexpr int NF = F::N, W = BR1L_WAVES;
  static_assert(W == 8 && NF == 8 * 64, "one wave per GGSW row and per register slot");
  // [ACC, -ACC] per poly (0 mask, 1 body), Lvl1Off form; 8 KB-aligned for the v_and_or addresses
  __shared__ __attribute__((aligned(8192))) uint32_t ext[2][2 * N1];
  __shared__ double2 xch_all[W][F::BUF];      // per wave: its transform's exchange, then its spectrum [e][lane]
  __shared__ double2 outs[2][8 * 64];         // outputs A, B: [e][lane]
  __shared__ double2 tws[NF];
  __shared__ uint16_t la[N0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = wave / D1, k = wave % D1;
  double2 *xch = xch_all[wave];
  const size_t g = blockIdx.x;  // rotation
  const int b = lvl1_stage_lwe(clue_a, clue_b, lwe_a, lwe_b, g, la, threadIdx.x, 64 * W);
  // ACC = (0, X^{-b} * LUT1): wave 0 owns the mask accumulator, wave 1 the body accumulator
  // (the accumulator in br1f's Lvl1Off form: ac'' = ac + H/2 in [0, Q), the stored negacyclic half
  // H - ac'' doubling as the digit operand; level1_common.hpp, tests/test_lvl1_offset_model.py)
  uint32_t ac[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if constexpr (FROM)
      ac[i] = Lvl1Off::enc(wave < 2 ? lvl1_acc_from(acc0, g, wave, acc_coef(lane, i)) : 0);
    else
      ac[i] = Lvl1Off::enc(wave == 1 ? (int)lvl1_acc_init(tb, b, acc_coef(lane, i)) : 0);
  }
  if (wave < 2) lvl1_stage_ext(ext[wave], ac, lane);
  for (int j = threadIdx.x; j < NF; j += 64 * W) tws[j] = tb.fft1[j];
  __syncthreads();
  // Wave v's key slice of an executed step: rows 0..7, outputs A / B at register slot v of every
  // lane (16 KB contiguous per wave), loaded two executed steps ahead (below).
  auto next_step = [&](int i) {  // first i' >= i with a_i' != 0 (uniform)
    while (i < N0 && la[i] == 0) ++i;
    return i;
  };
  double2 kk0[8][2], kk1[8][2];  // [row][output A/B] of two consecutive executed steps
  auto load_slice = [&](double2 (&kk)[8][2], int i) {
    if (i >= N0) return;
    const double2 *kr = bskl + ((size_t)i * 8 + wave) * 16 * 64 + lane;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int o = 0; o < 2; ++o) kk[r][o] = kr[(r * 2 + o) * 64];
  };
  const int pslot = __builtin_amdgcn_readfirstlane(blockIdx.x == 0 ? wave : -1);
  int hs = 0;
  RoundGuard<G> rg;  // waves 0 / 1 round the inverses
  // one CMUX step at executed step i with its key slice kk (kko: the other slice buffer; inext,
  // inext2: the next two executed steps)
  auto cmux = [&](int i, double2 (&kk)[8][2], double2 (&kko)[8][2], int inext, int inext2) {
    const int a = __builtin_amdgcn_readfirstlane(la[i]);  // != 0: (X^0 - 1) * ACC = 0 is skipped
    OMR_PHASE(pslot, hs, 0);
    double xr[1][8], xi[1][8];
    const Lvl1RotRead rot(ext[p], lane, a);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint32_t w = Lvl1Off::digits_u(rot(q), ext[p][N1 + acc_coef(lane, q)]);
      const double d = Lvl1Off::digit_shifts_u(w, k);
      if (q < 8)
        xr[0][q] = d;
      else
        xi[0][q - 8] = d;
    }
    OMR_PHASE(pslot, hs, 1);
    F::fwd<1, false>(xr, xi, xch, tws, lane);  // pass-0 twiddles from LDS (the lambda loses the
                                               // global table's restrict: vector loads every step)
    wave_lds_fence();  // the spectrum's writes stay below the transform's exchange reads
#pragma unroll
    for (int e = 0; e < 8; ++e) xch[e * 64 + lane] = make_double2(xr[0][e], xi[0][e]);
    OMR_PHASE(pslot, hs, 2);
    // waves 0 / 1 (the inverses' critical path) load the next step's slice here, in the time they
    // wait for waves 4..7, which share their SIMDs and finish their transforms ~2,500 cycles later
    if (wave < 2) load_slice(kko, inext);
    wg_barrier_lds();  // every spectrum is in LDS
    OMR_PHASE(pslot, hs, 3);
    {  // outputs A, B at register slot `wave` of every lane: rows in order, as br1f_step_lds
      double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const double2 x = xch_all[r][wave * 64 + lane];
        lvl1_mac(x.x, x.y, kk[r][0], kk[r][1], ar, ai, br, bi);
      }
      outs[0][wave * 64 + lane] = make_double2(ar, ai);
      outs[1][wave * 64 + lane] = make_double2(br, bi);
    }
    wg_barrier_lds();  // outputs complete; every spectrum read (the exchange buffers are free)
    OMR_PHASE(pslot, hs, 4);
    // waves 2..7: the slice two executed steps ahead, into the registers just consumed, issued
    // while waves 0 / 1 run the inverses (issuing 16 KB per wave before the barrier above held
    // every wave there ~2,300 cycles)
    if (wave >= 2) load_slice(kk, inext2);
    if (wave < 2) {  // wave 0: output A (mask accumulator), wave 1: output B (body accumulator)
      double sr[1][8], si[1][8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double2 v = outs[wave][e * 64 + lane];
        sr[0][e] = v.x;
        si[0][e] = v.y;
      }
      OMR_PHASE(pslot, hs, 5);
      F::inv<1, false>(sr, si, xch, tws, lane);
      OMR_PHASE(pslot, hs, 6);
#pragma unroll
      for (int q = 0; q < 16; ++q)
        ac[q] = Lvl1Off::add(ac[q], Lvl1Off::round<G>(q < 8 ? sr[0][q] : si[0][q - 8], &rg));  // exact (< 2^43)
      lvl1_stage_ext(ext[wave], ac, lane);
    }
    wg_barrier_lds();  // ACC staged for the next step's digits
    OMR_PHASE(pslot, hs, 7);
    ++hs;
  };
  // key slices alternate between kk0 and kk1: waves 2..7 load each two executed steps ahead,
  // waves 0 / 1 one step ahead (before the first barrier of the step in between)
  int i0 = next_step(0), i1 = next_step(i0 + 1);
  load_slice(kk0, i0);
  if (wave >= 2) load_slice(kk1, i1);
  OMR_PHASE_CLOCK(pslot, 0);
#pragma unroll 1
  while (i0 < N0) {
    const int i2 = __builtin_amdgcn_readfirstlane(next_step(i1 + 1));
    cmux(i0, kk0, kk1, i1, i2);
    if (i1 >= N0) break;
    const int i3 = __builtin_amdgcn_readfirstlane(next_step(i2 + 1));
    cmux(i1, kk1, kk0, i2, i3);
    i0 = i2;
    i1 = i3;
  }
  OMR_PHASE_CLOCK(pslot, 1);
  rg.publish(margin);
  if (mode == 0) {  // extract_lwe_locally (coefficient 0), detector.rs:561
    uint32_t *o = ext_out + g * (N1 + 1);
    for (int j = threadIdx.x; j < N1; j += 64 * W)
      o[j] = Lvl1Int::to_u32(j == 0 ? Lvl1Off::dec(ext[0][0]) : -Lvl1Off::dec(ext[0][N1 - j]));
    if (threadIdx.x == 0) o[N1] = Lvl1Int::to_u32(Lvl1Off::dec(ext[1][0]));
  } else {
    uint64_t *o = rlwe_out + g * 2 * N1;
    for (int j = threadIdx.x; j < N1; j += 64 * W) {
      o[j] = Lvl1Int::to_u32(Lvl1Off::dec(ext[0][j]));
      o[N1 + j] = Lvl1Int::to_u32(Lvl1Off::dec(ext[1][j]));
    }
  }
}

__global__ __launch_bounds__(64 * BR1L_WAVES, 1) void br1l_kernel(
    const uint16_t *__restrict__ clue_a, const uint16_t *__restrict__ clue_b,
    const uint16_t *__restrict__ lwe_a, const uint16_t *__restrict__ lwe_b,
    const double2 *__restrict__ bskl, DeviceTables tb, uint32_t *__restrict__ ext_out,
    uint64_t *__restrict__ rlwe_out, int mode) {
  br1l_body<false>(clue_a, clue_b, lwe_a, lwe_b, bskl, tb, ext_out, rlwe_out, mode, nullptr);
}
__global__ __launch_bounds__(64 * BR1L_WAVES, 1) void br1l_guard_kernel(
    const uint16_t *__restrict__ clue_a, const uint16_t *__restrict__ clue_b,
    const uint16_t *__restrict__ lwe_a, const uint16_t *__restrict__ lwe_b,
    const double2 *__restrict__ bskl, DeviceTables tb, uint32_t *__restrict__ ext_out,
    uint64_t *__restrict__ rlwe_out, int mode, unsigned long long *margin) {
  br1l_body<true>(clue_a, clue_b, lwe_a, lwe_b, bskl, tb, ext_out, rlwe_out, mode, margin);
}
__global__ __launch_bounds__(64 * BR1L_WAVES, 1) void br1l_from_kernel(
    const uint16_t *__restrict__ clue_a, const uint16_t *__restrict__ clue_b,
    const uint16_t *__restrict__ lwe_a, const uint16_t *__restrict__ lwe_b,
    const double2 *__restrict__ bskl, DeviceTables tb, uint32_t *__restrict__ ext_out,
    uint64_t *__restrict__ rlwe_out, int mode, const uint64_t *__restrict__ acc0) {
  br1l_body<false, true>(clue_a, clue_b, lwe_a, lwe_b, bskl, tb, ext_out, rlwe_out, mode, nullptr, acc0);
}
__global__ __launch_bounds__(64 * BR1L_WAVES, 1) void br1l_guard_from_kernel(
    const uint16_t *__restrict__ clue_a, const uint16_t *__restrict__ clue_b,
    const uint16_t *__restrict__ lwe_a, const uint16_t *__restrict__ lwe_b,
    const double2 *__restrict__ bskl, DeviceTables tb, uint32_t *__restrict__ ext_out,
    uint64_t *__restrict__ rlwe_out, int mode, unsigned long long *margin, const uint64_t *__restrict__ acc0) {
  br1l_body<true, true>(clue_a, clue_b, lwe_a, lwe_b, bskl, tb, ext_out, rlwe_out, mode, margin, acc0);
}

}  // namespace omr
