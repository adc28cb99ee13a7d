// Level-1 blind rotation on the exact modular NTT (round 5): BlindRotationKey::blind_rotate with
// concrete-ntt's arithmetic, as the reference runs it (detector.rs:553-557; omr_core/Cargo.toml:38-45).
// Two uses:
//  - the exact fallback of a guarded level-1 launch (detect.hip, launch_br1): run after the guarded
//    FFT kernel, every workgroup reads that launch's rounding-margin word and leaves unless it
//    reached the certificate threshold 1 - E1, in which case the launch's rotations are recomputed
//    here and overwrite the FFT outputs -- so a key whose a priori bound does not prove the FFT exact
//    still gets exact outputs, as level 2's breaches do (br2l_fallback_kernel);
//  - omr_ctx_set_exact_level1: every level-1 launch on this kernel, a full-size cross-check of the
//    FFT kernels (both families share the level-1 FFT) against an independent exact arithmetic.
// One 64-thread workgroup (one wave) per rotation: WgNtt<Mod<1>, 64, 16> is wave-private (its
// exchanges need no workgroup barrier), residues are exact integers in FP64 registers
// (device_ntt.hpp), the key rows are read from L2 in the NTT domain x N1^-1 (context.hip, ensure_bsk1n:
// [512][2 D1 rows][2 outputs][1024] centred doubles, NTT index order). Per CMUX step: the digits of
// (X^a - 1) * ACC for both polynomials (the same decomposition as br1f: Lvl1Int::digits), 8 forward
// transforms each multiplied into the two output accumulators, 2 inverse transforms, ACC += out.
// Not tuned: a fallback that never runs on a real key, and a test instrument.
#pragma once

#include "kernels.hpp"
#include "level1_common.hpp"

namespace omr {

using Ntt1W = WgNtt<Mod<1>, 64, 16>;
static_assert(Ntt1W::N == N1 && Ntt1W::LDS_DOUBLES * sizeof(double) >= 2 * N1 * sizeof(int),
              "the exchange buffer also stages [ACC, -ACC]");

// Rotation g: clue g % 7 of message g / 7 (lwe_a == nullptr) or LWE g; the outputs as br1f_body's
// (mode 0: the extracted LWE, mode 1: the full RLWE).
// acc0 (nullptr in the production kernels): the initial accumulator is acc0's rotation instead (br1f_body's
// FROM; a pointer tested at run time for br2l_body's reason, br2_ntt.hpp).
__device__ __forceinline__ void br1n_body(const uint16_t *__restrict__ clue_a, const uint16_t *__restrict__ clue_b,
                                          const uint16_t *__restrict__ lwe_a, const uint16_t *__restrict__ lwe_b,
                                          const double *__restrict__ bsk1n, const DeviceTables &tb,
                                          uint32_t *__restrict__ ext, uint64_t *__restrict__ rlwe_out, int mode,
                                          size_t g, const uint64_t *acc0 = nullptr) {
  using M = Mod<1>;
  __shared__ double lds[Ntt1W::LDS_DOUBLES];  // the transforms' exchanges; [ACC, -ACC] between them
  __shared__ uint16_t la[N0];
  const int lane = threadIdx.x;
  const int b = lvl1_stage_lwe(clue_a, clue_b, lwe_a, lwe_b, g, la, lane, 64);
  // ACC = (0, X^{-b} * LUT1); ac[p][e] = coefficient lane + 64 e, canonical centred
  double ac[2][16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (acc0) {
      ac[0][e] = (double)lvl1_acc_from(acc0, g, 0, lane + 64 * e);
      ac[1][e] = (double)lvl1_acc_from(acc0, g, 1, lane + 64 * e);
    } else {
      ac[0][e] = 0.0;
      ac[1][e] = lvl1_acc_init(tb, b, lane + 64 * e);
    }
  }
  __syncthreads();
  int *st = reinterpret_cast<int *>(lds);
#pragma unroll 1
  for (int i = 0; i < N0; ++i) {
    const int a = __builtin_amdgcn_readfirstlane(la[i]);
    uint32_t w[2][16];  // digit words of canon(X^a ACC_p - ACC_p), coefficient lane + 64 e
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        st[lane + 64 * e] = (int)ac[p][e];
        st[N1 + lane + 64 * e] = -(int)ac[p][e];
      }
      wave_lds_sync();
#pragma unroll
      for (int e = 0; e < 16; ++e) {  // (X^a ACC)[j] = [ACC, -ACC][(j - a) mod 2N]
        const int x = st[(lane + 64 * e - a) & (2 * N1 - 1)];
        w[p][e] = Lvl1Int::digits(Lvl1Int::canon(x - (int)ac[p][e]));
      }
      wave_lds_sync();  // the reads are done before the buffer is written again
    }
    double o[2][16];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll 1
      for (int k = 0; k < D1; ++k) {  // GGSW row p D1 + k: digit k of polynomial p
        double x[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = lvl1_digit(w[p][e], k);
        Ntt1W::fwd(x, lds, tb.tw1, lane);
        const double *kr = bsk1n + ((size_t)i * 2 * D1 + p * D1 + k) * 2 * N1 + lane * 16;
#pragma unroll
        for (int out = 0; out < 2; ++out)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const double v = mm<M>(x[e], kr[out * N1 + e]);
            o[out][e] = p == 0 && k == 0 ? v : o[out][e] + v;
          }
      }
#pragma unroll
    for (int out = 0; out < 2; ++out) {
#pragma unroll
      for (int e = 0; e < 16; ++e) o[out][e] = canon<M>(o[out][e]);
      Ntt1W::inv(o[out], lds, tb.itw1, lane);
#pragma unroll
      for (int e = 0; e < 16; ++e) ac[out][e] = canon<M>(ac[out][e] + o[out][e]);
    }
  }
  lvl1_store_wave([&](int p, int e) { return (int)ac[p][e]; }, st, g, mode, ext, rlwe_out, lane);
}

__global__ __launch_bounds__(64) void br1n_kernel(const uint16_t *__restrict__ clue_a,
                                                  const uint16_t *__restrict__ clue_b,
                                                  const uint16_t *__restrict__ lwe_a,
                                                  const uint16_t *__restrict__ lwe_b,
                                                  const double *__restrict__ bsk1n, DeviceTables tb,
                                                  uint32_t *__restrict__ ext, uint64_t *__restrict__ rlwe_out,
                                                  int mode, size_t nrot) {
  if (blockIdx.x >= nrot) return;
  br1n_body(clue_a, clue_b, lwe_a, lwe_b, bsk1n, tb, ext, rlwe_out, mode, blockIdx.x);
}
// The exact fallback of a guarded level-1 launch: runs only when that launch's margin word reached thr.
__global__ __launch_bounds__(64) void br1n_fallback_kernel(const uint16_t *__restrict__ clue_a,
                                                           const uint16_t *__restrict__ clue_b,
                                                           const uint16_t *__restrict__ lwe_a,
                                                           const uint16_t *__restrict__ lwe_b,
                                                           const double *__restrict__ bsk1n, DeviceTables tb,
                                                           uint32_t *__restrict__ ext,
                                                           uint64_t *__restrict__ rlwe_out, int mode, size_t nrot,
                                                           const unsigned long long *lmargin, double thr) {
  if (blockIdx.x >= nrot || !margin_breached(lmargin, thr)) return;
  br1n_body(clue_a, clue_b, lwe_a, lwe_b, bsk1n, tb, ext, rlwe_out, mode, blockIdx.x);
}
// Both of the above from acc0, as one kernel (lmargin == nullptr: unconditional).
__global__ __launch_bounds__(64) void br1n_from_kernel(
    const uint16_t *__restrict__ clue_a, const uint16_t *__restrict__ clue_b, const uint16_t *__restrict__ lwe_a,
    const uint16_t *__restrict__ lwe_b, const double *__restrict__ bsk1n, DeviceTables tb,
    uint32_t *__restrict__ ext, uint64_t *__restrict__ rlwe_out, int mode, size_t nrot,
    const unsigned long long *lmargin, double thr, const uint64_t *__restrict__ acc0) {
  if (blockIdx.x >= nrot || (lmargin && !margin_breached(lmargin, thr))) return;
  br1n_body(clue_a, clue_b, lwe_a, lwe_b, bsk1n, tb, ext, rlwe_out, mode, blockIdx.x, acc0);
}

}  // namespace omr
