// Geometry, tables and the plain NTT kernel shared by the detect / encode path (gfx950). Each kernel of
// the path cites the reference function it replaces; the launch code is in detect.hip and encode.hip,
// the key conversion in key_convert.hpp (context.hip).
#pragma once

#include "device_ntt.hpp"

namespace omr {

// Workgroup geometry per level (T threads x E residues per thread = N) of the modular NTTs.
// Level 2 (latency blind rotations, trace, encode, key conversion): 256 threads x 8 residues.
// Both throughput blind rotations run on exact complex FFTs (br1_fft.hpp, br2_fft.hpp); level 1
// needs the NTT only for omr_ntt (tests).
constexpr int BR1_T = 256, BR1_E = 4;  // N1 = 1024
constexpr int BR2_T = 256, BR2_E = 8;  // N2 = 2048
constexpr int ENC_T = 128, ENC_E = 16;
constexpr size_t OMR_DEFAULT_BATCH = 16384;  // messages per detect chunk (scratch 36 KiB/msg)
constexpr size_t OMR_ENC_MAX_CHUNKS = 4096;   // default chunk partials per encode ciphertext
// key-switch geometry (ks_mfma.hpp; the KSK's conversion is in key_convert.hpp)
constexpr int KSM_COLS = 672;  // NI + 1 = 671 output columns, padded to 21 tiles of 32
constexpr int KSM_LIMBS = 4;
constexpr size_t KSKB_WORDS = (size_t)N1 * KSM_LIMBS * KSM_COLS * 8;  // 32 int8 per (i, l, col)
constexpr int KS_SPLIT = 32;  // slices of the 1024 input coefficients

struct DeviceTables {
  const double *tw1, *itw1, *tw2, *itw2;  // psi^brv(k), psi^-brv(k) (centred)
  const double *tw2c;                     // tw2 with stages 9, 10 permuted for CmuxNtt
  const double *lut1, *lut2;              // LUTs, coefficient domain (centred)
  const uint16_t *trace_perm;             // [11][2048] NTT-domain permutation of sigma_g
  const uint16_t *trace_src;              // [11][2048] coefficient source index of sigma_g (+N: negate)
  const double2 *fft1;                    // level-1 FFT twiddles
};

// (X^r * p)[j] for p in LDS, r in [0, 2N): sign-corrected read.
template <int N>
__device__ __forceinline__ double rot_read(const double *p, int j, int r) {
  int t = j - r;
  double s = 1.0;
  if (t < 0) {
    t += N;
    s = -1.0;
  }
  if (t < 0) {
    t += N;
    s = 1.0;
  }
  return s * p[t];
}

// ---- plain NTT of canonical u64 polynomials (tests / omr_ntt) ----
template <int LEVEL>
__global__ void ntt_u64_kernel(uint64_t *polys, size_t npoly, int inverse, double ninv,
                               const double *tw, const double *itw) {
  using M = Mod<LEVEL>;
  constexpr int T = LEVEL == 1 ? BR1_T : BR2_T, E = LEVEL == 1 ? BR1_E : BR2_E;
  using NTT = WgNtt<M, T, E>;
  __shared__ double lds[NTT::LDS_DOUBLES];
  const size_t poly = blockIdx.x;
  const int tid = threadIdx.x;
  if (poly >= npoly) return;
  uint64_t *p = polys + poly * M::N;
  double x[E];
  if (!inverse) {
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = from_u64<M>(p[tid + e * T]);
    NTT::fwd(x, lds, tw, tid);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) p[tid * E + e] = to_u64<M>(canon<M>(x[e]));
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = from_u64<M>(p[tid * E + e]);
    NTT::inv(x, lds, itw, tid);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) p[tid + e * T] = to_u64<M>(canon<M>(mm<M>(canon<M>(x[e]), ninv)));
  }
}

}  // namespace omr
