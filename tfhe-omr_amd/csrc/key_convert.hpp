// Key conversion and bound kernels of context creation (context.hip launches them): the uploaded
// coefficient-domain keys -> the forms the rotation, key-switch and trace kernels read, and kappa_r
// of the stored spectra. The double-double spectra are key_spectra.hpp.
#pragma once

#include "device_fft.hpp"
#include "kernels.hpp"

namespace omr {

// ---- key conversion: coefficient-domain canonical residues -> NTT-domain centred residues ----
template <int LEVEL, typename IN, typename OUT>
__global__ void key_to_ntt_kernel(const IN *in, OUT *out, size_t npoly, double scale,
                                  const double *tw) {
  using M = Mod<LEVEL>;
  constexpr int T = LEVEL == 1 ? BR1_T : BR2_T, E = LEVEL == 1 ? BR1_E : BR2_E;
  using NTT = WgNtt<M, T, E>;
  __shared__ double lds[NTT::LDS_DOUBLES];
  const size_t poly = blockIdx.x;
  const int tid = threadIdx.x;
  if (poly >= npoly) return;
  const IN *src = in + poly * M::N;
  double x[E];
#pragma unroll
  for (int e = 0; e < E; ++e) x[e] = from_u64<M>((uint64_t)src[tid + e * T]);
  NTT::fwd(x, lds, tw, tid);
  OUT *dst = out + poly * M::N + tid * E;
#pragma unroll
  for (int e = 0; e < E; ++e)
    dst[e] = (OUT)(scale == 1.0 ? canon<M>(x[e]) : canon<M>(mm<M>(canon<M>(x[e]), scale)));
}

// KSK u32 [1024][27][671] -> int8 limbs [1024][4][672][32] (packed 4 per u32 word, byte b of word
// w = digit 4 w + b), zero for digits >= 27 and column 671.
__global__ void ksk_to_i8_kernel(const uint32_t *__restrict__ ksk, uint32_t *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= KSKB_WORDS) return;
  const int w = (int)(t & 7);
  const size_t rest = t >> 3;
  const int col = (int)(rest % KSM_COLS);
  const size_t il = rest / KSM_COLS;
  const int limb = (int)(il & 3), i = (int)(il >> 2);
  uint32_t word = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int j = 4 * w + b;
    uint32_t v = 0;
    if (j < KS_DIGITS && col <= NI) v = (ksk[((size_t)i * KS_DIGITS + j) * (NI + 1) + col] >> (7 * limb)) & 127u;
    word |= v << (8 * b);
  }
  out[t] = word;
}

// BSK1 rows [512][8 r][2 o][lane * 8 + e] -> the latency layout [512][8 e][8 r][2 o][64 lane]
__global__ __launch_bounds__(256) void bsk1_latency_layout_kernel(const double2 *__restrict__ in,
                                                                  double2 *__restrict__ out, size_t n) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int lane = (int)(idx & 63), o = (int)((idx >> 6) & 1), r = (int)((idx >> 7) & 7), e = (int)((idx >> 10) & 7);
  const size_t i = idx >> 13;
  out[idx] = in[((i * 8 + r) * 2 + o) * 512 + key1_pos(lane, e)];
}

// Largest |K^| of each stored key-spectrum row (len complex values; one workgroup per row):
// kappa_r of the a priori bound, rounded up past sqrt's error.
__global__ __launch_bounds__(256) void row_max_abs_kernel(const double2 *__restrict__ x, int len,
                                                          double *__restrict__ out) {
  __shared__ double wm[4];
  const double2 *row = x + (size_t)blockIdx.x * len;
  double m = 0.0;
  for (int i = threadIdx.x; i < len; i += 256) {
    const double2 v = row[i];
    m = fmax(m, sqrt(v.x * v.x + v.y * v.y) * (1.0 + 0x1p-50));
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
}

}  // namespace omr

// The two kernels that came out of context.hip keep the names they had there, outside namespace omr
// (the listings and profiles of earlier rounds name them); context.hip alone includes this header.
namespace {
using namespace omr;

// ---- BSK2 rows -> the CmuxNtt forward order, x scale (the blind rotation's key layout) ----
__global__ __launch_bounds__(256) static void key_to_cmux_kernel(const uint64_t *in, double *out, size_t npoly,
                                                        double scale, const double *tw2c) {
  using M = Mod<2>;
  using NTT = CmuxNtt;
  __shared__ double lds[NTT::LDS_DOUBLES];
  __shared__ double tws[NTT::N];
  const size_t poly = blockIdx.x;
  const int tid = threadIdx.x;
  if (poly >= npoly) return;
  const uint64_t *src = in + poly * NTT::N;
  double x[NTT::E];
#pragma unroll
  for (int e = 0; e < NTT::E; ++e) {
    x[e] = from_u64<M>(src[tid + e * NTT::T]);
    tws[tid + e * NTT::T] = tw2c[tid + e * NTT::T];
  }
  __syncthreads();
  NTT::fwd<0>(x, lds, tws, tid);
  double *dst = out + poly * NTT::N + tid * NTT::E;
#pragma unroll
  for (int e = 0; e < NTT::E; ++e) dst[e] = canon<M>(mm<M>(canon<M>(x[e]), scale));
}
}  // namespace

// Scale the even (alpha) rows of the trace key by N^-1 in place.
__global__ void scale_even_rows_kernel(double *rows, size_t npoly, double s) {
  using M = Mod<2>;
  const size_t poly = (size_t)blockIdx.x * 2;
  if (poly >= npoly) return;
  double *p = rows + poly * N2;
  for (int j = threadIdx.x; j < N2; j += blockDim.x) p[j] = canon<M>(mm<M>(p[j], s));
}

