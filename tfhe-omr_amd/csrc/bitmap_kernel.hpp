// Bitmap digest kernel (include/omr_gpu.h, "Bitmap digest"; none in the reference): message g of a board
// goes to ciphertext g / 16384, bit plane t = (g % 16384) / 2048 and coefficient j = g % 2048, so that
//   out[c][h][i] = sum_g pv_g[h][i] * 2^t * NTT(X^j)[i]  (mod q2),  NTT(X^j)[i] = psi^((2 brv11(i) + 1) j mod 4096).
// No transform runs: the monomial's NTT is a table look-up. psi^e = tw2[brv11(e)] for e < 2048 (tw2[k] =
// psi^brv11(k), the table every level-2 NTT uses) and psi^(e + 2048) = -psi^e. Each workgroup copies
// those 2,048 powers to LDS once (16 KiB) and steps each point's exponent by its odd constant per
// message; the other option, a running power per point, costs a third modular product per point and
// message and carries a dependency from message to message.
//
// Decomposition. A slice is 128 aligned consecutive messages: it never crosses a bit plane, so its
// messages share the factor 2^t, which is applied once to the slice's sum. A workgroup folds `spw`
// consecutive touched slices of one touched ciphertext for one quarter of the 2,048 evaluation
// points and writes one canonical partial; reduce_partials_kernel / accumulate_partials_kernel
// (encode_kernels.hpp) sum the partials. Thread `tid` owns the adjacent points i0 = 512 z + 2 tid and
// i0 + 1: one 16-byte load per message and half, and brv11(i0 + 1) = brv11(i0) + 1024, so the second
// point's power is the first's times psi^(2048 j) = (-1)^j: one look-up serves both.
#pragma once

#include "kernels.hpp"

// Variant builds (tools/build_variant.sh), both exact, measured in DESIGN.md §1: the slice length, and
// the running power per point instead of the stepped exponent and the LDS look-up per message.
#ifndef OMR_BMP_SLICE
#define OMR_BMP_SLICE 128
#endif
#ifndef OMR_BMP_RUNNING_POWER
#define OMR_BMP_RUNNING_POWER 0
#endif

namespace omr {

constexpr int BMP_T = 256;                // threads
constexpr int BMP_SPLIT = 4;              // workgroups per 2,048 evaluation points (2 points per thread)
constexpr int BMP_SLICE = OMR_BMP_SLICE;  // messages per slice, divides 2,048
constexpr int BMP_RUN = 8;                // products added between two reductions
constexpr uint64_t BMP_PER_CT = OMR_BITMAP_MESSAGES_PER_CT;
static_assert(BMP_T * 2 * BMP_SPLIT == N2 && N2 % BMP_SLICE == 0 && BMP_PER_CT == (uint64_t)OMR_BITMAP_BITS * N2,
              "bitmap geometry");

__device__ __forceinline__ uint64_t bmp_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t bmp_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// psi^e, e < 4096, from the workgroup's table of the first 2,048 powers
__device__ __forceinline__ double bmp_psi_pow(const double *pw, uint32_t e) {
  const double t = pw[e & 2047u];
  return (e & 2048u) ? -t : t;
}

// grid (chunks, touched ciphertexts, BMP_SPLIT); pv [D][2][N2] canonical u64, 16-byte aligned, message m
// has global index offset + m; first_ct = offset / 16384; partial [touched][chunks][2][N2] canonical u64.
// Chunk k of a touched ciphertext covers its touched slices [k spw, (k + 1) spw); a chunk beyond them
// writes zeros.
__global__ __launch_bounds__(BMP_T) void encode_bitmap_kernel(const uint64_t *__restrict__ pv, uint64_t D,
                                                              uint64_t offset, uint64_t first_ct, int spw,
                                                              const double *__restrict__ tw,
                                                              uint64_t *__restrict__ partial) {
  using M = Mod<2>;
  __shared__ double pw[N2];  // psi^e, e < 2048
  const int tid = threadIdx.x;
  for (int e = tid; e < N2; e += BMP_T) pw[e] = tw[__brev((uint32_t)e) >> 21];
  __syncthreads();
  const int i0 = (int)blockIdx.z * (N2 / BMP_SPLIT) + 2 * tid;
  const uint32_t k0 = 2 * (__brev((uint32_t)i0) >> 21) + 1;  // point i0 is psi^k0; point i0 + 1 is psi^(k0 + 2048)
  const uint64_t ct = first_ct + blockIdx.y;
  const uint64_t lo = bmp_max(offset, ct * BMP_PER_CT), hi = bmp_min(offset + D, (ct + 1) * BMP_PER_CT);  // lo < hi
  const uint64_t s_hi = (hi - 1) / BMP_SLICE + 1;
  uint64_t s = lo / BMP_SLICE + (uint64_t)blockIdx.x * spw;
  const uint64_t s_end = bmp_min(s_hi, s + (uint64_t)spw);
  double tot[4] = {0.0, 0.0, 0.0, 0.0};  // a[i0], a[i0 + 1], b[i0], b[i0 + 1]
#if OMR_BMP_RUNNING_POWER
  const double step = bmp_psi_pow(pw, k0);
#endif
#pragma unroll 1
  for (; s < s_end; ++s) {
    const uint64_t g0 = bmp_max(lo, s * BMP_SLICE), g1 = bmp_min(hi, (s + 1) * BMP_SLICE);
    const uint32_t l = (uint32_t)(g0 % BMP_PER_CT);
    uint32_t j = l % N2;
    uint32_t e = (k0 * j) & 4095u;
    const int n = (int)(g1 - g0);
    const uint64_t *p = pv + (g0 - offset) * 2 * N2 + i0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#if OMR_BMP_RUNNING_POWER
    double w = bmp_psi_pow(pw, e);  // |w| <= q/2 + 2 throughout: the bounds below keep their slack
#endif
    // Bounds: a product mm(x, w) of a centred x (|x| <= q/2) and |w| <= q/2 is at most 0.6 q in
    // magnitude (device_ntt.hpp), and an accumulator is at most q/2 + 2 after red. BMP_RUN = 8
    // products are added between reductions: 8 * 0.6 q + 0.5 q + 2 < 5.4 * 2^50 < 2^53, every sum exact.
#pragma unroll 1
    for (int mb = 0; mb < n; mb += BMP_RUN) {
      ulonglong2 va[BMP_RUN], vb[BMP_RUN];
#pragma unroll
      for (int r = 0; r < BMP_RUN; ++r) {  // the run's loads first: 256 bytes per thread in flight
        // the last message repeated past the end of the slice: loaded, never used
        const uint64_t *pm = p + (size_t)min(mb + r, n - 1) * 2 * N2;
        va[r] = *reinterpret_cast<const ulonglong2 *>(pm);
        vb[r] = *reinterpret_cast<const ulonglong2 *>(pm + N2);
      }
#pragma unroll
      for (int r = 0; r < BMP_RUN; ++r) {
        if (mb + r < n) {
#if OMR_BMP_RUNNING_POWER
          const double w0 = w;
          w = red<M>(mm<M>(w, step));
#else
          const double w0 = bmp_psi_pow(pw, e);
#endif
          const double w1 = (j & 1u) ? -w0 : w0;
          acc[0] += mm<M>(from_u64<M>(va[r].x), w0);
          acc[1] += mm<M>(from_u64<M>(va[r].y), w1);
          acc[2] += mm<M>(from_u64<M>(vb[r].x), w0);
          acc[3] += mm<M>(from_u64<M>(vb[r].y), w1);
          e = (e + k0) & 4095u;
          ++j;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = red<M>(acc[q]);
    }
    // the plane's factor: |acc| <= q/2 + 2 and 2^t <= 128, so the product is at most 0.6 q; with the
    // reduced total that is 1.1 q + 2, exact
    const double f = (double)(1u << (l / N2));
#pragma unroll
    for (int q = 0; q < 4; ++q) tot[q] = red<M>(tot[q] + mm<M>(acc[q], f));
  }
  uint64_t *o = partial + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2) * N2 + i0;
  ulonglong2 oa, ob;
  oa.x = to_u64<M>(canon<M>(tot[0]));
  oa.y = to_u64<M>(canon<M>(tot[1]));
  ob.x = to_u64<M>(canon<M>(tot[2]));
  ob.y = to_u64<M>(canon<M>(tot[3]));
  *reinterpret_cast<ulonglong2 *>(o) = oa;
  *reinterpret_cast<ulonglong2 *>(o + N2) = ob;
}

}  // namespace omr
