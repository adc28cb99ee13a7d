// Compact ciphertexts on the device (gfx950; include/omr_gpu.h, "Compact ciphertexts"): compact_kernel
// switches NttRlweCiphertexts from q2 to Q = 2^bits and writes them as bit streams, expand_kernel is its
// inverse. Included only by compact.hip, which launches both for the context, the digest session and
// the auditor. The per-value arithmetic and the stream layout are those of compact_math.hpp, the same
// functions the CPU statement's host test checks.
#pragma once

#include "compact_math.hpp"
#include "kernels.hpp"

namespace omr {

using CompactNtt = WgNtt<Mod<2>, BR2_T, BR2_E>;
// uint4 (four stream words) per polynomial: 16 bits, at most 512, so a thread stores at most two
constexpr int COMPACT_MAX_POLY_WORDS = 64 * COMPACT_MAX_BITS;
static_assert(COMPACT_N == N2 && COMPACT_Q2 == Q2, "compact_math.hpp restates the level-2 parameters");
static_assert(COMPACT_MAX_POLY_WORDS == N2, "a packed polynomial never needs more LDS words than it has values");

// 256 threads x 8 residues per polynomial, workgroup w takes ciphertexts w, w + grid, ...; a and b one
// after the other. Per polynomial: 64 contiguous bytes per thread as four 16-byte loads (thread tid owns
// NTT indices 8 tid + e, as CompactNtt::inv expects), issued one polynomial ahead so that they are in
// flight during the transform before; words reduced mod q2, the inverse NTT with ntt_u64_kernel's
// scaling to canonical coefficients (register e holds coefficient tid + 256 e), compact_rescale per
// coefficient, the 2,048 values through LDS (8 KiB), and the stream assembled as whole 32-bit words,
// four per thread and store: lane-consecutive 16-byte stores, 16 bits of them per polynomial. `magic` is
// compact_magic(bits), from the host. out must be 16-byte aligned (512 bits bytes per ciphertext keeps
// every ciphertext so).
//
// LDS reuse: CompactNtt::inv ends with a workgroup barrier after its last exchange reads, so its
// buffers are free for the next transform at once. `vals` is not in those buffers; a polynomial's
// values are written after that trailing barrier of its own transform, which every thread reaches only
// after it has assembled its words of the polynomial before, and read after the barrier below.
__global__ __launch_bounds__(BR2_T) void compact_kernel(const uint64_t *__restrict__ cts, size_t n, int bits,
                                                        uint32_t magic, const double *__restrict__ itw, double ninv,
                                                        uint32_t *__restrict__ out) {
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E;
  __shared__ double lds[CompactNtt::LDS_DOUBLES];
  __shared__ uint32_t vals[N2];
  const int tid = threadIdx.x;
  const int quads = 16 * bits;  // uint4 per polynomial
  size_t m = blockIdx.x;
  if (m >= n) return;  // the whole workgroup
  int h = 0;
  ulonglong2 cur[E / 2], nxt[E / 2];
  {
    const ulonglong2 *p = reinterpret_cast<const ulonglong2 *>(cts + m * 2 * N2 + tid * E);
#pragma unroll
    for (int k = 0; k < E / 2; ++k) cur[k] = p[k];
  }
#pragma unroll 1
  for (;;) {
    // this workgroup's next polynomial: b of the same ciphertext, or a of the next one
    const size_t nm = h ? m + gridDim.x : m;
    const int nh = h ^ 1;
    const bool more = nm < n;
    if (more) {
      const ulonglong2 *p = reinterpret_cast<const ulonglong2 *>(cts + (nm * 2 + nh) * N2 + tid * E);
#pragma unroll
      for (int k = 0; k < E / 2; ++k) nxt[k] = p[k];
    }
    double x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = from_u64<M>((e & 1 ? cur[e / 2].y : cur[e / 2].x) % Q2);
    CompactNtt::inv(x, lds, itw, tid);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const uint64_t c = to_u64<M>(canon<M>(mm<M>(canon<M>(x[e]), ninv)));
      vals[tid + e * T] = compact_rescale(c, bits);
    }
    wg_barrier_lds();
    uint4 *o = reinterpret_cast<uint4 *>(out + (m * 2 + h) * (size_t)(4 * quads));
    for (int q = tid; q < quads; q += T)
      o[q] = make_uint4(compact_stream_word(vals, 4 * q, bits, magic), compact_stream_word(vals, 4 * q + 1, bits, magic),
                        compact_stream_word(vals, 4 * q + 2, bits, magic), compact_stream_word(vals, 4 * q + 3, bits, magic));
    if (!more) break;
#pragma unroll
    for (int k = 0; k < E / 2; ++k) cur[k] = nxt[k];
    m = nm;
    h = nh;
  }
}

// The inverse, same geometry: a polynomial's 64 bits stream words come in as lane-consecutive 16-byte
// loads into LDS (8 KiB at most), thread tid takes values tid + 256 e out of them (the coefficient
// layout CompactNtt::fwd expects), compact_unscale, the forward NTT, and 64 contiguous bytes of canonical
// u64 per thread go out as four 16-byte stores. packed and cts must be 16-byte aligned.
//
// LDS reuse: `words` is not in the transform's buffers; the next polynomial's words are written after
// the trailing barrier of CompactNtt::fwd, which a thread reaches only after its reads of these.
__global__ __launch_bounds__(BR2_T) void expand_kernel(const uint32_t *__restrict__ packed, size_t n, int bits,
                                                       const double *__restrict__ tw, uint64_t *__restrict__ cts) {
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E;
  __shared__ double lds[CompactNtt::LDS_DOUBLES];
  __shared__ uint4 words4[COMPACT_MAX_POLY_WORDS / 4];
  const uint32_t *words = reinterpret_cast<const uint32_t *>(words4);
  const int tid = threadIdx.x;
  const int quads = 16 * bits;
  for (size_t m = blockIdx.x; m < n; m += gridDim.x) {
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const uint4 *p = reinterpret_cast<const uint4 *>(packed + (m * 2 + h) * (size_t)(4 * quads));
      for (int q = tid; q < quads; q += T) words4[q] = p[q];
      wg_barrier_lds();
      double x[E];
#pragma unroll
      for (int e = 0; e < E; ++e)
        x[e] = from_u64<M>(compact_unscale(compact_stream_value(words, tid + e * T, bits), bits));
      CompactNtt::fwd(x, lds, tw, tid);
      ulonglong2 *o = reinterpret_cast<ulonglong2 *>(cts + (m * 2 + h) * N2 + tid * E);
#pragma unroll
      for (int k = 0; k < E / 2; ++k)
        o[k] = make_ulonglong2(to_u64<M>(canon<M>(x[2 * k])), to_u64<M>(canon<M>(x[2 * k + 1])));
    }
  }
}

}  // namespace omr
