// The key audit's kernels (gfx950; include/omr_gpu.h, "Key audit"): the noise of detection-key rows under
// the secrets, where the key is, and the secret-free count of non-canonical words. Included only by
// audit.hip. The CPU statement of the same results is omr_audit_key_rows_cpu (key_audit.hip).
#pragma once

#include "audit_kernels.hpp"
#include "key_audit_math.hpp"

namespace omr {

static_assert(sizeof(omr_key_audit_summary) == 8 * (5 + OMR_AUDIT_RESIDUAL_BINS), "key audit summary as in include/omr_gpu.h");
// one launch per call: no component has more rows than one workgroup's 32-bit histogram allows
static_assert((size_t)N1 * KS_DIGITS <= AUDIT_MAX_PER_WORKGROUP && N1 <= N2, "key rows per workgroup");

// What the RLWE kernel needs besides the rows; pointers into the auditor's device buffers.
struct KeyAuditSecrets {
  const double *tw, *itw, *s_ntt;  // forward / inverse twiddles and NTT(s) of the level (centred)
  double ninv;                     // N^-1 mod q, centred
  const int8_t *s;                 // s in coefficient form, ternary
  const uint8_t *bits;             // s0 (BSK1) or s_int (BSK2); unused for TRACE
  const int8_t *sigma;             // [11][2048] sigma_g(s2) per trace step; TRACE only
};

// The workgroup's tallies -> the summary with global atomics: rows, noncanonical, max, rows_over,
// first_row_over, bins (at most 55 atomics; called by every thread after the histogram's barrier).
__device__ __forceinline__ void key_summary_flush(omr_key_audit_summary *summary, const unsigned *hist, int tid,
                                                  unsigned long long rows, unsigned long long nc, unsigned long long mx,
                                                  unsigned long long over, unsigned long long first_over) {
  auto *sum = reinterpret_cast<unsigned long long *>(summary);
  if (tid < OMR_AUDIT_RESIDUAL_BINS && hist[tid]) atomicAdd(sum + 5 + tid, (unsigned long long)hist[tid]);
  if (tid == 0) {
    atomicAdd(sum + 0, rows);
    if (nc) atomicAdd(sum + 1, nc);
    if (mx) atomicMax(sum + 2, mx);
    if (over) {
      atomicAdd(sum + 3, over);
      atomicMin(sum + 4, first_over);
    }
  }
}

// 256 threads x E words (4 at level 1, 8 at level 2); workgroup w takes rows w, w + grid, ... of the range,
// built like audit_kernel. NTT(s) stays in E registers per thread for the whole loop. Per row
// [a[N] | b[N]]: a s = N^-1 INTT(NTT(a) (.) NTT(s)), then e = b - a s -/+ message, centred, with the message
// from key_row_message(comp, first_row + m). The forward transform takes coefficient tid + T e in register
// e and the inverse returns the same layout, so a and b are read lane-consecutively (one fully coalesced
// 4- or 8-byte load per register; a 16-byte load per thread would need one more LDS exchange to reach this
// layout). Per row: row_max (wave reduce, then four partials through LDS) and N increments of the
// workgroup's LDS histogram; after the loop the tallies go to the summary. row_max or summary may be NULL.
//
// LDS reuse: fwd and inv each end with a workgroup barrier after their last exchange reads, so the next
// transform may write the exchange buffers at once. The reduction partials alternate between two sets,
// as in audit_kernel: set k is rewritten two rows later, beyond the barriers of the row in between.
template <int LEVEL, typename W>
__global__ __launch_bounds__(256) void key_audit_rlwe_kernel(const W *__restrict__ rows_ptr, int comp, size_t first_row,
                                                            size_t n, KeyAuditSecrets sec, uint64_t limit,
                                                            uint64_t *__restrict__ row_max,
                                                            omr_key_audit_summary *summary) {
  using M = Mod<LEVEL>;
  constexpr int T = 256, E = M::N / T;
  using NTT = WgNtt<M, T, E>;
  constexpr uint64_t Q = LEVEL == 1 ? Q1 : Q2;
  constexpr int WAVES = T / 64;
  __shared__ double lds[NTT::LDS_DOUBLES];
  __shared__ unsigned hist[OMR_AUDIT_RESIDUAL_BINS];
  __shared__ unsigned long long part_max[2][WAVES];
  __shared__ unsigned part_nc[2][WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x >= n) return;  // the whole workgroup

  double sn[E];
  int sc[E];  // s at the thread's coefficients tid + T e
#pragma unroll
  for (int e = 0; e < E; ++e) {
    sn[e] = sec.s_ntt[tid * E + e];
    sc[e] = sec.s[tid + e * T];
  }
  if (tid < OMR_AUDIT_RESIDUAL_BINS) hist[tid] = 0;
  __syncthreads();

  // thread 0's tallies of the workgroup's rows
  unsigned long long wg_rows = 0, wg_nc = 0, wg_max = 0, wg_over = 0, wg_first = ~0ull;
  int set = 0;
  for (size_t m = blockIdx.x; m < n; m += gridDim.x, set ^= 1) {
    const W *pa = rows_ptr + m * 2 * M::N, *pb = pa + M::N;
    W wa[E], wb[E];
#pragma unroll
    for (int e = 0; e < E; ++e) wa[e] = pa[tid + e * T];
#pragma unroll
    for (int e = 0; e < E; ++e) wb[e] = pb[tid + e * T];
    const KeyRowMessage msg = key_row_message(comp, first_row + m);  // workgroup-uniform
    // sign of the message at each of the thread's coefficients, times msg.mag (exact: mag < q / 2 < 2^49)
    const double mag = (double)msg.mag;
    const int bit = msg.kind == KA_TRACE ? 0 : (int)sec.bits[msg.index];

    unsigned nc = 0;
    double x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      nc += ((uint64_t)wa[e] >= Q) + ((uint64_t)wb[e] >= Q);
      x[e] = from_u64<M>((uint64_t)wa[e] % Q);
    }
    NTT::fwd(x, lds, sec.tw, tid);
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = mm<M>(canon<M>(x[e]), sn[e]);  // |.| <= 0.6 q
    NTT::inv(x, lds, sec.itw, tid);

    unsigned long long mx = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double as = canon<M>(mm<M>(canon<M>(x[e]), sec.ninv));
      const double ph = canon_small<M>(from_u64<M>((uint64_t)wb[e] % Q) - as);
      int sign;
      if (msg.kind == KA_TRACE) sign = sec.sigma[(size_t)msg.index * N2 + tid + e * T];
      else if (msg.kind == KA_A_GADGET) sign = bit * sc[e];
      else sign = (tid + e * T == 0) ? -bit : 0;
      // |ph| <= (q - 1) / 2 and mag < q / 2: one reduction centres the sum exactly
      const double ev = canon_small<M>(ph + (double)sign * mag);
      const unsigned long long a = (unsigned long long)fabs(ev);
      mx = a > mx ? a : mx;
      atomicAdd(&hist[key_noise_bits(a)], 1u);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long om = __shfl_xor(mx, off);
      mx = om > mx ? om : mx;
      nc += __shfl_xor(nc, off);
    }
    if (lane == 0) {
      part_max[set][wave] = mx;
      part_nc[set][wave] = nc;
    }
    wg_barrier_lds();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < WAVES; ++w) {
        mx = part_max[set][w] > mx ? part_max[set][w] : mx;
        nc += part_nc[set][w];
      }
      if (row_max) row_max[m] = mx;
      ++wg_rows;
      wg_nc += nc;
      wg_max = mx > wg_max ? mx : wg_max;
      if (mx > limit) {
        ++wg_over;
        wg_first = first_row + m < wg_first ? first_row + m : wg_first;
      }
    }
  }

  if (!summary) return;
  __syncthreads();  // every wave's histogram increments
  key_summary_flush(summary, hist, tid, wg_rows, wg_nc, wg_max, wg_over, wg_first);
}

// One wave per key-switching row [a[670] | b] (u32 mod q1), four waves per workgroup: wave v of workgroup w
// takes rows 4 w + v, 4 (w + grid) + v, ... Lane l sums the words a[l + 64 t] whose s_int bit is set (its 11
// bits sit in one register) in 64-bit integers, at most 11 words below 2^32 each; a wave reduce gives
// <a, s_int>, and lane 0 finishes e = b - <a, s_int> - s1_i 2^j mod q1 and tallies: one LDS histogram
// increment per row, and its wave's counts in registers. The waves never wait for each other inside the
// loop; after it their tallies meet in LDS and thread 0 adds the workgroup's to the summary (measured: the
// global atomics of one-wave workgroups cost 0.10 of 0.14 ms over the whole component).
constexpr int KSK_AUDIT_WAVES = 4;
__global__ __launch_bounds__(64 * KSK_AUDIT_WAVES) void key_audit_ksk_kernel(
    const uint32_t *__restrict__ rows_ptr, size_t first_row, size_t n, const uint8_t *__restrict__ sint,
    const int8_t *__restrict__ s1, uint64_t limit, uint64_t *__restrict__ row_max, omr_key_audit_summary *summary) {
  constexpr int PER_LANE = (NI + 63) / 64, WAVES = KSK_AUDIT_WAVES;
  __shared__ unsigned hist[OMR_AUDIT_RESIDUAL_BINS];
  __shared__ unsigned long long part[WAVES][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((size_t)blockIdx.x * WAVES >= n) return;  // the whole workgroup
  unsigned mask = 0;
#pragma unroll
  for (int t = 0; t < PER_LANE; ++t) {
    const int c = lane + 64 * t;
    if (c < NI && sint[c]) mask |= 1u << t;
  }
  if (tid < OMR_AUDIT_RESIDUAL_BINS) hist[tid] = 0;
  __syncthreads();

  // lane 0's tallies of the wave's rows
  unsigned long long wv_rows = 0, wv_nc = 0, wv_max = 0, wv_over = 0, wv_first = ~0ull;
  for (size_t m = (size_t)blockIdx.x * WAVES + wave; m < n; m += (size_t)gridDim.x * WAVES) {
    const uint32_t *p = rows_ptr + m * (NI + 1);
    // wave-uniform, and read before the row so that the loads overlap
    const KeyRowMessage msg = key_row_message(OMR_KEY_KSK, first_row + m);
    const int s1v = s1[msg.index];
    const uint32_t body = p[NI];
    unsigned long long acc = 0;
    unsigned nc = 0;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
      const int c = lane + 64 * t;
      if (c <= NI) {  // column NI is the body: counted, not summed
        const uint32_t v = p[c];
        nc += v >= Q1;
        if (c < NI && ((mask >> t) & 1u)) acc += v % (uint32_t)Q1;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      acc += __shfl_xor(acc, off);
      nc += __shfl_xor(nc, off);
    }
    if (lane == 0) {
      const uint64_t as = acc % Q1, b = body % (uint32_t)Q1;
      const uint64_t ph = b >= as ? b - as : b + Q1 - as;
      const uint64_t e = key_abs_centred(key_add_signed(ph, -s1v, msg.mag % Q1, Q1), Q1);
      if (row_max) row_max[m] = e;
      atomicAdd(&hist[key_noise_bits(e)], 1u);
      ++wv_rows;
      wv_nc += nc;
      wv_max = e > wv_max ? e : wv_max;
      if (e > limit) {
        ++wv_over;
        wv_first = first_row + m < wv_first ? first_row + m : wv_first;
      }
    }
  }
  if (!summary) return;
  if (lane == 0) {
    part[wave][0] = wv_rows;
    part[wave][1] = wv_nc;
    part[wave][2] = wv_max;
    part[wave][3] = wv_over;
    part[wave][4] = wv_first;
  }
  __syncthreads();  // the partials and every wave's histogram increments
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      wv_rows += part[w][0];
      wv_nc += part[w][1];
      wv_max = part[w][2] > wv_max ? part[w][2] : wv_max;
      wv_over += part[w][3];
      wv_first = part[w][4] < wv_first ? part[w][4] : wv_first;
    }
  }
  key_summary_flush(summary, hist, tid, wv_rows, wv_nc, wv_max, wv_over, wv_first);
}

// Words >= Q of n words: grid-stride compare, wave reduce, one atomic per wave that found any.
template <typename W, uint64_t Q>
__global__ __launch_bounds__(256) void count_noncanonical_kernel(const W *__restrict__ words, size_t n,
                                                                unsigned long long *count) {
  unsigned long long k = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    k += (uint64_t)words[i] >= Q;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) k += __shfl_xor(k, off);
  if ((threadIdx.x & 63) == 0 && k) atomicAdd(count, k);
}

}  // namespace omr
