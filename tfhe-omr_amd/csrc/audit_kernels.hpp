// The auditor's kernel (gfx950; include/omr_gpu.h, "Auditor"): decrypt, decode, classify and
// noise-audit NttRlweCiphertexts under s2 without moving them off the device. Included only by
// audit.hip.
#pragma once

#include "audit_decode.hpp"
#include "kernels.hpp"

namespace omr {

using AuditNtt = WgNtt<Mod<2>, BR2_T, BR2_E>;
constexpr int AUDIT_WAVES = BR2_T / 64;
// A workgroup tallies its residual histogram in 32-bit LDS counters, 2,048 increments per ciphertext:
// the launch code gives one workgroup at most this many ciphertexts per launch (2^31 increments).
constexpr size_t AUDIT_MAX_PER_WORKGROUP = (size_t)1 << 20;
static_assert(sizeof(omr_ct_audit) == 16 && sizeof(omr_audit_summary) == 8 * (5 + OMR_AUDIT_RESIDUAL_BINS),
              "audit records as in include/omr_gpu.h");

// 256 threads x 8 residues, workgroup w takes ciphertexts w, w + grid, ...: phase
// c = N2^-1 INTT(b - a . NTT(s2)) with NTT(s2) in 8 registers per thread (thread tid owns NTT indices
// 8 tid + e, as AuditNtt::inv expects; it returns coefficient tid + 256 e in register e), then
// decode_coeff per coefficient. Per ciphertext: the decoded values (u16, lane-consecutive stores), one
// record (wave reduce, then four partials through LDS), and 2,048 increments of the workgroup's LDS
// histogram. After the loop the workgroup adds its tallies to the summary with global atomics (at most
// 55, none without a summary); a workgroup without a ciphertext touches nothing. records, decoded and
// summary may each be NULL. cts must be 16-byte aligned.
//
// LDS reuse: AuditNtt::inv ends with a workgroup barrier after its last exchange reads, so the next
// ciphertext's transform may write the exchange buffers at once. The reduction partials are not in
// those buffers and alternate between two sets: set k is rewritten two ciphertexts later, beyond the
// barrier of the ciphertext in between, which thread 0 only reaches after it has read set k.
__global__ __launch_bounds__(BR2_T) void audit_kernel(const uint64_t *__restrict__ cts, size_t n,
                                                      const double *__restrict__ s2_ntt,
                                                      const double *__restrict__ itw, double ninv,
                                                      omr_ct_audit *__restrict__ records,
                                                      uint16_t *__restrict__ decoded, omr_audit_summary *summary) {
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E;
  __shared__ double lds[AuditNtt::LDS_DOUBLES];
  __shared__ unsigned hist[OMR_AUDIT_RESIDUAL_BINS];
  __shared__ unsigned long long part_max[2][AUDIT_WAVES];
  __shared__ unsigned part_nz[2][AUDIT_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x >= n) return;  // the whole workgroup

  double s[E];
#pragma unroll
  for (int e = 0; e < E; ++e) s[e] = s2_ntt[tid * E + e];
  if (tid < OMR_AUDIT_RESIDUAL_BINS) hist[tid] = 0;
  __syncthreads();

  // thread 0's tallies of the workgroup's ciphertexts
  unsigned long long wg_count = 0, wg_zero = 0, wg_one_hot = 0, wg_other = 0, wg_max = 0;
  int set = 0;
  for (size_t m = blockIdx.x; m < n; m += gridDim.x, set ^= 1) {
    // 64 contiguous bytes of a and of b per thread: four 16-byte loads each
    const ulonglong2 *pa = reinterpret_cast<const ulonglong2 *>(cts + m * 2 * N2 + tid * E);
    const ulonglong2 *pb = pa + N2 / 2;
    ulonglong2 va[E / 2], vb[E / 2];
#pragma unroll
    for (int k = 0; k < E / 2; ++k) va[k] = pa[k];
#pragma unroll
    for (int k = 0; k < E / 2; ++k) vb[k] = pb[k];
    double x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const uint64_t a = (e & 1 ? va[e / 2].y : va[e / 2].x) % Q2, b = (e & 1 ? vb[e / 2].y : vb[e / 2].x) % Q2;
      // |b - a s| <= q/2 + 0.6 q (mm's bound for |a|, |s| <= q/2)
      x[e] = canon<M>(from_u64<M>(b) - mm<M>(from_u64<M>(a), s[e]));
    }
    AuditNtt::inv(x, lds, itw, tid);

    unsigned long long mx = 0;
    unsigned nz = 0, first = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      // the scaling of ntt_u64_kernel: canonical c in [0, q2)
      const uint64_t c = to_u64<M>(canon<M>(mm<M>(canon<M>(x[e]), ninv)));
      const DecodedCoeff d = decode_coeff(c);
      if (decoded) decoded[m * N2 + tid + e * T] = (uint16_t)d.t;
      if (e == 0) first = d.t;  // thread 0: coefficient 0
      nz += d.t != 0;
      mx = d.abs_r > mx ? d.abs_r : mx;
      atomicAdd(&hist[bit_length(d.abs_r)], 1u);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long om = __shfl_xor(mx, off);
      mx = om > mx ? om : mx;
      nz += __shfl_xor(nz, off);
    }
    if (lane == 0) {
      part_max[set][wave] = mx;
      part_nz[set][wave] = nz;
    }
    wg_barrier_lds();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < AUDIT_WAVES; ++w) {
        mx = part_max[set][w] > mx ? part_max[set][w] : mx;
        nz += part_nz[set][w];
      }
      if (records) records[m] = omr_ct_audit{mx, nz, first};
      ++wg_count;
      wg_zero += nz == 0;
      wg_one_hot += nz == 1 && first == 1;
      wg_other += !(nz == 0 || (nz == 1 && first == 1));
      wg_max = mx > wg_max ? mx : wg_max;
    }
  }

  if (!summary) return;
  __syncthreads();  // every wave's histogram increments
  auto *sum = reinterpret_cast<unsigned long long *>(summary);  // ciphertexts, zero, one_hot, other, max, bins
  if (tid < OMR_AUDIT_RESIDUAL_BINS && hist[tid]) atomicAdd(sum + 5 + tid, (unsigned long long)hist[tid]);
  if (tid == 0) {
    atomicAdd(sum + 0, wg_count);
    if (wg_zero) atomicAdd(sum + 1, wg_zero);
    if (wg_one_hot) atomicAdd(sum + 2, wg_one_hot);
    if (wg_other) atomicAdd(sum + 3, wg_other);
    if (wg_max) atomicMax(sum + 4, wg_max);
  }
}

}  // namespace omr
