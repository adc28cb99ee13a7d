// Level 2 on the exact modular NTT: the latency blind rotations (br2l_kernel: one workgroup per
// message; br2x_kernel: two, on two CUs), the homomorphic trace (trace_kernel; trace_x_kernel over
// TRACE_X CUs per message) and the exact fallbacks of a guarded throughput launch. Residues are
// exact integers in FP64 registers (device_ntt.hpp); same digits, rows and reduction points as
// the throughput kernels (br2_fft.hpp), so the outputs are bit-identical.
#pragma once

#include "exactness.hpp"
#include "handoff.hpp"
#include "level2_common.hpp"

namespace omr {

// ---- the CMUX step's parts (br2l_body, br2x_kernel) ----------------------------------------------
// Both kernels run 512 threads as two 256-thread groups, each with its own CmuxNtt buffers
// (staging X1, digits X0 X1 X0 .., inverse X0: consecutive cross-wave uses alternate); the
// workgroup barriers are a superset of a group's, and both groups run the same barrier sequence
// (a is uniform).
constexpr int BR2L_T = 2 * BR2_T;
constexpr int CMUX_TWS = N2 + 5 * 136;  // forward twiddles + the five small-digit stage tables

// The LDS tables, by all BR2L_T threads (the caller's barrier follows): tw2c, then table k of
// CmuxNtt::fwd_small: d * c_k, d = tid - 64 (c = tw1, tw2, tw1 tw2, tw3, tw1 tw3). The pass-0
// twiddles are read from this copy too (gt = tw): from the global table they were vector loads on
// every step's critical path (no restrict on DeviceTables' pointers, so no scalar loads).
__device__ __forceinline__ void cmux_tables(double *tws, const DeviceTables &tb) {
  using M = Mod<2>;
  for (int j = threadIdx.x; j < N2; j += BR2L_T) tws[j] = tb.tw2c[j];
  if (threadIdx.x <= 128) {
    const double w1 = tb.tw2[1], w2 = tb.tw2[2], w3 = tb.tw2[3];
    const double c[5] = {w1, w2, canon<M>(mm<M>(w1, w2)), w3, canon<M>(mm<M>(w1, w3))};
#pragma unroll
    for (int k = 0; k < 5; ++k)
      tws[N2 + 136 * k + threadIdx.x] = canon<M>(mm<M>((double)((int)threadIdx.x - 64), c[k]));
  }
}

// Digit words of (X^a - 1) * ACC, the accumulator staged at st (N2 doubles of LDS, coefficient
// t + e T): the threads with `stage` write their acc there, a workgroup barrier, then every
// thread decomposes its coefficients. OWN: minus the thread's own acc (br2l: each group stages and
// decomposes its own polynomial); otherwise minus the staged value (br2x: group 1 holds none).
template <bool OWN>
__device__ __forceinline__ void cmux_decompose(double *st, bool stage, const double (&acc)[BR2_E], int a, int t,
                                               uint32_t (&pk)[BR2_E][Digits2::DW]) {
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E, N = N2;
  if (stage) {
#pragma unroll
    for (int e = 0; e < E; ++e) st[t + e * T] = acc[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; ++e)
    Digits2::pack(canon_small<M>(rot_read_lds<N>(st, t + e * T, a) - (OWN ? acc[e] : st[t + e * T])), pk[e]);
  wave_lds_fence();
}

// The digit loop: digits first .. first + COUNT - 1 of pk in order (the throughput kernel's
// (j, j + 3) pairing measured 6 % slower in br2l: its row choice splits the loop body into blocks
// the scheduler cannot overlap), transformed on X0, X1, X0, .. and multiplied into accA / accB
// (zeroed here) by the GGSW rows at `rows`, one per digit, each loaded one digit ahead. The sums
// are reduced after every fourth product: four products on a reduced sum stay below 7.6q
// (tests/test_fp64_residues.py); three on a zero sum (COUNT = 3) below 5.3q. ROLLED: the loop over
// digit pairs is not unrolled.
template <int COUNT, bool ROLLED>
__device__ __forceinline__ void cmux_mac(const uint32_t (&pk)[BR2_E][Digits2::DW], int first, const double *rows,
                                         double *X, const double *tw, const double *t0, int t,
                                         double (&accA)[BR2_E], double (&accB)[BR2_E]) {
  using M = Mod<2>;
  constexpr int E = BR2_E, N = N2, PAIRS_UNROLLED = ROLLED ? 1 : (COUNT + 1) / 2;
#pragma unroll
  for (int e = 0; e < E; ++e) accA[e] = accB[e] = 0.0;
  KeyRow<double, E> cur;
  cur.load(rows, N, t * E);
#pragma unroll PAIRS_UNROLLED
  for (int h2 = 0; h2 < COUNT; h2 += 2) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int h = h2 + b;
      if (COUNT % 2 && h >= COUNT) break;
      double x[E];
      int f[E];
#pragma unroll
      for (int e = 0; e < E; ++e) f[e] = Digits2::get_int(pk[e], first + h) + 64;
      if (b == 0)
        CmuxNtt::template fwd_small<0>(f, t0, x, X, tw, t, tw);
      else
        CmuxNtt::template fwd_small<1>(f, t0, x, X, tw, t, tw);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        accA[e] += mm<M>(x[e], cur.a[e]);
        accB[e] += mm<M>(x[e], cur.b[e]);
      }
      if ((h & 3) == 3) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          accA[e] = red<M>(accA[e]);
          accB[e] = red<M>(accB[e]);
        }
      }
      if (h + 1 < COUNT) cur.load(rows + (size_t)(h + 1) * 2 * N, N, t * E);
    }
  }
}

// Everything below defines kernels: two_cu_from.hip, which needs the parts above only, defines
// OMR_LEVEL2_PARTS_ONLY (a kernel's host stub may be defined in one translation unit only: ctx.hpp).
#ifndef OMR_LEVEL2_PARTS_ONLY

// ---- level 2, one workgroup per message -----------------------------------------------------------
// Group 0 owns the mask accumulator and its 6 digits (GGSW rows 0..5), group 1 the body
// accumulator and rows 6..11 (6 + 1 transforms per group instead of the throughput kernel's
// 12 + 2). Per CMUX step each group stages its polynomial, transforms its 6 digits and
// multiply-accumulates both outputs; group 0 hands its output-B partial to group 1 and group 1 its
// output-A partial to group 0 through `part`; each group then runs one inverse transform. Output:
// the blind rotation in the coefficient domain, u64 [2][N2] (mode 1 of br2f_kernel); trace_kernel
// finishes mode 0.
// acc0 (the test entries omr_blind_rotate_level2_from; nullptr in the production kernels, where the
// branch folds away): the initial accumulator is acc0's message (canonical u64 [2][N2], the output's
// layout) instead. A pointer tested at run time, not a template flag: as a template instantiation
// this body compiled to different code in br2l_kernel (192 instead of 194 VGPRs, another schedule).
__device__ __forceinline__ void br2l_body(const uint32_t *__restrict__ lwe_int, const double *__restrict__ bsk2,
                                          DeviceTables tb, uint64_t *__restrict__ out,
                                          const uint64_t *acc0 = nullptr) {
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E, N = N2;
  using NTT = CmuxNtt;
  __shared__ double xbuf[2][NTT::LDS_DOUBLES];
  __shared__ double part[2][N];
  __shared__ double tws[CMUX_TWS];
  const int g = threadIdx.x / T, t = threadIdx.x % T;
  double *X = xbuf[g];
  const double *tw = tws, *t0 = tws + N;
  const uint32_t *lwe = lwe_int + (size_t)blockIdx.x * (NI + 1);
  double acc[E];
  {
    if (acc0) {
      const uint64_t *a0 = acc0 + (size_t)blockIdx.x * 2 * N + (size_t)g * N;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = from_u64<M>(a0[t + e * T]);
    } else {
      const int b = (int)lwe[NI];
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = g == 1 ? acc2_init(tb.lut2, b, t + e * T) : 0.0;
    }
    cmux_tables(tws, tb);
    __syncthreads();
  }
#pragma unroll 1
  for (int i = 0; i < NI; ++i) {
    const int a = (int)__builtin_amdgcn_readfirstlane(lwe[i]) & (2 * N - 1);
    if (a == 0) continue;  // (X^0 - 1) * ACC = 0
    const double *ggsw = bsk2 + ((size_t)i * 2 * D2 + (size_t)g * D2) * 2 * N;
    uint32_t pk[E][Digits2::DW];
    cmux_decompose<true>(X + N, true, acc, a, t, pk);  // staged in the group's X1
    double accA[E], accB[E];
    cmux_mac<D2, true>(pk, 0, ggsw, X, tw, t0, t, accA, accB);
    // exchange the partial the other group owns: group 0 sends B, group 1 sends A
#pragma unroll
    for (int e = 0; e < E; ++e) part[1 - g][e * T + t] = red<M>(g == 0 ? accB[e] : accA[e]);
    __syncthreads();
    double s[E];
#pragma unroll
    for (int e = 0; e < E; ++e) s[e] = red<M>(red<M>(g == 0 ? accA[e] : accB[e]) + part[g][e * T + t]);
    NTT::template inv<0>(s, X, tw, t, tw);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = canon<M>(acc[e] + s[e]);
  }
  uint64_t *o = out + (size_t)blockIdx.x * 2 * N + (size_t)g * N;
#pragma unroll
  for (int e = 0; e < E; ++e) o[t + e * T] = to_u64<M>(acc[e]);
}
__global__ __launch_bounds__(BR2L_T, 1) void br2l_kernel(const uint32_t *__restrict__ lwe_int,
                                                         const double *__restrict__ bsk2, DeviceTables tb,
                                                         uint64_t *__restrict__ out) {
  br2l_body(lwe_int, bsk2, tb, out);
}
// The exact fallback of a guarded throughput level-2 launch (detect.hip, launch_br2): the same
// rotation on the modular NTT, run only when that launch's observed rounding margin reached the
// certificate threshold 1 - E2 (every workgroup reads the word and leaves otherwise).
__global__ __launch_bounds__(BR2L_T, 1) void br2l_fallback_kernel(const uint32_t *__restrict__ lwe_int,
                                                                  const double *__restrict__ bsk2, DeviceTables tb,
                                                                  uint64_t *__restrict__ out,
                                                                  const unsigned long long *lmargin, double thr) {
  if (!margin_breached(lmargin, thr)) return;
  br2l_body(lwe_int, bsk2, tb, out);
}
// Both of the above from acc0, as one kernel (lmargin == nullptr: unconditional).
__global__ __launch_bounds__(BR2L_T, 1) void br2l_from_kernel(const uint32_t *__restrict__ lwe_int,
                                                              const double *__restrict__ bsk2, DeviceTables tb,
                                                              uint64_t *__restrict__ out,
                                                              const unsigned long long *lmargin, double thr,
                                                              const uint64_t *__restrict__ acc0) {
  if (lmargin && !margin_breached(lmargin, thr)) return;
  br2l_body(lwe_int, bsk2, tb, out, acc0);
}

// ---- level 2 over two CUs per message --------------------------------------------------------
// Workgroup 2m + r owns polynomial r (0 mask, 1 body) of message m and its accumulator: its two
// 256-thread groups transform digits 3g .. 3g + 2 of that polynomial (GGSW rows r D2 + 3g + ..)
// and multiply-accumulate both outputs; group 1's partials join group 0's through LDS; the
// output the partner owns (mask CU: B, body CU: A) crosses to it through global memory and the
// partner's arrives the same way (handoff.hpp); group 0 runs the inverse transform and updates
// ACC_r. Half the transforms of br2l_kernel per CU and step, plus one hand-off.
// The hand-off slots are lane-contiguous (register e of thread t at e * 256 + t): each 8 B sc1 store
// or load instruction covers 512 B of four whole lines (profiles/r03q/handoff_layout_ab.log).
// Steps with a_i = 0 are skipped by both workgroups, so the hand-offs are numbered by a counter hc
// of EXECUTED steps: the flag carries hc + 1 and the payload slot is hc & 1.
__global__ __launch_bounds__(BR2L_T, 1) void br2x_kernel(const uint32_t *__restrict__ lwe_int,
                                                         const double *__restrict__ bsk2, DeviceTables tb,
                                                         double *xg, uint32_t *flags, int *err,
                                                         uint64_t *__restrict__ out) {
#define OMR_BR2X_FROM 0
#include "br2x_kernel_body.inc"
#undef OMR_BR2X_FROM
}

// ---- hom_trace (detector.rs:626-639) on the NTT ---------------------------------------------------
// c *= N^-1; for each automorphism k: c += KS_k(sigma_g(c)); output NTT(c). The mask stays in the
// coefficient domain (ca, layout tid + e*T); the body moves to the NTT domain (cb, layout
// tid*E + e) where sigma_g is an index permutation. The steps below are shared by the one-group
// trace (hom_trace_store) and the trace over TRACE_X workgroups (trace_x_kernel). tw / itw: NTT
// twiddles in LDS; xch: N2 doubles of LDS.
using TraceNtt = WgNtt<Mod<2>, BR2_T, BR2_E>;

// c *= N^-1, the body to the NTT domain; both canonical
__device__ __forceinline__ void trace_scale(double (&ca)[BR2_E], double (&cb)[BR2_E], double *xch, const double *tw,
                                            int tid) {
  using M = Mod<2>;
#pragma unroll
  for (int e = 0; e < BR2_E; ++e) {
    ca[e] = canon<M>(mm<M>(ca[e], NINV2));
    cb[e] = canon<M>(mm<M>(cb[e], NINV2));
  }
  TraceNtt::fwd(cb, xch, tw, tid);
#pragma unroll
  for (int e = 0; e < BR2_E; ++e) cb[e] = canon<M>(cb[e]);
}
// the digit words of sigma_g(a) (src: the automorphism's signed source indices)
__device__ __forceinline__ void trace_digits(const double (&ca)[BR2_E], const uint16_t *src, double *xch, int tid,
                                             uint32_t (&pk)[BR2_E][DigitsTrace::DW]) {
  constexpr int T = BR2_T, E = BR2_E, N = N2;
#pragma unroll
  for (int e = 0; e < E; ++e) xch[tid + e * T] = ca[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int s = src[tid + e * T];
    DigitsTrace::pack(s < N ? xch[s] : -xch[s - N], pk[e]);
  }
  __syncthreads();
}
// b_ntt += sigma_g(b)_ntt + B
__device__ __forceinline__ void trace_body_update(double (&cb)[BR2_E], const double (&accB)[BR2_E],
                                                  const uint16_t *perm, double *xch, int tid) {
  using M = Mod<2>;
  constexpr int E = BR2_E;
#pragma unroll
  for (int e = 0; e < E; ++e) xch[tid * E + e] = cb[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; ++e) cb[e] = canon<M>(cb[e] + xch[perm[tid * E + e]] + red<M>(accB[e]));
  __syncthreads();
}
// a += INTT(A); the caller has reduced A
__device__ __forceinline__ void trace_mask_update(double (&ca)[BR2_E], double (&accA)[BR2_E], double *xch,
                                                  const double *itw, int tid) {
  TraceNtt::inv(accA, xch, itw, tid);
#pragma unroll
  for (int e = 0; e < BR2_E; ++e) ca[e] = canon<Mod<2>>(ca[e] + accA[e]);
}
// NTT(c) as NttRlweCiphertext u64 [2][N2] at o
__device__ __forceinline__ void trace_store(double (&ca)[BR2_E], const double (&cb)[BR2_E], double *xch,
                                            const double *tw, uint64_t *__restrict__ o, int tid) {
  using M = Mod<2>;
  TraceNtt::fwd(ca, xch, tw, tid);
#pragma unroll
  for (int e = 0; e < BR2_E; ++e) {
    const int t = tid * BR2_E + e;
    o[t] = to_u64<M>(canon<M>(ca[e]));
    o[N2 + t] = to_u64<M>(cb[e]);
  }
}

// hom_trace of the level-2 accumulator (ca mask, cb body: coefficient layout tid + e*T, canonical)
// and store of NTT(c) at o.
__device__ __forceinline__ void hom_trace_store(double (&ca)[BR2_E], double (&cb)[BR2_E], double *xch,
                                                const double *tw, const double *itw, const double *__restrict__ tk,
                                                const DeviceTables &tb, uint64_t *__restrict__ o, int tid) {
  using M = Mod<2>;
  constexpr int E = BR2_E, N = N2;
  trace_scale(ca, cb, xch, tw, tid);
#pragma unroll 1
  for (int k = 0; k < TRACE_STEPS; ++k) {
    uint32_t pk[E][DigitsTrace::DW];
    trace_digits(ca, tb.trace_src + k * N, xch, tid, pk);
    // The digit loop (trace_x_kernel's is this one from w in steps of TRACE_X, reducing after every
    // third executed digit; as one function of start and stride, in every spelling tried, either
    // kernel allocates two VGPRs more than before, so each keeps its text).
    double accA[E], accB[E];
#pragma unroll
    for (int e = 0; e < E; ++e) accA[e] = accB[e] = 0.0;
    const double *key = tk + (size_t)k * DT * 2 * N;
#pragma unroll 1
    for (int d = 0; d < DT; ++d) {
      const double *ka = key + (size_t)(d * 2) * N + tid * E;  // alpha (pre-scaled by N^-1)
      const double *kb = ka + N;                                 // beta (unscaled)
      double kra[E], krb[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        kra[e] = ka[e];
        krb[e] = kb[e];
      }
      double x[E];
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = DigitsTrace::get(pk[e], d);
      TraceNtt::fwd(x, xch, tw, tid);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        accA[e] += mm<M>(x[e], kra[e]);
        accB[e] += mm<M>(x[e], krb[e]);
      }
      if ((d % 3) == 2) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          accA[e] = red<M>(accA[e]);
          accB[e] = red<M>(accB[e]);
        }
      }
    }
    trace_body_update(cb, accB, tb.trace_perm + k * N, xch, tid);
#pragma unroll
    for (int e = 0; e < E; ++e) accA[e] = red<M>(accA[e]);
    trace_mask_update(ca, accA, xch, itw, tid);
  }
  trace_store(ca, cb, xch, tw, o, tid);
}

// In place on blind-rotation outputs (coefficient domain, canonical u64 [2][N2] per message) ->
// NttRlweCiphertext u64 [2][N2].
__device__ __forceinline__ void trace_body(uint64_t *__restrict__ io, const double *__restrict__ tk, DeviceTables tb) {
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E, N = N2;
  __shared__ double xch[TraceNtt::LDS3_DOUBLES];
  __shared__ double tws[N];
  const int tid = threadIdx.x;
  uint64_t *o = io + (size_t)blockIdx.x * 2 * N;
  double acc0[E], acc1[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    acc0[e] = from_u64<M>(o[tid + e * T]);
    acc1[e] = from_u64<M>(o[N + tid + e * T]);
    tws[tid + e * T] = tb.tw2[tid + e * T];
    xch[2 * N + tid + e * T] = tb.itw2[tid + e * T];
  }
  __syncthreads();
  hom_trace_store(acc0, acc1, xch, tws, xch + 2 * N, tk, tb, o, tid);
}
__global__ __launch_bounds__(BR2_T, 2) void trace_kernel(uint64_t *__restrict__ io, const double *__restrict__ tk,
                                                         DeviceTables tb) {
  trace_body(io, tk, tb);
}
// trace of br2l_fallback_kernel's output (same condition)
__global__ __launch_bounds__(BR2_T, 2) void trace_fallback_kernel(uint64_t *__restrict__ io, const double *__restrict__ tk,
                                                                  DeviceTables tb, const unsigned long long *lmargin,
                                                                  double thr) {
  if (!margin_breached(lmargin, thr)) return;
  trace_body(io, tk, tb);
}

// omr_trace's guarded run: the saved input back in place ahead of trace_fallback_kernel (same condition;
// within launch_br2 the fallback rotation rewrites the trace's input instead)
__global__ __launch_bounds__(BR2_T, 2) void trace_restore_kernel(uint64_t *__restrict__ io,
                                                                 const uint64_t *__restrict__ saved,
                                                                 const unsigned long long *lmargin, double thr) {
  if (!margin_breached(lmargin, thr)) return;
  const size_t base = (size_t)blockIdx.x * 2 * N2;
  for (int j = threadIdx.x; j < 2 * N2; j += BR2_T) io[base + j] = saved[base + j];
}

// hom_trace of the latency path over TRACE_X workgroups (CUs) per message: every workgroup keeps
// the mask and body (redundantly: the per-step updates are cheap), takes the 25 digits of
// sigma_g(a) and transforms and multiply-accumulates only digits d = w, w + TRACE_X, ...; the
// partial sums (A, B), reduced, are all-reduced through global memory (handoff.hpp: one flag per
// workgroup carrying the step + 1, slot = step parity), then every workgroup applies B to the body
// and INTT(A) to the mask. Workgroup 0 stores NTT(c). The partials are canonicalised before the
// exchange, so their sum stays below TRACE_X q / 2 < 2^53, and the residues are canonicalised as in
// hom_trace_store: the output is bit-identical to it.
__global__ __launch_bounds__(BR2_T, 2) void trace_x_kernel(uint64_t *__restrict__ io, const double *__restrict__ tk,
                                                           DeviceTables tb, double *xg, uint32_t *flags, int *err) {
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E, N = N2;
  __shared__ double xch[TraceNtt::LDS_DOUBLES];
  __shared__ double tw[N], itw[N];
  __shared__ int stop;
  const int m = blockIdx.x / TRACE_X, w = blockIdx.x % TRACE_X;
  const int tid = threadIdx.x;
  uint64_t *o = io + (size_t)m * 2 * N;
  double ca[E], cb[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    ca[e] = from_u64<M>(o[tid + e * T]);
    cb[e] = from_u64<M>(o[N + tid + e * T]);
    tw[tid + e * T] = tb.tw2[tid + e * T];
    itw[tid + e * T] = tb.itw2[tid + e * T];
  }
  if (tid == 0) stop = 0;
  __syncthreads();
  trace_scale(ca, cb, xch, tw, tid);
#pragma unroll 1
  for (int k = 0; k < TRACE_STEPS; ++k) {
    uint32_t pk[E][DigitsTrace::DW];
    trace_digits(ca, tb.trace_src + k * N, xch, tid, pk);
    // hom_trace_store's digit loop from w in steps of TRACE_X (see there)
    double accA[E], accB[E];
#pragma unroll
    for (int e = 0; e < E; ++e) accA[e] = accB[e] = 0.0;
    const double *key = tk + (size_t)k * DT * 2 * N;
    int cnt = 0;
#pragma unroll 1
    for (int d = w; d < DT; d += TRACE_X) {
      const double *ka = key + (size_t)(d * 2) * N + tid * E;
      const double *kb = ka + N;
      double kra[E], krb[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        kra[e] = ka[e];
        krb[e] = kb[e];
      }
      double x[E];
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = DigitsTrace::get(pk[e], d);
      TraceNtt::fwd(x, xch, tw, tid);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        accA[e] += mm<M>(x[e], kra[e]);
        accB[e] += mm<M>(x[e], krb[e]);
      }
      if ((++cnt % 3) == 0) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          accA[e] = red<M>(accA[e]);
          accB[e] = red<M>(accB[e]);
        }
      }
    }
    // all-reduce of the partials
    double *mine = trace_x_slot(xg, m, w, k & 1) + tid;  // lane-contiguous: 512 B per store instruction
#pragma unroll
    for (int e = 0; e < E; ++e) {
      accA[e] = red<M>(red<M>(accA[e]));  // canonical: TRACE_X of them sum below TRACE_X q / 2
      accB[e] = red<M>(red<M>(accB[e]));
      st_sc1(mine + e * T, accA[e]);
      st_sc1(mine + N + e * T, accB[e]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) handoff_flags(flags + (size_t)m * TRACE_X_FLAGS, TRACE_X, w, (uint32_t)(k + 1), false, &stop, err);
    __syncthreads();
    if (stop) break;
#pragma unroll
    for (int p = 0; p < TRACE_X; ++p) {
      if (p == w) continue;
      const double *theirs = trace_x_slot(xg, m, p, k & 1) + tid;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        accA[e] += ld_sc1(theirs + e * T);
        accB[e] += ld_sc1(theirs + N + e * T);
      }
    }
    trace_body_update(cb, accB, tb.trace_perm + k * N, xch, tid);
    // (the sum of partials canonicalised first: a tighter input than the one-group trace's)
#pragma unroll
    for (int e = 0; e < E; ++e) accA[e] = red<M>(red<M>(accA[e]));
    trace_mask_update(ca, accA, xch, itw, tid);
  }
  if (w != 0 || stop) return;
  trace_store(ca, cb, xch, tw, o, tid);
}

#endif  // OMR_LEVEL2_PARTS_ONLY

}  // namespace omr
