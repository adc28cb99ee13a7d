// The body of br2x_kernel (br2_ntt.hpp) and of br2x_from_kernel (two_cu_from.hip), included inside each
// kernel's braces with OMR_BR2X_FROM defined 0 / 1. Shared as text, not as a function: called as an
// inlined body (template flag or run-time pointer) br2x_kernel compiled to other code than before, and so
// it did with a second kernel beside it in one translation unit. Uses the kernel's parameters lwe_int,
// bsk2, tb, xg, flags, err, out and, with OMR_BR2X_FROM, acc0 (canonical u64 [n][2][N2]).
  using M = Mod<2>;
  constexpr int T = BR2_T, E = BR2_E, N = N2;
  using NTT = CmuxNtt;
  constexpr int KD = D2 / 2;  // digits per group
  __shared__ double xbuf[2][NTT::LDS_DOUBLES];
  __shared__ double part[2][N];
  __shared__ double tws[CMUX_TWS];
  __shared__ int stop;
  const int m = blockIdx.x >> 1, r = blockIdx.x & 1;
  const int g = threadIdx.x / T, t = threadIdx.x % T;
  double *X = xbuf[g];
  double *ST = xbuf[0] + N;  // the staged accumulator (group 0's X1), read by both groups
  const double *tw = tws, *t0 = tws + N;
  const uint32_t *lwe = lwe_int + (size_t)m * (NI + 1);
  double acc[E];  // ACC_r, group 0 only
  {
#if OMR_BR2X_FROM
    const uint64_t *a0 = acc0 + (size_t)blockIdx.x * N;  // polynomial r of message m: [m][r][N]
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = from_u64<M>(a0[t + e * T]);
#else
    const int b = (int)lwe[NI];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = r == 1 ? acc2_init(tb.lut2, b, t + e * T) : 0.0;
#endif
    cmux_tables(tws, tb);
    if (threadIdx.x == 0) stop = 0;
    __syncthreads();
  }
  uint32_t hc = 0;  // hand-offs so far (executed steps)
  const int pslot = __builtin_amdgcn_readfirstlane(blockIdx.x < 2 ? 8 + 8 * (int)blockIdx.x + (int)(threadIdx.x >> 6) : -1);
  OMR_PHASE_CLOCK(pslot, 0);
#pragma unroll 1
  for (int i = 0; i < NI; ++i) {
    const int a = (int)__builtin_amdgcn_readfirstlane(lwe[i]) & (2 * N - 1);
    if (a == 0) continue;  // (X^0 - 1) * ACC = 0 (both workgroups of the message skip it)
    OMR_PHASE(pslot, (int)hc, 0);
    const size_t slot = hc & 1;
    const double *ggsw = bsk2 + ((size_t)i * 2 * D2 + (size_t)r * D2 + (size_t)g * KD) * 2 * N;
    uint32_t pk[E][Digits2::DW];
    cmux_decompose<false>(ST, g == 0, acc, a, t, pk);  // group 0 stages ACC_r, both groups decompose it
    OMR_PHASE(pslot, (int)hc, 1);
    double accA[E], accB[E];
    cmux_mac<KD, false>(pk, g * KD, ggsw, X, tw, t0, t, accA, accB);  // X0, X1, X0 (the staging used group 0's X1)
    // group 1's partials join group 0's; part[] is lane-contiguous (register e of thread t at
    // e * 256 + t: no LDS bank conflicts)
    if (g == 1) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        part[0][e * T + t] = red<M>(accA[e]);
        part[1][e * T + t] = red<M>(accB[e]);
      }
    }
    __syncthreads();
    OMR_PHASE(pslot, (int)hc, 3);
    double keep[E];
    if (g == 0) {
      double *mine = br2x_slot(xg, m, r, slot) + t;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double sa = red<M>(red<M>(accA[e]) + part[0][e * T + t]);
        const double sb = red<M>(red<M>(accB[e]) + part[1][e * T + t]);
        keep[e] = r == 0 ? sa : sb;
        st_sc1(mine + e * T, r == 0 ? sb : sa);  // the partner's output
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    OMR_PHASE(pslot, (int)hc, 4);
    if (threadIdx.x == 0) handoff_flags(flags + (size_t)m * BR2X_FLAGS, 2, r, hc + 1, false, &stop, err);
    __syncthreads();
    OMR_PHASE(pslot, (int)hc, 5);
    if (stop) break;
    if (g == 0) {
      const double *theirs = br2x_slot(xg, m, 1 - r, slot) + t;
      double s[E];
#pragma unroll
      for (int e = 0; e < E; ++e) s[e] = red<M>(keep[e] + ld_sc1(theirs + e * T));
      NTT::template inv<0>(s, X, tw, t, tw);
      OMR_PHASE(pslot, (int)hc, 6);
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = canon<M>(acc[e] + s[e]);
    } else {
      __syncthreads();  // the inverse's one workgroup barrier (its cross-wave exchange)
      OMR_PHASE(pslot, (int)hc, 6);
    }
    OMR_PHASE(pslot, (int)hc, 7);
    ++hc;
  }
  OMR_PHASE_CLOCK(pslot, 1);
  if (g == 0) {
    uint64_t *o = out + (size_t)m * 2 * N + (size_t)r * N;
#pragma unroll
    for (int e = 0; e < E; ++e) o[t + e * T] = to_u64<M>(acc[e]);
  }
