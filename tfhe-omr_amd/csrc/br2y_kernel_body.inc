// The body of br2y_kernel (br2_fft.hpp) and of br2y_from_kernel (two_cu_from.hip), included inside each
// kernel's braces with OMR_BR2Y_FROM defined 0 / 1 (shared as text for br2x_kernel_body.inc's reason). Uses
// the kernel's parameters lwe_int, bskf, twg, tb, xg, flags, err, out, nmsg, w8, allow_fast and, with
// OMR_BR2Y_FROM, acc0 (canonical u64 [n][2][N2]).
  using F = Fft1024;
  using M = Mod<2>;
  constexpr int E = F::E, NN = N2, n = F::n, T = F::T;
  __shared__ double2 tws[n];
  __shared__ double2 xb[2][2][n];  // [group][X0, X1]
  __shared__ double2 px[2][n];     // [group]: its limb-(1 - g) partial of output 1 - r; the rounded halves
  __shared__ double acs[NN];       // ACC_r
  __shared__ int stop, same_xcd;
  const int m = (int)blockIdx.x % w8, row = (int)blockIdx.x / w8;  // uniform
  if (m >= nmsg) return;
  if (row >= 2) {
    br2y_prefetch(lwe_int, bskf, flags, 2 * m + ((row - 2) & 1), (row - 2) >> 1);
    return;
  }
  const int r = row, wid = 2 * m + r;
  const int g = __builtin_amdgcn_readfirstlane((int)threadIdx.x / T), t = (int)threadIdx.x % T;
  const int pslot = __builtin_amdgcn_readfirstlane(wid < 2 ? 8 + 8 * wid + (int)(threadIdx.x >> 6) : -1);
  OMR_PHASE_CLOCK(pslot, 0);
  const uint32_t *lwe = lwe_int + (size_t)m * (NI + 1);
  if (g == 0) F::load_twiddles(tws, twg, t);
  {  // ACC_r = X^{-b} * LUT2 (body) or 0 (mask)
#if OMR_BR2Y_FROM
    const uint64_t *a0 = acc0 + (size_t)wid * NN;  // polynomial r of message m: [m][r][N2]
    for (int c = (int)threadIdx.x; c < NN; c += BR2Y_T) acs[F::slot_stage(c)] = from_u64<M>(a0[c]);
#else
    const int b = (int)lwe[NI];
    for (int c = (int)threadIdx.x; c < NN; c += BR2Y_T) acs[F::slot_stage(c)] = r == 1 ? acc2_init(tb.lut2, b, c) : 0.0;
#endif
    if (threadIdx.x == 0) {
      stop = 0;
      // XCD ids through global memory (sc1 both ways); a partner that never answers leaves the
      // sc1 protocol in place (the step loop's bounded poll then reports it)
      uint32_t *xid = flags + 2 * nmsg;
      const uint32_t mine = (uint32_t)__builtin_amdgcn_s_getreg(6164) + 1u;  // hwreg(HW_REG_XCC_ID, 0, 4)
      __hip_atomic_store(xid + wid, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      uint32_t theirs = 0;
      for (int k = 0; k < (1 << 20) && theirs == 0; ++k) {
        theirs = __hip_atomic_load(xid + (wid ^ 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (theirs == 0) __builtin_amdgcn_s_sleep(2);
      }
      same_xcd = allow_fast && theirs == mine;
    }
  }
  double2 wc[4][2];  // this thread's forward twiddles of passes 1..4
  F::load_ct(wc, twg, t);
  __syncthreads();  // same_xcd (and the accumulator) visible
  const bool fast = __builtin_amdgcn_readfirstlane(same_xcd) != 0;
  const __amdgpu_buffer_rsrc_t rsrc = bsk2_rsrc(bskf);
  const uint32_t t16 = (uint32_t)t * 16u;
  uint32_t hc = 0;  // hand-offs so far (executed steps)
  double2 ka[2][E], kb[2][E];
  int pre = -1;  // the step whose first row ka / kb hold
#pragma unroll 1
  for (int i = 0; i < NI; ++i) {
    const int a = (int)__builtin_amdgcn_readfirstlane(lwe[i]) & (2 * NN - 1);
    if (a == 0) continue;  // (X^0 - 1) * ACC = 0 (both workgroups of the message skip it)
    OMR_PHASE(pslot, (int)hc, 0);
    const int q0 = i * 2 * D2 + r * D2 + 3 * g;  // the group's first GGSW row of this step
    if (pre != i) {
      br2f_load_half(ka, rsrc, q0, 0, t16);
      br2f_load_half(kb, rsrc, q0, 1, t16);
    }
    wg_barrier_lds();  // ACC_r (init or the previous update) visible; the previous step's LDS reads done
    uint32_t pw[2][E];  // word g of the digits at the thread's P0 points (coefficients j, j + 1024)
    {
      uint32_t pk[2][E][Digits2S::DW];
      br2f_digits(acs, a, t, pk);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < E; ++e) pw[h][e] = g ? pk[h][e][1] : pk[h][e][0];
    }
    OMR_PHASE(pslot, (int)hc, 1);
    double sr[2][2][E], si[2][2][E];  // [output][limb] partial spectra of the group's three digits
    br2f_zero(sr, si);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int wd = g == 1 && j == 2 ? Digits2S::TOP_WIDTH : 7;  // the top digit of word 1
      double xr[E], xi[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        xr[e] = (double)(int)__builtin_amdgcn_sbfe(pw[0][e], 7 * j, wd);
        xi[e] = (double)(int)__builtin_amdgcn_sbfe(pw[1][e], 7 * j, wd);
      }
      F::fwd(xr, xi, xb[g][j & 1], t, wc);
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        br2f_mac(xr, xi, o ? kb : ka, sr[o], si[o]);
        if (j < 2) br2f_load_half(o ? kb : ka, rsrc, q0 + j + 1, o, t16);
      }
    }
    OMR_PHASE(pslot, (int)hc, 2);
    // the four partials by role (r and g are uniform: selects, no dynamic register indexing):
    // [0] output r limb g (kept), [1] output r limb 1 - g, [2] output 1 - r limb g (handed to the
    // partner), [3] output 1 - r limb 1 - g
    double pr4[4][E], pi4[4][E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double rlr = r ? sr[1][0][e] : sr[0][0][e], rhr = r ? sr[1][1][e] : sr[0][1][e];
      const double nlr = r ? sr[0][0][e] : sr[1][0][e], nhr = r ? sr[0][1][e] : sr[1][1][e];
      const double rli = r ? si[1][0][e] : si[0][0][e], rhi = r ? si[1][1][e] : si[0][1][e];
      const double nli = r ? si[0][0][e] : si[1][0][e], nhi = r ? si[0][1][e] : si[1][1][e];
      pr4[0][e] = g ? rhr : rlr;
      pi4[0][e] = g ? rhi : rli;
      pr4[1][e] = g ? rlr : rhr;
      pi4[1][e] = g ? rli : rhi;
      pr4[2][e] = g ? nhr : nlr;
      pi4[2][e] = g ? nhi : nli;
      pr4[3][e] = g ? nlr : nhr;
      pi4[3][e] = g ? nli : nhi;
    }
    // limb swap: group g posts its limb-(1 - g) partials (output r in its X1, free since the third
    // transform's barrier; output 1 - r in px[g]) and takes the other group's limb-g ones
    {
      double2 *pr_ = xb[g][1], *ph = px[g];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        pr_[e * T + t] = make_double2(pr4[1][e], pi4[1][e]);
        ph[e * T + t] = make_double2(pr4[3][e], pi4[3][e]);
      }
    }
    wg_barrier_lds();
    OMR_PHASE(pslot, (int)hc, 3);
    double fr[E], fi[E];  // limb g of output r: this workgroup's six rows, then the partner's six
    {
      const double2 *qr = xb[1 - g][1], *qh = px[1 - g];
      double *dst = br2y_slot(xg, m, r, hc & 1, g);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double2 vr = qr[e * T + t], vh = qh[e * T + t];
        fr[e] = pr4[0][e] + vr.x;
        fi[e] = pi4[0][e] + vr.y;
        if (fast) {  // plain stores: the lines stay in this XCD's L2 for the partner's sc1 loads
          dst[e * T + t] = pr4[2][e] + vh.x;
          dst[n + e * T + t] = pi4[2][e] + vh.y;
        } else {
          st_sc1(dst + e * T + t, pr4[2][e] + vh.x);  // limb g of output 1 - r: the partner's
          st_sc1(dst + n + e * T + t, pi4[2][e] + vh.y);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    OMR_PHASE(pslot, (int)hc, 4);
    if (threadIdx.x == 0) handoff_flags(flags + 2 * m, 2, r, hc + 1, fast, &stop, err);  // fast: a plain flag store
    __syncthreads();
    OMR_PHASE(pslot, (int)hc, 5);
    if (stop) break;
    {  // the partner's limb g of output r
      const double *src = br2y_slot(xg, m, 1 - r, hc & 1, g);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        fr[e] += ld_sc1(src + e * T + t);
        fi[e] += ld_sc1(src + n + e * T + t);
      }
    }
    asm volatile("" : "+v"(fr[0]), "+v"(fr[1]), "+v"(fr[2]), "+v"(fr[3]), "+v"(fi[0]), "+v"(fi[1]), "+v"(fi[2]),
                 "+v"(fi[3])::"memory");  // consumed before the prefetch below is issued
    if (i + 1 < NI) {  // the next step's first row (kept when that step runs next)
      br2f_load_half(ka, rsrc, q0 + 2 * D2, 0, t16);
      br2f_load_half(kb, rsrc, q0 + 2 * D2, 1, t16);
      pre = i + 1;
    }
    F::inv(fr, fi, xb[g][1], tws, t);  // X1: every reader of the limb swap passed the hand-off barriers
    OMR_PHASE(pslot, (int)hc, 6);
    // round limb g; the groups swap halves: group g recombines the coefficients idx(0, t, e) + 1024 g
    double lv[2][E];  // [h][e]: limb g of coefficient idx(0, t, e) + 1024 h
#pragma unroll
    for (int e = 0; e < E; ++e) {
      lv[0][e] = rint(fr[e]);
      lv[1][e] = rint(fi[e]);
    }
    double *hx = reinterpret_cast<double *>(px[g]);
#pragma unroll
    for (int e = 0; e < E; ++e) hx[e * T + t] = g ? lv[0][e] : lv[1][e];
    wg_barrier_lds();
    const double *ho = reinterpret_cast<const double *>(px[1 - g]);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double other = ho[e * T + t];
      const double lo = g == 0 ? lv[0][e] : other, hr = g == 0 ? other : lv[1][e];
      double &acc = acs[F::slot_stage(F::idx(0, t, e) + n * g)];
      acc = limb_acc(acc, lo, hr);
    }
    OMR_PHASE(pslot, (int)hc, 7);
    ++hc;
  }
  OMR_PHASE_CLOCK(pslot, 1);
  __syncthreads();  // the last updates everywhere
  uint64_t *o = out + (size_t)m * 2 * NN + (size_t)r * NN;
  for (int c = (int)threadIdx.x; c < NN; c += BR2Y_T) o[c] = to_u64<M>(acs[F::slot_stage(c)]);
