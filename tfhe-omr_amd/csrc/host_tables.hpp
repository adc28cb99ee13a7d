// Host-side tables of the detector context (context.hip uploads them; no HIP runtime call here):
// the modular NTT twiddles and LUTs, the FFT twiddle tables of Fft512 / Fft1024, the double-double
// tree twiddles of the key transforms, the CmuxNtt mirror of the level-2 twiddles, the trace
// permutation tables and the a priori rounding bound. Every entry's arithmetic is fixed: the tables
// are compared bit for bit with tests/golden/host_tables.npz (tests/test_host_tables.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "exactness.hpp"
#include "fft1024.hpp"
#include "host_ring.hpp"

namespace omr {

// psi^brv(k), psi^-brv(k) as centred doubles (the convention of include/omr_gpu.h).
inline void twiddles(uint64_t q, int N, uint64_t g, std::vector<double> &tw, std::vector<double> &itw) {
  const int L = __builtin_ctz(N);
  const uint64_t psi = powmod(g, (q - 1) / (2 * (uint64_t)N), q);
  const uint64_t ipsi = powmod(psi, q - 2, q);
  tw.resize(N);
  itw.resize(N);
  for (int k = 0; k < N; ++k) {
    const uint32_t e = bitrev((uint32_t)k, L);
    tw[k] = centred(powmod(psi, e, q), q);
    itw[k] = centred(powmod(ipsi, e, q), q);
  }
}
// N^-1 mod q, centred.
inline double ninv_centred(int N, uint64_t q) { return centred(powmod((uint64_t)N, q - 2, q), q); }

// LookUpTable::negacyclic_lut (lut.rs:12-27): chunk c of N >> log_t coefficients holds
// v[(c+1)/2] (itertools::interleave(v, v[1..])).
inline std::vector<double> negacyclic_lut(const std::vector<uint64_t> &v, int N, int log_t, uint64_t q) {
  std::vector<double> lut(N, 0.0);
  const int hd = N >> log_t;
  for (int c = 0; c < N / hd; ++c) {
    const size_t idx = (size_t)(c + 1) / 2;
    const uint64_t val = idx < v.size() ? v[idx] : 0;
    for (int j = 0; j < hd; ++j) lut[c * hd + j] = centred(val, q);
  }
  return lut;
}
// The detector's two LUTs (detector.rs:457-476 and :479-503).
inline std::vector<double> first_level_lut() {
  const uint64_t one1 = ((Q1 >> 4) + 1) >> 1;
  return negacyclic_lut({one1, 0, 0, 0, Q1 - one1}, N1, 3, Q1);
}
inline std::vector<double> second_level_lut() {
  std::vector<uint64_t> v2(TI, 0);
  v2[2 * CLUES] = (2 * Q2 + P) / (2 * P);  // round_half_up(q2/257)
  return negacyclic_lut(v2, N2, 5, Q2);
}

// The epsilon tree of the FFTs with n = 2^L points: eps(0, 0) = n, eps(s+1, 2i) = eps(s, i) / 2,
// eps(s+1, 2i+1) = eps(s, i) / 2 + 2n (mod 4n). Returns half[s][i] = eps(s, i) / 2, the integer
// exponent of node i of stage s: its twiddle is w^half[s][i], w = exp(i pi / 2n).
inline std::vector<std::vector<long>> eps_tree(int L) {
  const long n = 1L << L;
  std::vector<std::vector<long>> half(L);
  std::vector<long> eps{n};
  for (int s = 0; s < L; ++s) {
    std::vector<long> next;
    for (long e : eps) {
      half[s].push_back(e / 2);
      next.push_back((e / 2) % (4 * n));
      next.push_back((e / 2 + 2 * n) % (4 * n));
    }
    eps.swap(next);
  }
  return half;
}

// w^h for the FP64 FFT tables: the exact angle pi h / 2n evaluated in long double and rounded once.
struct TreeAngle {
  long n;
  long double angle(long h) const {
    return 3.14159265358979323846264338327950288L * (long double)(h % (8 * n)) / (long double)(2 * n);
  }
  double2 at(long h) const { return make_double2((double)cosl(angle(h)), (double)sinl(angle(h))); }
  // tangent form (cos, tan), tan = sin / cos in long double; no node of the tree lies on an axis, so cos != 0
  double2 ct(long h) const {
    const long double c = cosl(angle(h)), s = sinl(angle(h));
    return make_double2((double)c, (double)(s / c));
  }
};

// FFT twiddles of Fft512 (device_fft.hpp, WgFft): node i of stage s -> w^(eps(s, i) / 2),
// w = exp(i pi / 2n), n = 512 (eps_tree). Layout (WgFft::TW_*): [0, 7) T_1..T_7 of the
// pass-0 radix-8 block (A = node(0, 0), B = node(1, 0), C = node(2, 0), T = (C, B, BC, A, AC, AB,
// ABC)), inverse only; [7, 11) the tangent forms (cos, tan) of pass 0's A, B, C, w8 C = node(2, 2);
// 11 + 2 blk + (A, B) the tangent forms of the pass-1 radix-4 block blk (A = node(3, blk),
// B = node(4, 2 blk)); 27 + (t - 1) 32 + hi the pass-2 T_t (A = node(5, hi), B = node(6, 2 hi),
// C = node(7, 4 hi)), inverse only; 251 + 32 k + hi the tangent forms of pass 2's A, B, C, w8 C;
// 379 + 64 e1 + lane the tangent form of the pass-3 (stage 8) even-sibling node
// ((lane & 31) << 3 | (lane >> 5) << 2 | e1 << 1). Each entry is an exact angle (sum of the nodes'
// integer half-eps) evaluated in long double and rounded once (tan = sin / cos in long double).
inline std::vector<double2> fft_twiddles() {
  using F = Fft512;
  const int L = 9, n = 1 << L;
  std::vector<double2> tw(n, make_double2(1.0, 0.0));
  const auto half = eps_tree(L);
  const TreeAngle w{n};
  auto radix8 = [&](int s0, int hi, auto put) {
    const long a = half[s0][hi], b = half[s0 + 1][2 * hi], c = half[s0 + 2][4 * hi];
    const long h[8] = {0, c, b, b + c, a, a + c, a + b, a + b + c};
    for (int t = 1; t < 8; ++t) put(t, w.at(h[t]));
  };
  auto radix8_ct = [&](int s0, int hi, auto put) {
    const long h[4] = {half[s0][hi], half[s0 + 1][2 * hi], half[s0 + 2][4 * hi], half[s0 + 2][4 * hi + 2]};
    for (int k = 0; k < 4; ++k) put(k, w.ct(h[k]));
  };
  radix8(0, 0, [&](int t, double2 v) { tw[F::TW_P0I + t - 1] = v; });
  radix8_ct(0, 0, [&](int k, double2 v) { tw[F::TW_P0F + k] = v; });
  for (int blk = 0; blk < 8; ++blk) {
    tw[F::TW_P1 + 2 * blk] = w.ct(half[3][blk]);
    tw[F::TW_P1 + 2 * blk + 1] = w.ct(half[4][2 * blk]);
  }
  for (int hi = 0; hi < 32; ++hi) {
    radix8(5, hi, [&](int t, double2 v) { tw[F::TW_P2I + (t - 1) * 32 + hi] = v; });
    radix8_ct(5, hi, [&](int k, double2 v) { tw[F::TW_P2F + k * 32 + hi] = v; });
  }
  for (int e1 = 0; e1 < 2; ++e1)
    for (int lane = 0; lane < 64; ++lane)
      tw[F::TW_P3 + 64 * e1 + lane] = w.ct(half[8][((lane & 31) << 3) | ((lane >> 5) << 2) | (e1 << 1)]);
  return tw;
}

// Fft1024 twiddles (fft1024.hpp): pass p = 1..4, block hi -> (B, A, AB) at tw_off(p) + 3 hi (the
// inverse), then the forward's tangent forms (cos, tan) of (A, B) at TW_LEN + ct_off(p) + 2 hi, with
// A = W(2p, hi), B = W(2p + 1, 2 hi) of the tree with n = 1024 (eps(0, 0) = n, w = e^{i pi / 2n});
// each entry an exact angle evaluated in long double and rounded once.
inline std::vector<double2> fft2_twiddles() {
  const int L = 10, n = 1 << L;
  const auto half = eps_tree(L);
  const TreeAngle w{n};
  std::vector<double2> tw(Fft1024::TW_LEN + Fft1024::CT_LEN);
  int off = 0;
  for (int p = 1; p <= 4; ++p)
    for (int hi = 0; hi < (1 << (2 * p)); ++hi) {
      const long a = half[2 * p][hi], b = half[2 * p + 1][2 * hi];
      tw[off++] = w.at(b);
      tw[off++] = w.at(a);
      tw[off++] = w.at(a + b);
      tw[Fft1024::TW_LEN + Fft1024::ct_off(p) + 2 * hi] = w.ct(a);
      tw[Fft1024::TW_LEN + Fft1024::ct_off(p) + 2 * hi + 1] = w.ct(b);
    }
  return tw;
}

// ---- exact twiddles of the double-double key transforms (key_spectra.hpp) ----
// exp(i pi h / 2n) in double-double: quadrant and complement reduction on the integer h, then
// Taylor series of sin / cos on [0, pi/4] (terms below 2^-110 dropped): accurate to a few 2^-104.
inline DD dd_div_d(DD a, double b) {
  const double q1 = a.hi / b, p = q1 * b, pe = std::fma(q1, b, -p);
  return dd_quick(q1, ((a.hi - p) - pe + a.lo) / b);
}
inline void dd_sincos(DD x, DD &sn, DD &cs) {  // 0 <= x <= pi / 4
  const DD x2 = dd_mul(x, x);
  DD ts = x, tc = {1.0, 0.0};
  sn = x;
  cs = tc;
  for (int k = 1; k < 20; ++k) {
    ts = dd_div_d(dd_mul(ts, x2), (double)((2 * k) * (2 * k + 1)));
    tc = dd_div_d(dd_mul(tc, x2), (double)((2 * k - 1) * (2 * k)));
    sn = dd_add(sn, k & 1 ? dd_neg(ts) : ts);
    cs = dd_add(cs, k & 1 ? dd_neg(tc) : tc);
  }
}
inline CDD dd_expi(long h, long n) {
  const DD PI = {3.141592653589793116, 1.2246467991473532e-16};
  const long r = ((h % (4 * n)) + 4 * n) % (4 * n);  // angle pi r / 2n, period 4n
  const long quad = r / n, rho = r % n;               // quad * pi/2 + pi rho / 2n
  const bool comp = 2 * rho > n;                      // beyond pi/4: use the complement
  const long m = comp ? n - rho : rho;
  DD sn, cs;
  dd_sincos(dd_mul(PI, DD{(double)m / (2.0 * (double)n), 0.0}), sn, cs);
  DD c = comp ? sn : cs, s = comp ? cs : sn;  // cos, sin of pi rho / 2n
  for (long q = 0; q < quad; ++q) {             // rotate by pi/2: (c, s) -> (-s, c)
    const DD t = c;
    c = dd_neg(s);
    s = t;
  }
  return {c, s};
}
// tree twiddles W(s, i) = w^(eps(s, i) / 2), stage s node i at (1 << s) - 1 + i (dd_tree_fft)
inline std::vector<CDD> dd_tree_twiddles(int L) {
  std::vector<CDD> tw;
  for (const auto &stage : eps_tree(L))
    for (long h : stage) tw.push_back(dd_expi(h, 1L << L));
  return tw;
}

// CmuxNtt's copy of the level-2 twiddles: the stage-9/10 twiddles at their lane-contiguous positions.
inline std::vector<double> cmux_twiddles(const std::vector<double> &tw2) {
  std::vector<double> tw2c(tw2);
  for (int st = 9; st <= 10; ++st)
    for (int t = 0; t < CmuxNtt::T; ++t)
      for (int e = 0; e < CmuxNtt::E; ++e)
        if (!(e & (st == 9 ? 4 : 2)))
          tw2c[(1 << st) + cmux_tw_off(3, st, t, e)] = tw2[(1 << st) + (cmux_idx(3, t, e) >> (11 - st))];
  return tw2c;
}

// Trace tables [2][TRACE_STEPS][N2]: for step k (g = N2 / 2^k + 1), first the coefficient-domain
// source of sigma_g (position e holds coefficient i, + N2 when it is negated), then the NTT-domain
// permutation (the value at t comes from t' with eps(t') = g eps(t)).
inline std::vector<uint16_t> trace_tables() {
  std::vector<uint16_t> ttab(2 * TRACE_STEPS * N2);
  for (int k = 0; k < TRACE_STEPS; ++k) {
    const uint32_t g = (uint32_t)(N2 >> k) + 1;
    for (int i = 0; i < N2; ++i) {  // sigma_g: coefficient i -> position i*g mod 2N
      const uint32_t e = (uint32_t)(((uint64_t)i * g) % (2 * N2));
      if (e < (uint32_t)N2) ttab[k * N2 + e] = (uint16_t)i;
      else ttab[k * N2 + (e - N2)] = (uint16_t)(i + N2);
    }
    for (int t = 0; t < N2; ++t) {  // NTT domain: value at t comes from t' with eps(t') = g*eps(t)
      const uint32_t eps = 2 * bitrev((uint32_t)t, 11) + 1;
      const uint32_t e2 = (uint32_t)(((uint64_t)eps * g) % (2 * N2));
      ttab[(TRACE_STEPS + k) * N2 + t] = (uint16_t)bitrev((e2 - 1) / 2, 11);
    }
  }
  return ttab;
}

// A priori bound on |computed - exact| of every rounded coefficient of one external product
// (DESIGN.md §3a). For one CMUX step and one output spectrum, with n complex points, D =
// sqrt(2n) d_max the 2-norm bound of a digit polynomial, kappa_r the largest |K^| of GGSW row r
// (row_max_abs_kernel), the rows accumulated in the order r(0), r(1), ... by two fmas each:
//   E = n D (1 + 2^-30) [(delta_fwd + delta_inv + u (1 + 2^-40)) sum_r kappa_r + sqrt(2) u sum_k (2R - 2k) kappa_r(k)]
// the forward digit transforms within delta_fwd and the inverse within delta_inv relative 2-norm
// error (forward in tangent form, 4u per radix-2 stage: level 1 37u (9 stages), level 2 41u (10);
// inverse: level 1 32u -- 8u per premultiplied radix-8 pass, 5u per Gentleman-Sande stage of P1 and
// P3 --, level 2 26u -- 5u per premultiplied radix-4 pass --, rounded up), the sequential fma accumulation, and
// the double-double keys' |K^ - K| <= u |K|. The maximum over every step and output spectrum.
// kmax: [steps][rows][outputs] (level 1: [512][8][2]; level 2: [670][12][2 out][2 limb], the limbs
// as two more "outputs"). Level 3: level 2 as br2y_kernel (the latency path) accumulates it: each
// 256-thread group chains its three rows (its j-th at weight 2 (3 - j)), then two additions (the
// two groups' partials, the partner workgroup's) add 1 each: weight 8 - 2 j for digit 3 g + j.
// Level 4: the fused FFT trace (br2f_trace): 11 steps, 25 rows (digits |d| <= 3) accumulated in
// order, the trace key's rows [11 * 25][2 out][2 limb] as kmax.
inline double apriori_bound(int level, const std::vector<double> &kmax) {
  const double u = 0x1p-53;
  const bool y = level == 3, tr = level == 4;
  if (y || tr) level = 2;
  const int n = level == 1 ? 512 : 1024, R = level == 1 ? 2 * D1 : tr ? DT : 2 * D2, O = level == 1 ? 2 : 4;
  const int steps = level == 1 ? N0 : tr ? TRACE_STEPS : NI;
  // accumulation order of the kernels' MAC: br1f / br1l rows 0..7; br2f digits in issue order
  // g = 2 j + w, row p D2 + j + 3 w (br2_fft.hpp)
  const int order2[12] = {0, 3, 1, 4, 2, 5, 6, 9, 7, 10, 8, 11};
  // largest digit: level 1 16, level 2 64, the trace's balanced base-4 digits 2 (the top one 3)
  const double D = std::sqrt(2.0 * n) * (level == 1 ? 16.0 : tr ? 3.0 : 64.0);
  const double dft = level == 1 ? 37 + 32 : 41 + 26;  // delta_fwd + delta_inv, in units of u
  const double cf = dft * u + u * (1 + 0x1p-40), cw = std::sqrt(2.0) * u;
  double worst = 0.0;
  for (int i = 0; i < steps; ++i)
    for (int o = 0; o < O; ++o) {
      double s = 0.0, w = 0.0;
      for (int k = 0; k < R; ++k) {
        const int r = level == 1 || tr ? k : order2[k];
        const double kap = kmax[((size_t)i * R + r) * O + o];
        s += kap;
        w += (y ? 8.0 - 2.0 * ((r % D2) % 3) : 2.0 * R - 2.0 * k) * kap;
      }
      worst = std::max(worst, cf * s + cw * w);
    }
  return (double)n * D * worst * (1 + 0x1p-30);
}

}  // namespace omr
