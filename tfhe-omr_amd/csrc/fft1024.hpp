// Fft1024, the 1,024-point complex transform of level 2 (layouts and passes: the header comment of
// br2_fft.hpp), and the 25-bit limb split of its keys. A header of its own because the key conversion
// (key_spectra.hpp) and the host tables (host_tables.hpp) need it without br2_fft.hpp's kernels.
#pragma once

#include "device_fft.hpp"

namespace omr {

struct Fft1024 {
  static constexpr int T = 256, E = 4, n = 1024, L = 10;
  static constexpr int TW_LEN = 3 * (4 + 16 + 64 + 256);  // passes 1..4: (B, A, AB) per block (inverse)
  OMR_HD static constexpr int tw_off(int p) { return p == 1 ? 0 : p == 2 ? 12 : p == 3 ? 60 : 252; }
  // the forward passes' tangent forms (cos, tan) of (A, B) per block follow in the global table:
  // TW_LEN + ct_off(p) + 2 b + k (k: 0 A, 1 B); each thread holds its four blocks' in registers
  static constexpr int CT_LEN = 2 * (4 + 16 + 64 + 256);
  OMR_HD static constexpr int ct_off(int p) { return p == 1 ? 0 : p == 2 ? 8 : p == 3 ? 40 : 168; }

  // index bit of each position bit (e1, e0, l5, l4, l3, l2, l1, l0, w1, w0), per pass layout
  OMR_HD static constexpr int lay(int p, int k) {
    constexpr int tab[5][10] = {{9, 8, 7, 6, 3, 2, 1, 0, 5, 4},
                                {7, 6, 9, 8, 3, 2, 1, 0, 5, 4},
                                {5, 4, 3, 2, 1, 0, 9, 8, 7, 6},
                                {3, 2, 5, 4, 1, 0, 9, 8, 7, 6},
                                {1, 0, 5, 4, 3, 2, 9, 8, 7, 6}};
    return tab[p][k];
  }
  // point index held by register e of thread t in pass layout p
  OMR_HD static constexpr int idx(int p, int t, int e) {
    const int pos[10] = {(e >> 1) & 1, e & 1, (t >> 5) & 1, (t >> 4) & 1, (t >> 3) & 1, (t >> 2) & 1,
                         (t >> 1) & 1, t & 1, (t >> 7) & 1, (t >> 6) & 1};
    int j = 0;
    for (int k = 0; k < 10; ++k) j |= pos[k] << lay(p, k);
    return j;
  }
  OMR_HD static constexpr int bit(int j, int b) { return (j >> b) & 1; }
  // exchange swizzles: slot bits s0..s9 as XORs of index bits (tests/fft2_model.py SWIZZLES)
  OMR_HD static constexpr int slot_xf(int j) {  // P1 -> P2
    return bit(j, 0) | bit(j, 1) << 1 | (bit(j, 2) ^ bit(j, 8)) << 2 | bit(j, 9) << 3 | bit(j, 8) << 4 |
           bit(j, 3) << 5 | ((j >> 4) & 15) << 6;
  }
  OMR_HD static constexpr int slot_xi(int j) {  // P2 -> P1
    return bit(j, 0) | (bit(j, 1) ^ bit(j, 8)) << 1 | (bit(j, 2) ^ bit(j, 9)) << 2 | bit(j, 3) << 3 |
           bit(j, 8) << 4 | bit(j, 9) << 5 | ((j >> 4) & 15) << 6;
  }
  OMR_HD static constexpr int slot_wf(int j) {  // P3 -> P4 (wave bits j7 j6 -> slot bits 9 8)
    return bit(j, 8) | bit(j, 9) << 1 | (bit(j, 2) ^ bit(j, 0)) << 2 | bit(j, 3) << 3 | bit(j, 0) << 4 |
           bit(j, 1) << 5 | ((j >> 4) & 15) << 6;
  }
  OMR_HD static constexpr int slot_wi(int j) {  // P4 -> P3
    return bit(j, 8) | bit(j, 9) << 1 | (bit(j, 2) ^ bit(j, 0)) << 2 | bit(j, 1) << 3 | bit(j, 0) << 4 |
           bit(j, 3) << 5 | ((j >> 4) & 15) << 6;
  }
  // rotation staging of 2048 real coefficients (doubles): conflict-free ds_write_b64 / ds_read_b64
  OMR_HD static constexpr int slot_stage(int c) { return c ^ (((c >> 6) & 1) << 4); }

  // pass-0 twiddles (block 0): B = w^256 = e^{i pi / 8}, A = w^512 = e^{i pi / 4}, AB = e^{3 i pi / 8};
  // tangent forms A = R2 (1 + i), B = C8 (1 + i T8)
  static constexpr double C8 = 0.92387953251128675613, S8 = 0.38268343236508977173, R2 = 0.70710678118654752440;
  static constexpr double T8 = 0.41421356237309504880;  // tan(pi / 8) = sqrt 2 - 1

  __device__ static __forceinline__ void cmulc(double &xr, double &xi, double wr, double wi) {  // * conj(w)
    const double r = __fma_rn(xr, wr, xi * wi);
    const double i = __fma_rn(xi, wr, -xr * wi);
    xr = r;
    xi = i;
  }
  // adjoint network of "x *= T = (1, B, A, AB), then (a0 + a1, a0 - a1, b0 + i b1, b0 - i b1)"
  // (4 x its inverse): y0 = a0 + b0, y1 = a1 + b1, y2 = a0 - b0, y3 = a1 - b1
  __device__ static __forceinline__ void inet4(double (&xr)[E], double (&xi)[E]) {
    const double a0r = xr[0] + xr[1], a0i = xi[0] + xi[1], a1r = xr[0] - xr[1], a1i = xi[0] - xi[1];
    const double b0r = xr[2] + xr[3], b0i = xi[2] + xi[3];
    const double b1r = xi[2] - xi[3], b1i = xr[3] - xr[2];  // -i (o2 - o3)
    xr[0] = a0r + b0r;
    xi[0] = a0i + b0i;
    xr[2] = a0r - b0r;
    xi[2] = a0i - b0i;
    xr[1] = a1r + b1r;
    xi[1] = a1i + b1i;
    xr[3] = a1r - b1r;
    xi[3] = a1i - b1i;
  }
  template <int P>
  __device__ static __forceinline__ int block(int t) {
    return idx(P, t, 0) >> (L - 2 * P);
  }
  // LDS slot of twiddle k (0 B, 1 A, 2 AB) of block b in pass P. The global table (host order) is
  // tw_off(P) + 3 b + k, whose ds_read_b128 reads conflict 4-way in passes 3 and 4; there each k
  // has its own array with the block XOR-swizzled, conflict-free (tests/test_fft2_layout.py::
  // test_twiddle_read_cycles; level 2 0.8 % faster, profiles/r03q/twiddle_soa_ab.log).
  OMR_HD static constexpr int tw_slot(int P, int b, int k) {
    return P == 3 ? tw_off(3) + k * 64 + (b ^ (((b >> 4) & 3) << 1))
         : P == 4 ? tw_off(4) + k * 256 + (b ^ (((b >> 6) & 3) << 2))
                  : tw_off(P) + 3 * b + k;
  }
  // the global table (host order) into LDS slots
  __device__ static __forceinline__ void load_twiddles(double2 *tws, const double2 *__restrict__ twg, int t) {
    for (int j = t; j < TW_LEN; j += T) {
      const int P = j < tw_off(2) ? 1 : j < tw_off(3) ? 2 : j < tw_off(4) ? 3 : 4;
      const int r = j - tw_off(P);
      tws[tw_slot(P, r / 3, r % 3)] = twg[j];
    }
  }
  template <int P>
  __device__ static __forceinline__ void inv_pass(double (&xr)[E], double (&xi)[E], const double2 *tws, int t) {
    inet4(xr, xi);
    if constexpr (P == 0) {
      cmulc(xr[1], xi[1], C8, S8);
      cmulc(xr[2], xi[2], R2, R2);
      cmulc(xr[3], xi[3], S8, C8);
    } else {
      const int b = block<P>(t);
      const double2 B = tws[tw_slot(P, b, 0)], A = tws[tw_slot(P, b, 1)], AB = tws[tw_slot(P, b, 2)];
      cmulc(xr[1], xi[1], B.x, B.y);
      cmulc(xr[2], xi[2], A.x, A.y);
      cmulc(xr[3], xi[3], AB.x, AB.y);
    }
  }
  // inv_pass with the pass's (B, A, AB) already loaded (w)
  __device__ static __forceinline__ void inv_pass_w(double (&xr)[E], double (&xi)[E], const double2 (&w)[3]) {
    inet4(xr, xi);
    cmulc(xr[1], xi[1], w[0].x, w[0].y);
    cmulc(xr[2], xi[2], w[1].x, w[1].y);
    cmulc(xr[3], xi[3], w[2].x, w[2].y);
  }
  template <int P>
  __device__ static __forceinline__ void inv_tw(double2 (&w)[3], const double2 *tws, int t) {
    const int b = block<P>(t);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = tws[tw_slot(P, b, k)];
  }
  // P0 <-> P1 and P2 <-> P3 (an involution): register bit 1 <-> lane bit 5, register bit 0 <-> lane bit 4
  __device__ static __forceinline__ void perm(double (&xr)[E], double (&xi)[E]) {
    swap_lane_bit<5>(xr[0], xr[2]);
    swap_lane_bit<5>(xi[0], xi[2]);
    swap_lane_bit<5>(xr[1], xr[3]);
    swap_lane_bit<5>(xi[1], xi[3]);
    swap_lane_bit<4>(xr[0], xr[1]);
    swap_lane_bit<4>(xi[0], xi[1]);
    swap_lane_bit<4>(xr[2], xr[3]);
    swap_lane_bit<4>(xi[2], xi[3]);
  }
  OMR_HD static constexpr int swz(int S, int j) {
    return S == 0 ? slot_xf(j) : S == 1 ? slot_xi(j) : S == 2 ? slot_wf(j) : slot_wi(j);
  }
  // Slot of register e of thread t in layout P under swizzle S, as base(t) ^ xk(e) + ak(e): the
  // swizzles and layouts are linear over GF(2), so slot = swz(idx(P, t, 0)) ^ swz(idx(P, 0, e));
  // the bits of the second term that base(t) never sets are added as an immediate offset, the
  // rest (at most one distinct value here) is one XOR: two address registers per side.
  OMR_HD static constexpr int base_mask(int S, int P) {
    int m = 0;
    for (int t = 0; t < T; ++t) m |= swz(S, idx(P, t, 0));
    return m;
  }
  template <int S, int P>
  __device__ static __forceinline__ int slot_of(int base, int e) {
    constexpr int M0 = base_mask(S, P);
    const int k = swz(S, idx(P, 0, e));
    return (k & M0 ? base ^ (k & M0) : base) + (k & ~M0);
  }
  // LDS exchange PF -> PT through buf (1024 double2) with swizzle S; CROSS: workgroup barrier
  // between the writes and the reads (a cross-wave exchange), else wave-level ordering
  template <int PF, int PT, int S, bool CROSS>
  __device__ static __forceinline__ void exchange(double (&xr)[E], double (&xi)[E], double2 *buf, int t) {
    const int bw = swz(S, idx(PF, t, 0)), br = swz(S, idx(PT, t, 0));
#pragma unroll
    for (int e = 0; e < E; ++e) buf[slot_of<S, PF>(bw, e)] = make_double2(xr[e], xi[e]);
    if constexpr (CROSS)
      wg_barrier_lds();  // global loads (the next key blocks) stay in flight
    else
      wave_lds_sync();
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double2 v = buf[slot_of<S, PT>(br, e)];
      xr[e] = v.x;
      xi[e] = v.y;
    }
    wave_lds_fence();  // the next writes stay below these reads (in-order LDS per wave)
  }
  // forward radix-4 pass in tangent form (device_fft.hpp, bfly): the tree's stage A on the pairs
  // (0, 2), (1, 3), then B on (0, 1) and i B on (2, 3) -- the same map as "T = (1, B, A, AB), then
  // net4" in 24 FMAs instead of 28 operations
  __device__ static __forceinline__ void fwd_pass_t(double (&xr)[E], double (&xi)[E], double2 A, double2 B) {
    bfly<false>(xr[0], xi[0], xr[2], xi[2], A.x, A.y);
    bfly<false>(xr[1], xi[1], xr[3], xi[3], A.x, A.y);
    bfly<false>(xr[0], xi[0], xr[1], xi[1], B.x, B.y);
    bfly<true>(xr[2], xi[2], xr[3], xi[3], B.x, B.y);
  }
  // thread t's (A, B) tangent forms of pass P from the global table (its block is the same for all
  // four registers and all transforms)
  template <int P>
  __device__ static __forceinline__ void block_ct(double2 (&w)[2], const double2 *__restrict__ twg, int t) {
    const int b = block<P>(t);
#pragma unroll
    for (int k = 0; k < 2; ++k) w[k] = twg[TW_LEN + ct_off(P) + 2 * b + k];
  }
  // thread t's forward twiddles of passes 1..4 (wc[P - 1]), for every transform it runs
  __device__ static __forceinline__ void load_ct(double2 (&wc)[4][2], const double2 *__restrict__ twg, int t) {
    block_ct<1>(wc[0], twg, t);
    block_ct<2>(wc[1], twg, t);
    block_ct<3>(wc[2], twg, t);
    block_ct<4>(wc[3], twg, t);
  }
  // forward: in P0 layout (point idx(0, t, e)), out P4 layout. X: this transform's cross-wave buffer;
  // the wave-local exchange (P3 -> P4) runs in the wave's own quarter of X (slot bits 9, 8 = wave:
  // tests/test_fft2_layout.py::test_exchange_regions), which after this transform's cross-wave reads
  // no other wave touches until the next-but-one transform writes X behind the next barrier. Every
  // pass in tangent form on the thread's (A, B) held in registers (wc[P - 1]: block_ct<P>).
  struct NoMid {
    __device__ void operator()() const {}
  };
  // mid(): called after the cross-wave exchange (br2f_digit issues key loads there)
  template <typename Mid = NoMid>
  __device__ static __forceinline__ void fwd(double (&xr)[E], double (&xi)[E], double2 *X, int t,
                                             const double2 (&wc)[4][2], Mid mid = Mid()) {
    fwd_pass_t(xr, xi, make_double2(R2, 1.0), make_double2(C8, T8));
    perm(xr, xi);
    fwd_pass_t(xr, xi, wc[0][0], wc[0][1]);
    exchange<1, 2, 0, true>(xr, xi, X, t);
    mid();
    fwd_pass_t(xr, xi, wc[1][0], wc[1][1]);
    perm(xr, xi);
    fwd_pass_t(xr, xi, wc[2][0], wc[2][1]);
    exchange<3, 4, 2, false>(xr, xi, X, t);
    fwd_pass_t(xr, xi, wc[3][0], wc[3][1]);
  }
  // unscaled inverse (x 1024; the keys carry 1/1024): in P4 layout, out P0 layout; the wave-local
  // exchange first, in the wave's own quarter of X (which the previous use of X, two cross-wave
  // uses back, has finished with behind the last barrier), then the cross-wave one (own-quarter
  // writes)
  // Each pass's (B, A, AB) is requested one pass ahead, before the previous pass's arithmetic (round 6:
  // level 2 -0.4 %, profiles/r06f/ab.log), so its LDS round trip is off the pass's critical path.
  __device__ static __forceinline__ void inv(double (&xr)[E], double (&xi)[E], double2 *X, const double2 *tws, int t) {
    double2 w4[3], w3[3], w2[3], w1[3];
    inv_tw<4>(w4, tws, t);
    inv_tw<3>(w3, tws, t);
    inv_pass_w(xr, xi, w4);
    exchange<4, 3, 3, false>(xr, xi, X, t);
    inv_tw<2>(w2, tws, t);
    inv_pass_w(xr, xi, w3);
    perm(xr, xi);
    inv_tw<1>(w1, tws, t);
    inv_pass_w(xr, xi, w2);
    exchange<2, 1, 1, true>(xr, xi, X, t);
    __builtin_amdgcn_s_setprio(2);  // raised past the cross-wave barrier, as in br2f_digit
    inv_pass_w(xr, xi, w1);
    perm(xr, xi);
    inv_pass<0>(xr, xi, tws, t);
    __builtin_amdgcn_s_setprio(0);
  }
};

constexpr double LIMB = 33554432.0;  // 2^25: key = lo + 2^25 hi

}  // namespace omr
