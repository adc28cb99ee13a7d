// Level-2 blind rotation on the exact complex FFT (second_level_bootstrapping, detector.rs:599-624).
//
// The external product only multiplies gadget digits (|d| <= 64) by key residues, so with the
// key split into two 25-bit limbs, k = k_lo + 2^25 k_hi (|k_lo|, |k_hi| <= 2^24), every coefficient
// of sum_r d_r * k_r,limb over the 12 GGSW rows is an integer below 12 * 2048 * 64 * 2^24 < 2^44.6,
// and an FP64 FFT product rounds to it exactly (tests/fft2_model.py: worst error ~1e-2 with
// adversarial digits; tests/test_fft2_layout.py). The limb products are recombined mod q2 as
// red(P_hi * 2^25) + P_lo (2^25 P_hi is an exact double). Same digits and rows as the NTT kernels,
// so the output is bit-identical to them.
//
// Transform (Fft1024, fft1024.hpp): R[X]/(X^2048 + 1) -> C[X]/(X^1024 - i), z_j = p_j + i p_{j+1024}; 1,024
// complex points on 256 threads x 4 registers, five radix-4 passes of the twiddle tree of
// device_fft.hpp (n = 1024). Index bits j9..j0, pass P holds bits (9 - 2P, 8 - 2P) in registers
// e = (e1, e0); layouts (position bits e1 e0 | lane l5..l0 | wave w1 w0 -> index bits):
//   P0: 9 8 | 7 6 3 2 1 0 | 5 4    (input: coefficient pairs (j, j + 1024) of point j)
//   P1: 7 6 | 9 8 3 2 1 0 | 5 4    P0 -> P1: register bits 1, 0 <-> lane bits 5, 4 (permlane swaps)
//   P2: 5 4 | 3 2 1 0 9 8 | 7 6    P1 -> P2: cross-wave LDS exchange (X0 / X1)
//   P3: 3 2 | 5 4 1 0 9 8 | 7 6    P2 -> P3: permlane swaps
//   P4: 1 0 | 5 4 3 2 9 8 | 7 6    P3 -> P4: wave-local LDS exchange (W); the multiply-accumulate
//                                  layout: thread t holds points 4t..4t+3 of the key's storage order
// Each exchange has its own XOR swizzle, conflict-free for the ds_write_b128 8-lane and
// ds_read_b128 16-lane groups in its direction (tests/test_fft2_layout.py models the banks).
// Per CMUX step: 12 forward transforms, 48 complex multiply-accumulates per point, 4 inverse
// transforms (2 outputs x 2 limbs) instead of the NTT kernel's 12 + 2 modular transforms.
#pragma once

#include "exactness.hpp"
#include "fft1024.hpp"
#include "handoff.hpp"
#include "level2_common.hpp"

namespace omr {

// Storage position of point 4 t + e (P4 layout: thread t's register e) within a key block:
// register-major, so that each of a thread's four loads per block is one 1 KB-contiguous wave
// instruction (16 B per lane). The point-major order (4 t + e: 64 B per thread, 16 B per lane at a
// 64 B stride per instruction) ran level 2 8.7 % slower: 667 vs 609 ms per 16,384 messages
// (profiles/r03q/key_layout_ab.log).
__device__ __forceinline__ int key_pos(int t, int e) { return e * Fft1024::T + t; }

// BSK2 rows (canonical u64 [670][12][2][2048]) -> FFT-domain limbs, x 1/1024, as double2
// [670][12][2 out][2 limb][1024], point idx(4, t, e) at key_pos(t, e): key_spectrum_dd_kernel<2>
// (key_spectra.hpp), in double-double.

// Level-2 digit words for br2f: the Digits2 decomposition (NonPowOf2ApproxSignedBasis logB 7,
// d 6, drop 8) with every field a two's-complement digit, so that each digit is one v_bfe_i32
// (Digits2's biased fields need a v_bfe_u32 and a subtraction of 64). Digits 0..4 are biased by 64
// as in Digits2 (so the words have no borrows) and each 7-bit field is then XORed with 64
// ((f - 64) mod 128 = f ^ 64); the top digit d5 is left unbiased, so y >> 21 holds it as a signed
// value in bits 14..29 (sign-extended by the extract; |y| < 2^42, so |d5| < 2^7).
// The words come out of the FP64 bit pattern (round 5): Y = y + 1.5 * 2^52 is exact and its low 51
// mantissa bits are y in two's complement, so lo = Y's low dword (fields 0..2 at bits 0..20; the
// bits above are never extracted) and hi = bits 21..52 of Y (one v_alignbit_b32): 3 FP64 + 3
// integer operations per word pair instead of 8 FP64-rate (two floors, two conversions) + 2.
struct Digits2S {
  static constexpr int DW = 2;
  static_assert(LOGB2 == 7 && D2 == 6 && DROP2 == 8, "closed form written for the level-2 basis");
  __device__ static __forceinline__ void pack(double v, uint32_t (&pk)[DW]) {
    // + 64 (1 + 128 + .. + 128^4) + 1.5 * 2^52, an exact double
    const double y = floor(__fma_rn(v, 1.0 / 256.0, 0.5)) + (17315143744.0 + 6755399441055744.0);
    const uint64_t b = __builtin_bit_cast(uint64_t, y);
    const uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
    pk[0] = lo ^ 0x102040u;                                   // fields 0, 1, 2
    pk[1] = __builtin_amdgcn_alignbit(hi, lo, 21) ^ 0x2040u;  // fields 3, 4; d5 in bits 14..29
  }
  static constexpr int TOP_WIDTH = 16;  // d5: bits 35..50 of Y
  // digit j + 3 h as a double (h: the word, a compile-time constant)
  template <int H>
  __device__ static __forceinline__ double digit(const uint32_t (&pk)[DW], int j) {
    return (double)(int)__builtin_amdgcn_sbfe(pk[H], 7 * j, H == 1 && j == 2 ? TOP_WIDTH : 7);
  }
};

// acc + lo + 2^25 hr, reduced to the exact centred representative mod q2 (acc canonical; lo, hr the
// rounded limb products, |lo|, |hr| < 2^46): x = acc + lo and 2^25 hr are exact, the quotient
// k = rint((2^25 hr + x) / q2) is within 2^-30 of the true one, so fma(-k, q2, 2^25 hr) is the exact
// integer r - x (|r| <= q2 / 2 + 2^21), and one red of r is exact (|r| <= q2 - 1): 12 FP64
// operations with the two limb roundings instead of 14 (red of the high product, then canon).
__device__ __forceinline__ double limb_acc(double acc, double lo, double hr) {
  using M = Mod<2>;
  const double x = acc + lo;
  const double hi = hr * LIMB;
  const double k = rint(__fma_rn(hr, LIMB * M::QINV, x * M::QINV));
  return canon_small<M>(__fma_rn(-k, M::Q, hi) + x);
}

// BSK2 (FFT form) through a buffer descriptor: each key load is buffer_load_dwordx4 with the
// thread's byte offset (t * 16) in voffset and the row / block / register offset in soffset, so a
// digit's 16 loads cost no VALU address arithmetic (64-bit VGPR address adds before).
constexpr int BR2_ROW = 4 * Fft1024::n;  // double2 per GGSW row: [2 out][2 limb][1024]
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bsk2_rsrc(const double2 *bskf) {
  constexpr uint32_t bytes = (uint32_t)((size_t)NI * 2 * D2 * BR2_ROW * sizeof(double2));
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double2 *>(bskf), 0, bytes, 0x00020000);
}
typedef unsigned br2_v4u __attribute__((ext_vector_type(4)));
// the block of output o, limb l of global row q: thread t's 4 points (key_pos(t, e) = e * 256 + t)
__device__ __forceinline__ void br2f_load_block(double2 (&k)[Fft1024::E], __amdgpu_buffer_rsrc_t rsrc, int q, int o,
                                                int l, uint32_t t16) {
#pragma unroll
  for (int e = 0; e < Fft1024::E; ++e) {
    const uint32_t soff = (uint32_t)q * (uint32_t)(BR2_ROW * sizeof(double2)) +
                          (uint32_t)(((o * 2 + l) * Fft1024::n + e * Fft1024::T) * sizeof(double2));
    k[e] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rsrc, t16, (int)soff, 0));
  }
}
// output o's two limb blocks
__device__ __forceinline__ void br2f_load_half(double2 (&k)[2][Fft1024::E], __amdgpu_buffer_rsrc_t rsrc, int q,
                                               int o, uint32_t t16) {
  br2f_load_block(k[0], rsrc, q, o, 0, t16);
  br2f_load_block(k[1], rsrc, q, o, 1, t16);
}
// A transformed digit (xr, xi) times one output's two limb blocks k, into that output's spectra
__device__ __forceinline__ void br2f_mac(const double (&xr)[Fft1024::E], const double (&xi)[Fft1024::E],
                                         const double2 (&k)[2][Fft1024::E], double (&sr)[2][Fft1024::E],
                                         double (&si)[2][Fft1024::E]) {
#pragma unroll
  for (int l = 0; l < 2; ++l)
#pragma unroll
    for (int e = 0; e < Fft1024::E; ++e) {
      const double2 kv = k[l][e];
      sr[l][e] = __fma_rn(xr[e], kv.x, __fma_rn(-xi[e], kv.y, sr[l][e]));
      si[l][e] = __fma_rn(xr[e], kv.y, __fma_rn(xi[e], kv.x, si[l][e]));
    }
}
__device__ __forceinline__ void br2f_zero(double (&sr)[2][2][Fft1024::E], double (&si)[2][2][Fft1024::E]) {
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int e = 0; e < Fft1024::E; ++e) sr[o][l][e] = si[o][l][e] = 0.0;
}

// Digit words of (X^a - 1) * ACC_p from the LDS-resident accumulator (acp: 2048 doubles at
// Fft1024::slot_stage positions): coefficient j and j + 1024 of the thread's P0 points, as the
// Digits2S words (the rotated entry with its negacyclic sign as one xor of bit 63).
__device__ __forceinline__ void br2f_digits(const double *acp, int a, int t,
                                            uint32_t (&pk)[2][Fft1024::E][Digits2S::DW]) {
  using F = Fft1024;
  using M = Mod<2>;
  constexpr int NN = N2;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < F::E; ++e) {
      const int c = F::idx(0, t, e) + F::n * h;
      const uint32_t u = (uint32_t)(c - a) & (2 * NN - 1);
      const double v = acp[F::slot_stage(u & (NN - 1))];
      const uint32_t vh = (uint32_t)(__builtin_bit_cast(uint64_t, v) >> 32) ^ ((u & NN) << (31 - 11));
      const double rot = __builtin_bit_cast(double, (__builtin_bit_cast(uint64_t, v) & 0xffffffffull) |
                                                        ((uint64_t)vh << 32));
      Digits2S::pack(canon_small<M>(rot - acp[F::slot_stage(c)]), pk[h][e]);
      // keep the words as integers (not the doubles they come from) across the digit loop
      asm volatile("" : "+v"(pk[h][e][0]), "+v"(pk[h][e][1]));
    }
}

// One digit of a CMUX step: forward transform of digit j + 3 w (W) of the poly whose words are pk,
// then the multiply-accumulate into the four (output, limb) spectra: output A with ka (loaded one
// digit ahead, in flight across the transform), output B with kb (limb 0 loaded mid-transform, limb 1
// after it, in flight across output A's multiply-accumulate); ka is reloaded for the next digit nx
// between the two. (A function, not a lambda: by-reference captures drop __restrict__ / address-space facts.)
template <int W>
__device__ __forceinline__ void br2f_digit(const uint32_t (&pk)[2][Fft1024::E][Digits2S::DW], int j, int q, int nx,
                                           double (&sr)[2][2][Fft1024::E], double (&si)[2][2][Fft1024::E],
                                           double2 (&ka)[2][Fft1024::E], double2 (&kb)[2][Fft1024::E], double2 *X,
                                           __amdgpu_buffer_rsrc_t rsrc, uint32_t t16, int t, const double2 (&wc)[4][2]) {
  using F = Fft1024;
  constexpr int E = F::E;
  double xr[E], xi[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    xr[e] = Digits2S::digit<W>(pk[0][e], j);
    xi[e] = Digits2S::digit<W>(pk[1][e], j);
  }
  // output B's limb-0 blocks issued mid-transform (after its cross-wave exchange: 1.3 % faster at
  // level 2 than after the transform; both limbs there spill and run 20-34 % slower,
  // profiles/r05zf/bench_variants.log), limb 1 after it, in flight across output A's products
  // Wave priority (s_setprio) raised from the transform's cross-wave barrier to the end of the
  // digit's multiply-accumulates, normal otherwise: of the two workgroups sharing each SIMD, the wave
  // past a barrier issues first, so a workgroup's four waves reach the next barrier closer together
  // (level 2 -3.7 %, stable over 8 alternating runs: profiles/r05zo/; the inverses the same way,
  // Fft1024::inv: profiles/r05zq/). Left raised past the digit
  // (through the inverses and the next digit words) it was as fast in most runs but bimodal, one run
  // in four 50 % slower at level 2 (profiles/r05zn/).
  constexpr int LE = 1;  // limbs issued mid-transform (this form is the measured schedule)
  F::fwd(xr, xi, X, t, wc, [&]() {
    __builtin_amdgcn_s_setprio(2);
#pragma unroll
    for (int l = 0; l < LE; ++l) br2f_load_block(kb[l], rsrc, q, 1, l, t16);
  });
#pragma unroll
  for (int l = LE; l < 2; ++l) br2f_load_block(kb[l], rsrc, q, 1, l, t16);
#pragma unroll
  for (int o = 0; o < 2; ++o) {  // (as a loop: two calls in a row spill 9 VGPRs here)
    br2f_mac(xr, xi, o ? kb : ka, sr[o], si[o]);
    if (o == 0) br2f_load_half(ka, rsrc, nx, 0, t16);
  }
  __builtin_amdgcn_s_setprio(0);
}

// Rounding to the exact limb products, recombination mod q2 and ACC_o += (in place in LDS): thread
// t owns coefficients idx(0, t, e) + 1024 h of ACC_o, which only it reads before the next step.
template <bool G>
__device__ __forceinline__ void br2f_update(double *aco, const double (&sr)[2][Fft1024::E],
                                           const double (&si)[2][Fft1024::E], RoundGuard<G> &rg, int t) {
  using F = Fft1024;
#pragma unroll
  for (int e = 0; e < F::E; ++e)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double ylo = h ? si[0][e] : sr[0][e], yhi = h ? si[1][e] : sr[1][e];
      const double lo = rint(ylo), hr = rint(yhi);
      rg.note(ylo, lo);
      rg.note(yhi, hr);
      double &a = aco[F::slot_stage(F::idx(0, t, e) + F::n * h)];
      a = limb_acc(a, lo, hr);
    }
}

// LDS of br2f_body and trace_fft_body, carved from one 80 KB pool (two workgroups per CU): X0, X1
// (the transforms' cross-wave buffers), ACC (mask, body at slot_stage positions), then the twiddles.
constexpr size_t BR2_LDS_X = 0, BR2_LDS_TWS = 4 * (size_t)Fft1024::n * sizeof(double2),
                 BR2_LDS_BYTES = BR2_LDS_TWS + (size_t)Fft1024::n * sizeof(double2);
struct Br2Lds {
  double2 *tws;
  double2 (*Xb)[Fft1024::n];  // X0, X1
  double *acs;
};
__device__ __forceinline__ Br2Lds br2_lds(double2 *pool) {
  double2 *x = pool + BR2_LDS_X / sizeof(double2);
  return {pool + BR2_LDS_TWS / sizeof(double2), reinterpret_cast<double2(*)[Fft1024::n]>(x),
          reinterpret_cast<double *>(x + 2 * Fft1024::n)};
}

// hom_trace (detector.rs:626-639; secret.rs:167-168 for N^-1) on the exact FFT (round 5), in place on
// the LDS-resident accumulator (acs: mask, body at slot_stage positions, canonical): c *= N^-1, then
// for each of the 11 automorphisms sigma_g: c += KS_g(sigma_g(c)), where the key switch decomposes
// sigma_g(a) into 25 balanced base-4 digits (DigitsTrace) and multiply-accumulates them with the
// trace key's rows exactly as a CMUX step does with BSK2's: the same Fft1024 transforms, the key as
// two 25-bit limbs (tkf: [11 * 25 rows][2 out][2 limb][1024], x 1/1024, row q = 11 k + d ... in
// the order k * 25 + d), the four inverses rounded to the exact limb products and recombined mod q2
// (limb_acc). Both halves stay in the coefficient domain, where sigma_g is the signed permutation
// trace_src; A goes to the mask, sigma_g(b) + B to the body. Each digit's products are below
// 2 * 2^24 * 2048 * 25 < 2^42 (|d| <= 2 for 24 of them, 3 for the top one), so the a priori bound
// of this accumulation (apriori_bound level 4) is far below level 2's; the host falls back to the
// NTT trace when it is not below 0.5. 25 transforms of 120 FP64 operations per thread and step
// instead of 25 modular NTTs of ~450.
template <bool G>
__device__ __forceinline__ void br2f_trace(const Br2Lds &lds, const double2 *__restrict__ tkf,
                                           const double2 *__restrict__ twg, const DeviceTables &tb,
                                           RoundGuard<G> &rg, int t) {
  using F = Fft1024;
  using M = Mod<2>;
  constexpr int E = F::E, NN = N2;
  double *acs = lds.acs;
  double2(*Xb)[F::n] = lds.Xb;
  const double2 *tws = lds.tws;
  double2 wc[4][2];  // the forward twiddles again (not kept live across the rotation)
  F::load_ct(wc, twg, t);
  static_assert(DT == 25 && TRACE_STEPS == 11, "trace geometry");
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        double &x = acs[p * NN + F::slot_stage(F::idx(0, t, e) + F::n * h)];
        x = canon<M>(mm<M>(x, NINV2));
      }
  constexpr uint32_t bytes = (uint32_t)((size_t)TRACE_STEPS * DT * BR2_ROW * sizeof(double2));
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<double2 *>(tkf), 0, bytes, 0x00020000);
  const uint32_t t16 = (uint32_t)t * 16u;
#pragma unroll 1
  for (int k = 0; k < TRACE_STEPS; ++k) {
    const uint16_t *src = tb.trace_src + k * NN;
    double2 ka[2][E], kb[2][E];
    br2f_load_half(ka, rsrc, k * DT, 0, t16);
    __syncthreads();  // the previous update (or the scaling) visible
    uint32_t pk[2][E][DigitsTrace::DW];  // sigma_g(a) at the thread's P0 points (coefficients j, j + 1024)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int sidx = src[F::idx(0, t, e) + F::n * h];
        const double v = sidx < NN ? acs[F::slot_stage(sidx)] : -acs[F::slot_stage(sidx - NN)];
        DigitsTrace::pack(v, pk[h][e]);
        asm volatile("" : "+v"(pk[h][e][0]), "+v"(pk[h][e][1]));
      }
    double sr[2][2][E], si[2][2][E];  // [output A / B][limb]
    br2f_zero(sr, si);
#pragma unroll 1
    for (int d = 0; d < DT; ++d) {
      const int q = k * DT + d;
      double xr[E], xi[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        xr[e] = DigitsTrace::get(pk[0][e], d);
        xi[e] = DigitsTrace::get(pk[1][e], d);
      }
      // output B's limb-0 blocks mid-transform, limb 1 after it (as br2f_digit)
      F::fwd(xr, xi, Xb[d & 1], t, wc, [&]() { br2f_load_block(kb[0], rsrc, q, 1, 0, t16); });
      br2f_load_block(kb[1], rsrc, q, 1, 1, t16);
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        br2f_mac(xr, xi, o ? kb : ka, sr[o], si[o]);
        if (o == 0) br2f_load_half(ka, rsrc, d + 1 < DT ? q + 1 : q, 0, t16);
      }
    }
    // the four inverses on X0, X1, X0, X1 (the digits' last use of X1 was two uses back)
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int l = 0; l < 2; ++l) F::inv(sr[o][l], si[o][l], Xb[l], tws, t);
    double sb[2][E];  // sigma_g(b) at the thread's coefficients, read before any thread updates acs
    const uint16_t *srcb = src;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int sidx = srcb[F::idx(0, t, e) + F::n * h];
        sb[h][e] = sidx < NN ? acs[NN + F::slot_stage(sidx)] : -acs[NN + F::slot_stage(sidx - NN)];
      }
    __syncthreads();  // every thread has read sigma_g(a) and sigma_g(b)
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = F::slot_stage(F::idx(0, t, e) + F::n * h);
        const double alo = h ? si[0][0][e] : sr[0][0][e], ahi = h ? si[0][1][e] : sr[0][1][e];
        const double blo = h ? si[1][0][e] : sr[1][0][e], bhi = h ? si[1][1][e] : sr[1][1][e];
        const double ral = rint(alo), rah = rint(ahi), rbl = rint(blo), rbh = rint(bhi);
        rg.note(alo, ral);
        rg.note(ahi, rah);
        rg.note(blo, rbl);
        rg.note(bhi, rbh);
        acs[c] = limb_acc(acs[c], ral, rah);
        acs[NN + c] = limb_acc(acs[NN + c] + sb[h][e], rbl, rbh);
      }
  }
}

// Level-2 blind rotation (BlindRotationKey::blind_rotate, detector.rs:623) on the exact FFT: one
// 256-thread workgroup per message; output the coefficient-domain rotation (mode 1) or, after
// hom_trace (detector.rs:626-639), the NttRlweCiphertext (mode 0).
// The accumulator lives in LDS (ACC_p at slot_stage positions): each step reads the rotated digits
// of ACC_p straight from it and the update writes it in place, so there is no staging exchange and
// its 32 VGPRs hold the thread's forward twiddles instead (round 5: the tangent forms of passes
// 1..4, the inverse reading the premultiplied (B, A, AB) from LDS). Per CMUX step: for
// each of the 12 digits in issue order (poly p, digit j + 3 w) a forward transform and the
// multiply-accumulate into the four (output, limb) spectra with the key row (output A's blocks
// loaded one digit ahead); then the four inverses, rounding, limb recombination mod q2 and the
// update. Cross-wave uses alternate X0, X1 over the 12 digits and the 4 inverses, and every
// wave-local exchange runs in the wave's own quarter of the current X (Fft1024::fwd / inv), so each
// use rewrites a buffer whose readers have passed a later barrier: 17 workgroup barriers per step
// (one at the step start: the previous update visible to the rotated reads).
// LDS: twiddles 16 KB, X0 / X1 32 KB, ACC 32 KB (80 KB: two workgroups per CU).
// FROM (the test entries omr_blind_rotate_level2_from): the initial accumulator is acc0's message
// (canonical u64 [2][N2], the output's layout) instead; separate kernels, so that the production
// kernels' code does not move.
template <bool G, bool FROM = false>
__device__ __forceinline__ void br2f_body(const uint32_t *__restrict__ lwe_int, const double2 *__restrict__ bskf,
                                          const double2 *__restrict__ twg, DeviceTables tb, uint64_t *__restrict__ out,
                                          unsigned long long *margin, double2 *pool, size_t item,
                                          const uint64_t *__restrict__ acc0 = nullptr) {
  using F = Fft1024;
  using M = Mod<2>;
  constexpr int E = F::E, NN = N2;
  static_assert(F::TW_LEN <= F::n, "the twiddle table's LDS doubles as the trace's NTT table");
  const Br2Lds lds = br2_lds(pool);
  double2 *tws = lds.tws;
  double2(*Xb)[F::n] = lds.Xb;
  double *acs = lds.acs;
  const int t = threadIdx.x;
  const uint32_t *lwe = lwe_int + item * (NI + 1);
  F::load_twiddles(tws, twg, t);
  if constexpr (FROM) {  // ACC = the caller's
    const uint64_t *a0 = acc0 + item * 2 * NN;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int c = F::idx(0, t, e) + F::n * h;
        acs[F::slot_stage(c)] = from_u64<M>(a0[c]);
        acs[NN + F::slot_stage(c)] = from_u64<M>(a0[NN + c]);
      }
  } else {  // ACC = (0, X^{-b} * LUT2)
    const int b = (int)lwe[NI];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int c = F::idx(0, t, e) + F::n * h;
        acs[F::slot_stage(c)] = 0.0;
        acs[NN + F::slot_stage(c)] = acc2_init(tb.lut2, b, c);
      }
  }
  __syncthreads();
  double2 wc[4][2];  // this thread's forward twiddles of passes 1..4, for every transform of the rotation
  F::load_ct(wc, twg, t);
  double2 ka[2][E], kb[2][E];
  const __amdgpu_buffer_rsrc_t rsrc = bsk2_rsrc(bskf);
  const uint32_t t16 = (uint32_t)t * 16u;
  RoundGuard<G> rg;
  int kq = -1;  // the row whose output-A blocks ka already holds (the previous step's last digit loads them)
#pragma unroll 1
  for (int i = 0; i < NI; ++i) {
    const int a = (int)__builtin_amdgcn_readfirstlane(lwe[i]) & (2 * NN - 1);
    if (a == 0) continue;  // (X^0 - 1) * ACC = 0
    const int q0 = i * 2 * D2;  // the step's first global row
    if (kq != q0) br2f_load_half(ka, rsrc, q0, 0, t16);
    kq = i + 1 < NI ? q0 + 2 * D2 : -1;
    wg_barrier_lds();  // ACC (init or the previous update) visible; the previous inverses' reads done
    double sr[2][2][E], si[2][2][E];  // [output][limb] spectra
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      uint32_t pk[2][E][Digits2S::DW];  // [coefficient j / j + 1024][point] digit words
      br2f_digits(acs + p * NN, a, t, pk);
      // digits in issue order g = 2 j + w: digit j + 3 w sits in word w at field j, so the word is
      // chosen at compile time; its GGSW row is p D2 + j + 3 w. The next digit in issue order: after
      // (j, 0) comes (j, 1), after (j, 1) (j + 1, 0), after the mask's last digit the body's first,
      // after the body's last the next step's first row (in flight across the inverses; kq above;
      // the last step reloads its own row: harmless).
      auto nxt = [&](int j, int w) {
        return q0 + (w == 0 ? p * D2 + j + 3
                            : (j + 1 < D2 / 2 ? p * D2 + j + 1 : (p == 0 ? D2 : (kq >= 0 ? 2 * D2 : 2 * D2 - 1))));
      };
      if (p == 0) br2f_zero(sr, si);  // (peeling the step's first digit instead measured 10 % slower: 22 spills)
#pragma unroll 1
      for (int j = 0; j < D2 / 2; ++j) {
        br2f_digit<0>(pk, j, q0 + p * D2 + j, nxt(j, 0), sr, si, ka, kb, Xb[0], rsrc, t16, t, wc);
        br2f_digit<1>(pk, j, q0 + p * D2 + j + 3, nxt(j, 1), sr, si, ka, kb, Xb[1], rsrc, t16, t, wc);
      }
    }
    // inverses on X0, X1, X0, X1, rounding to the exact limb products, recombination mod q2
    // (pipelining them in barrier stages, the second half of one beside the first half of the next,
    // measured no faster: profiles/r05zd/bench_variants.log, var_kpi; nor reading the accumulator
    // entries ahead of each output's last inverse: profiles/r05zg/, var_upf)
#pragma unroll
    for (int o = 0; o < 2; ++o) {
#pragma unroll
      for (int l = 0; l < 2; ++l) F::inv(sr[o][l], si[o][l], Xb[l], tws, t);
      br2f_update<G>(acs + o * NN, sr[o], si[o], rg, t);
    }
  }
  rg.publish(margin);
  __syncthreads();  // the last updates everywhere
  uint64_t *o = out + item * 2 * NN;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int c = F::idx(0, t, e) + F::n * h;
        o[p * NN + c] = to_u64<M>(acs[p * NN + F::slot_stage(c)]);
      }
}

// The trace as its own launch on the FFT (trace_fft_kernel, round 5): in place on level 2's
// coefficient-domain output (canonical u64 [2][N2] per message) -> NttRlweCiphertext. br2f_body's
// LDS layout (X0, X1, ACC, twiddles: 80 KB, two workgroups per CU); br2f_trace, then both halves
// to the NTT domain. Its own launch, not fused into br2f_kernel: fused, the trace's live values
// pushed the rotation loop to 37-53 VGPR spills.
template <bool G>
__device__ __forceinline__ void trace_fft_body(uint64_t *__restrict__ io, const double2 *__restrict__ tkf,
                                               const double2 *__restrict__ twg, DeviceTables tb,
                                               unsigned long long *margin) {
  using F = Fft1024;
  using M = Mod<2>;
  constexpr int E = F::E, NN = N2;
  __shared__ double2 pool[BR2_LDS_BYTES / sizeof(double2)];
  const Br2Lds lds = br2_lds(pool);
  double2 *tws = lds.tws;
  double *acs = lds.acs;
  const int t = threadIdx.x;
  uint64_t *o = io + (size_t)blockIdx.x * 2 * NN;
  F::load_twiddles(tws, twg, t);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int c = F::idx(0, t, e) + F::n * h;
        acs[p * NN + F::slot_stage(c)] = from_u64<M>(o[p * NN + c]);
      }
  RoundGuard<G> rg;
  br2f_trace<G>(lds, tkf, twg, tb, rg, t);
  rg.publish(margin);
  __syncthreads();  // the last updates everywhere
  // to_ntt_rlwe: both halves to the NTT domain (the trace NTTs' coefficient layout t + 256 e)
  using NTT = WgNtt<M, BR2_T, BR2_E>;
  double ca[BR2_E], cb[BR2_E];
#pragma unroll
  for (int e = 0; e < BR2_E; ++e) {
    ca[e] = acs[F::slot_stage(t + e * BR2_T)];
    cb[e] = acs[NN + F::slot_stage(t + e * BR2_T)];
  }
  double *xch = reinterpret_cast<double *>(lds.Xb);  // 2 N2 doubles (below the accumulator)
  double *tw = reinterpret_cast<double *>(tws);           // N2 doubles
  static_assert(NTT::LDS_DOUBLES * sizeof(double) <= 2 * F::n * sizeof(double2), "NTT exchange below ACC");
#pragma unroll
  for (int e = 0; e < BR2_E; ++e) tw[t + e * BR2_T] = tb.tw2[t + e * BR2_T];
  __syncthreads();
  NTT::fwd(ca, xch, tw, t);
  NTT::fwd(cb, xch, tw, t);
#pragma unroll
  for (int e = 0; e < BR2_E; ++e) {
    const int j = t * BR2_E + e;
    o[j] = to_u64<M>(canon<M>(ca[e]));
    o[NN + j] = to_u64<M>(canon<M>(cb[e]));
  }
}
#ifndef OMR_LEVEL2_PARTS_ONLY  // the kernels: not in two_cu_from.hip (br2_ntt.hpp)
__global__ __launch_bounds__(256, 2) void trace_fft_kernel(uint64_t *__restrict__ io, const double2 *__restrict__ tkf,
                                                           const double2 *__restrict__ twg, DeviceTables tb) {
  trace_fft_body<false>(io, tkf, twg, tb, nullptr);
}
__global__ __launch_bounds__(256, 2) void trace_fft_guard_kernel(uint64_t *__restrict__ io,
                                                                 const double2 *__restrict__ tkf,
                                                                 const double2 *__restrict__ twg, DeviceTables tb,
                                                                 unsigned long long *margin) {
  trace_fft_body<true>(io, tkf, twg, tb, margin);
}

__global__ __launch_bounds__(256, 2) void br2f_kernel(const uint32_t *__restrict__ lwe_int,
                                                      const double2 *__restrict__ bskf,
                                                      const double2 *__restrict__ twg, DeviceTables tb,
                                                      uint64_t *__restrict__ out) {
  __shared__ double2 pool[BR2_LDS_BYTES / sizeof(double2)];
  br2f_body<false>(lwe_int, bskf, twg, tb, out, nullptr, pool, blockIdx.x);
}
__global__ __launch_bounds__(256, 2) void br2f_guard_kernel(const uint32_t *__restrict__ lwe_int,
                                                            const double2 *__restrict__ bskf,
                                                            const double2 *__restrict__ twg, DeviceTables tb,
                                                            uint64_t *__restrict__ out, unsigned long long *margin) {
  __shared__ double2 pool[BR2_LDS_BYTES / sizeof(double2)];
  br2f_body<true>(lwe_int, bskf, twg, tb, out, margin, pool, blockIdx.x);
}
__global__ __launch_bounds__(256, 2) void br2f_from_kernel(const uint32_t *__restrict__ lwe_int,
                                                           const double2 *__restrict__ bskf,
                                                           const double2 *__restrict__ twg, DeviceTables tb,
                                                           uint64_t *__restrict__ out,
                                                           const uint64_t *__restrict__ acc0) {
  __shared__ double2 pool[BR2_LDS_BYTES / sizeof(double2)];
  br2f_body<false, true>(lwe_int, bskf, twg, tb, out, nullptr, pool, blockIdx.x, acc0);
}
__global__ __launch_bounds__(256, 2) void br2f_guard_from_kernel(const uint32_t *__restrict__ lwe_int,
                                                                 const double2 *__restrict__ bskf,
                                                                 const double2 *__restrict__ twg, DeviceTables tb,
                                                                 uint64_t *__restrict__ out,
                                                                 unsigned long long *margin,
                                                                 const uint64_t *__restrict__ acc0) {
  __shared__ double2 pool[BR2_LDS_BYTES / sizeof(double2)];
  br2f_body<true, true>(lwe_int, bskf, twg, tb, out, margin, pool, blockIdx.x, acc0);
}
#endif  // OMR_LEVEL2_PARTS_ONLY


// ---- level 2 over two CUs per message on the exact FFT (the latency path) --------------------
// br2x_kernel's division of labour (br2_ntt.hpp) on br2f's arithmetic. Workgroup 2m + r
// owns polynomial r (0 mask, 1 body) of message m and its accumulator ACC_r (LDS, slot_stage
// positions). Its group g (256 threads: one Fft1024 transform) takes word g of the Digits2S
// decomposition of (X^a - 1) ACC_r -- digits 3g + j, GGSW rows r D2 + 3g + j -- and for each digit
// runs the forward transform and multiply-accumulates the four (output, limb) spectra. Group g
// finalises limb g of output r: the groups swap their limb-(1 - g) partials of both outputs through
// LDS; group g keeps limb g of output r and sends limb g of output 1 - r to the partner workgroup
// through global memory under br2x's hand-off rules (sc1 stores, vmcnt(0), a barrier, one flag
// carrying the executed-step count, a bounded poll, sc1 loads; slot = step parity); it adds the
// partner's limb g of output r, runs the inverse, rounds, and the groups swap half of the rounded
// limbs so that each recombines (mod q2) and updates 1,024 of ACC_r's coefficients. Per CU and
// step: three forward transforms per group, one inverse, one hand-off -- br2x's schedule, with
// transforms of 120 / 140 FP64 operations per thread instead of the modular NTT's ~450.
// Key rows: output A's two limb blocks of the next digit are issued after output A's MAC, output
// B's after output B's (in flight across the next transform); the next step's first row is issued
// once the partner's payload has been consumed, so no wait of the hand-off covers it and it stays
// in flight across the inverse, the update and the next step's digit extraction.
// Exact when the a priori bound of this accumulation order (apriori_bound level 3) is below 0.5;
// otherwise, or on a guarded context, the host runs br2x_kernel's exact NTT instead.
// LDS: twiddles 16 KB, X0 / X1 of each group 64 KB, the limb swap 32 KB (+ the groups' X1), ACC_r
// 16 KB: 128 KB, one workgroup per CU.
// Key prefetchers (round 5): a lone message's workgroup streams 384 KB of FFT-form key per step
// from HBM / the Infinity Cache at the per-CU rate of a few outstanding loads (~31 GB/s: 8.3 ms of
// level 2, against 6.1 ms with the key loads skipped, profiles/r05o/); from its XCD's L2 a CU reads
// ~118 GB/s (tools/microbench_l2.hip). So the launch carries BR2Y_H helper workgroups per worker
// on the worker's XCD (workgroups b and b + 8 share one: MI355X_MICROARCH.md, §Workgroup dispatch;
// a placement that differs costs speed, never correctness -- helpers only read the key): helper k
// touches one dword per 64 B of its quarter of the worker's rows of each executed step, at most
// BR2Y_PF executed steps ahead of the worker's hand-off count (its flag), so the rows are L2-resident
// when the worker loads them.
// Same-XCD hand-off (round 5): the hand-off cost 1.2 of br2y's 6.6 ms (profiles/r05t: its payload
// stores, poll and loads removed in a timing-only build) -- an sc1 store writes the line through and
// drops it from L2, so the partner's loads go beyond L2. Both workers of a message are therefore
// placed in one grid column (so on one XCD when the dispatcher deals blocks round-robin), each reads
// its XCD id (HW_REG_XCC_ID) and they swap it through global memory with sc1 accesses once per
// launch. When the ids agree, the payload and the flag are written with plain stores, which stay in
// that XCD's L2 where the partner's sc1 loads (L1 bypassed) find them; otherwise the sc1 protocol
// above runs unchanged. Either way every payload load is an sc1 load, so the choice follows the
// actual placement and changes speed only.
// Grid: w8 = n rounded up to a multiple of 8 columns (message m in column m); row 0 = the mask
// workers, row 1 = the body workers, rows 2 + 2k + r = helper k of worker (m, r); the host launches
// the helper rows only when every workgroup fits on its own CU. flags[2n .. 4n): the XCD ids + 1.
constexpr int BR2Y_T = 2 * Fft1024::T;
constexpr int BR2Y_H = 4, BR2Y_PF = 2;

__device__ __forceinline__ void br2y_prefetch(const uint32_t *__restrict__ lwe_int, const double2 *__restrict__ bskf,
                                              const uint32_t *flags, int wid, int k) {
  constexpr int STEP_LINES = D2 * BR2_ROW * (int)sizeof(double2) / 64;  // 64 B lines of one step's rows
  constexpr int PER_THREAD = STEP_LINES / (BR2Y_H * BR2Y_T);
  static_assert(PER_THREAD * BR2Y_H * BR2Y_T == STEP_LINES, "helpers split a step's rows evenly");
  __shared__ int go;
  const int m = wid >> 1, r = wid & 1;
  const uint32_t *lwe = lwe_int + (size_t)m * (NI + 1);
  uint32_t acc = 0;
  int e = 0;  // executed steps prefetched
#pragma unroll 1
  for (int i = 0; i < NI; ++i) {
    const int a = (int)__builtin_amdgcn_readfirstlane(lwe[i]) & (2 * N2 - 1);
    if (a == 0) continue;
    if (threadIdx.x == 0) {  // the worker has published hand-off e - BR2Y_PF (bounded: a helper may give up)
      int ok = 1, n = 0;
      while ((int)__hip_atomic_load(flags + wid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < e - BR2Y_PF) {
        if (++n == (1 << 16)) {
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      go = ok;
    }
    __syncthreads();
    if (!go) break;
    const char *rows = reinterpret_cast<const char *>(bskf + ((size_t)i * 2 * D2 + (size_t)r * D2) * BR2_ROW);
    uint32_t v[PER_THREAD];
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u)
      v[u] = *reinterpret_cast<const uint32_t *>(rows + (size_t)((u * BR2Y_H + k) * BR2Y_T + (int)threadIdx.x) * 64);
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) acc ^= v[u];
    __syncthreads();  // thread 0's next poll after every load of this step returned
    ++e;
  }
  asm volatile("" ::"v"(acc));  // the loads stay live
}

#ifndef OMR_LEVEL2_PARTS_ONLY
__global__ __launch_bounds__(BR2Y_T, 1) void br2y_kernel(const uint32_t *__restrict__ lwe_int,
                                                         const double2 *__restrict__ bskf,
                                                         const double2 *__restrict__ twg, DeviceTables tb,
                                                         double *xg, uint32_t *flags, int *err,
                                                         uint64_t *__restrict__ out, int nmsg, int w8,
                                                         int allow_fast) {
#define OMR_BR2Y_FROM 0
#include "br2y_kernel_body.inc"
#undef OMR_BR2Y_FROM
}
#endif  // OMR_LEVEL2_PARTS_ONLY

}  // namespace omr
