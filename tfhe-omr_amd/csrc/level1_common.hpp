// What every level-1 kernel family shares (br1_fft.hpp: the throughput FFT; br1_latency.hpp: the
// eight-wave FFT; br1_ntt.hpp: the exact modular NTT): the integer residue arithmetic and digit
// words, the accumulator layout, the LWE staging, the initial accumulator, the staged [ACC, -ACC]
// with its rotated read, the row product and a wave's output store.
#pragma once

#include "exactness.hpp"
#include "kernels.hpp"

namespace omr {

struct Lvl1Int {
  static constexpr int Q = 134215681, H = 67107840;
  __device__ static __forceinline__ int canon(int x) {  // |x| < q + H -> [-H, H]
    // unsigned min folds, no VCC (compare/select pairs serialise on VCC with hazard NOPs):
    // y = x + H in [-Q, 2Q); min(y, y + Q) lifts [-Q, 0) into [0, Q), min(y, y - Q) lowers
    // [Q, 2Q) into [0, Q) (the other operand wraps above 2^31 and loses)
    uint32_t y = (uint32_t)(x + H);
    y = min(y, y + (uint32_t)Q);
    y = min(y, y - (uint32_t)Q);
    return (int)y - H;
  }
  __device__ static __forceinline__ uint32_t to_u32(int x) { return (uint32_t)(x < 0 ? x + Q : x); }
  // y = an integer + e (|y| < 2^43, |e| < 0.1: an FFT product output): round(y) mod q in [0, q], as
  // a u32. The quotient is floor(y / q) (as computed: it may exceed the true floor only when y is
  // within 2^-37 q of a multiple of q, and then r rounds to 0; it may fall one short only when the
  // rounded result is q), r = y - kq keeps the fraction, and adding 1.5 * 2^52 rounds r to the
  // nearest integer in the low mantissa bits: one FP64 add instead of rint + conversion. The result
  // q (= 0 mod q) is allowed: Lvl1Off::add folds it. With a RoundGuard, |r - round(r)| =
  // |y - rint(y)| (r = y - kq is exact) is recorded.
  template <bool G = false>
  __device__ static __forceinline__ uint32_t round_mod(double y, RoundGuard<G> *rg = nullptr) {
    const double r = __fma_rn(-floor(y * (1.0 / 134215681.0)), 134215681.0, y);
    const double s = r + 6755399441055744.0;
    if constexpr (G) rg->note(r, s - 6755399441055744.0);
    return (uint32_t)__builtin_bit_cast(uint64_t, s);
  }
  // NonPowOf2ApproxSignedBasis (logB 5, d 4, drop 7) on a canonical residue: y = floor((v + 2^6)
  // / 2^7) has balanced base-32 digits d_k in [-16, 15] (k < 3) and an unbounded top digit; in
  // closed form, with y' = y + 16 (1 + 32 + 32^2): d_k = ((y' >> 5k) & 31) - 16 for k < 3 and
  // d_3 = y' >> 15 (the same digits as the recursive Digits8<LOGB1, D1, DROP1>). The word kept is
  // y' ^ (16 (1 + 32 + 32^2)): field k then holds d_k in two's complement (d_k + 16 = f in
  // [0, 32) and (f - 16) mod 32 = f ^ 16), the top digit is unchanged, and every digit is one
  // signed bit-field extract with wave-uniform offset and width (Lvl1Off::digit_u). Returns that word.
  static constexpr int DIGIT_BIAS = ((1 << (LOGB1 * (D1 - 1))) - 1) / ((1 << LOGB1) - 1) * (1 << (LOGB1 - 1));
  __device__ static __forceinline__ uint32_t digits(int v) {
    return (uint32_t)(((v + (1 << (DROP1 - 1))) >> DROP1) + DIGIT_BIAS) ^ (uint32_t)DIGIT_BIAS;
  }
};

// br1f keeps ACC offset by H/2: ac'' in [0, Q) with ac'' = ac + H/2 (mod Q). The stored negacyclic
// extension n = H - ac'' = -ac + H/2 is then in the same representation (as a signed u32, in
// [-H, H]) and is also the operand of the digit word: for a rotated entry x'' (either half),
// t = x'' + n = (x - ac) + H (mod Q) with t in (-Q, 2Q), so one v_min3_u32(t, t + Q, t - Q) (the
// wrapped operands lose) is canon(x - ac) + H in [0, Q), and the digit word of the canonical
// residue y - H is ((y - H + 2^6 + 2^7 DIGIT_BIAS) >> 7) ^ DIGIT_BIAS (the bias folded in before
// the shift; the shift itself folds into the extraction offsets, digits_u): 5 integer operations
// per word. The accumulator update adds a
// rounded product in [0, Q] (Lvl1Int::round_mod): s in [0, 2Q), min(s, s - Q), 3 operations.
struct Lvl1Off {
  static constexpr uint32_t Q = (uint32_t)Lvl1Int::Q, H = (uint32_t)Lvl1Int::H, OFF = H / 2;
  static_assert(H % 2 == 0, "H/2 offset");
  __device__ static __forceinline__ uint32_t fold(uint32_t y, uint32_t yq, uint32_t ymq) {  // y, y + Q, y - Q
    return min(min(y, yq), ymq);
  }
  // centred value v in [-H, H] -> ac''
  __device__ static __forceinline__ uint32_t enc(int v) {
    const uint32_t y = (uint32_t)(v + (int)OFF);
    return min(y, y + Q);
  }
  // ac'' -> centred value in [-H, H]
  __device__ static __forceinline__ int dec(uint32_t acpp) { return Lvl1Int::canon((int)acpp - (int)OFF); }
  // the stored negacyclic half "-ac + H/2" and the digit operand
  __device__ static __forceinline__ uint32_t neg(uint32_t acpp) { return H - acpp; }
  // digit word of canon(x - ac) from a stored entry x'' and n = neg(ac''): t = x - ac + H; the
  // Lvl1Int::digits word before its shift by DROP1 (bits 7.. hold the fields, bits 0..6 the dropped
  // remainder, never read): the shift folds into the extraction offsets (digit_u / digit_shifts_u),
  // one operation fewer per word. Both br1l and br1f use it (br1f since round 5: at 248 VGPRs it no
  // longer spills; same speed, profiles/r05n/bench_variants.log).
  __device__ static __forceinline__ uint32_t digits_u(uint32_t xs, uint32_t n) {
    const uint32_t t = xs + n;
    const uint32_t y = fold(t, t + Q, t - Q);
    constexpr uint32_t C = (uint32_t)((1 << (DROP1 - 1)) - Lvl1Int::H + (Lvl1Int::DIGIT_BIAS << DROP1));
    return (y + C) ^ ((uint32_t)Lvl1Int::DIGIT_BIAS << DROP1);
  }
  // signed digit k of a digits_u() word: one v_bfe_i32 at offset DROP1 + 5 k (the top digit: the
  // word's sign-extended rest)
  __device__ static __forceinline__ double digit_u(uint32_t w, int k) {
    return (double)(int)__builtin_amdgcn_sbfe(w, DROP1 + LOGB1 * k, k < D1 - 1 ? LOGB1 : 32 - DROP1 - LOGB1 * (D1 - 1));
  }
  // signed digit k of a digits_u() word by two shifts
  __device__ static __forceinline__ double digit_shifts_u(uint32_t w, int k) {
    const int s1 = k < D1 - 1 ? 32 - DROP1 - LOGB1 * (k + 1) : 0;
    const int s2 = k < D1 - 1 ? 32 - LOGB1 : DROP1 + LOGB1 * (D1 - 1);
    return (double)((int)(w << s1) >> s2);
  }
  // ac'' + r for r in [0, Q], reduced to [0, Q)
  __device__ static __forceinline__ uint32_t add(uint32_t acpp, uint32_t r) {
    const uint32_t s = acpp + r;
    return min(s, s - Q);
  }
  template <bool G>
  __device__ static __forceinline__ uint32_t round(double y, RoundGuard<G> *rg) { return Lvl1Int::round_mod<G>(y, rg); }
};

// ACC layout: ac[p][h * 8 + e] = coefficient lane + 64 e + 512 h of poly p (0 mask, 1 body).
__device__ __forceinline__ int acc_coef(int lane, int i) { return lane + 64 * (i & 7) + 512 * (i >> 3); }

typedef __attribute__((address_space(3))) uint32_t lds_u32;

// signed digit k of an Lvl1Int::digits word: fields of LOGB1 bits from bit 0, the top digit the
// sign-extended rest
__device__ __forceinline__ double lvl1_digit(uint32_t w, int k) {
  return (double)(int)__builtin_amdgcn_sbfe(w, LOGB1 * k, k < D1 - 1 ? LOGB1 : 32 - LOGB1 * (D1 - 1));
}

// The LWE of rotation g into la[0..N0) (LDS), by thread t of nt; returns its body b. Clue g % 7 of
// message g / 7 (lwe_a == nullptr: CmLweCiphertext::extract_all, :514) or LWE g. The caller's
// barrier makes la visible.
__device__ __forceinline__ int lvl1_stage_lwe(const uint16_t *__restrict__ clue_a,
                                              const uint16_t *__restrict__ clue_b,
                                              const uint16_t *__restrict__ lwe_a,
                                              const uint16_t *__restrict__ lwe_b, size_t g, uint16_t *la, int t,
                                              int nt) {
  if (lwe_a == nullptr) {
    const size_t m = g / CLUES;
    const int c = (int)(g % CLUES);
    const uint16_t *A = clue_a + m * N0;
    for (int i = t; i < N0; i += nt)
      la[i] = i <= c ? (uint16_t)(A[c - i] & (Q0 - 1)) : (uint16_t)((Q0 - A[N0 + c - i]) & (Q0 - 1));
    return clue_b[m * CLUES + c] & (Q0 - 1);
  }
  for (int i = t; i < N0; i += nt) la[i] = lwe_a[g * N0 + i] & (Q0 - 1);
  return lwe_b[g] & (Q0 - 1);
}

// Coefficient j of the initial body accumulator X^{-b} * LUT1 (the mask starts at 0), centred.
__device__ __forceinline__ double lvl1_acc_init(const DeviceTables &tb, int b, int j) {
  const int r0 = (2 * N1 - (b % (2 * N1))) % (2 * N1);
  return canon_small<Mod<1>>(rot_read<N1>(tb.lut1, j, r0));
}

// Centred coefficient j of polynomial p of rotation g's caller-supplied initial accumulator (the
// test entry omr_blind_rotate_level1_from: acc0 canonical u64 [2][N1] per rotation, the output's layout).
__device__ __forceinline__ int lvl1_acc_from(const uint64_t *__restrict__ acc0, size_t g, int p, int j) {
  const int v = (int)acc0[(g * 2 + p) * N1 + j];
  return v > Lvl1Int::H ? v - Lvl1Int::Q : v;
}

// One polynomial staged with its negacyclic extension ext = [ACC, -ACC] (2N u32 = 8 KB at st), so
// (X^a * ACC)[j] = ext[(j - a) mod 2N]: no sign fix-up per coefficient. ACC in the Lvl1Off
// representation: ext = [ac'', H - ac''], every entry "value + H/2". n: the stored negacyclic half,
// for a caller that keeps it in registers as the digit operand.
__device__ __forceinline__ void lvl1_stage_ext(uint32_t *st, const uint32_t (&ac)[16], int lane, uint32_t (&n)[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    n[i] = Lvl1Off::neg(ac[i]);
    st[acc_coef(lane, i)] = ac[i];
    st[N1 + acc_coef(lane, i)] = n[i];
  }
}
__device__ __forceinline__ void lvl1_stage_ext(uint32_t *st, const uint32_t (&ac)[16], int lane) {
  uint32_t n[16];
  lvl1_stage_ext(st, ac, lane, n);
}
// Rotated reads of the staged ext by X^a: entry (j - a) mod 2N for coefficient j = acc_coef(lane, i)
// = lane + 64 i. st is 8 KB-aligned, so the entry's LDS byte address is
// st | ((4 (lane - a) + 256 i) & 8191): one add and one v_and_or_b32 per read (not formed by the
// compiler; the mask in an SGPR: no VOP3 literals on gfx9, one SGPR per VOP3).
struct Lvl1RotRead {
  uint32_t sbase, b4;
  __device__ __forceinline__ Lvl1RotRead(const uint32_t *st, int lane, int a)
      : sbase((uint32_t)(size_t)(lds_u32 *)st), b4((uint32_t)(lane - a) * 4u) {}
  __device__ __forceinline__ uint32_t operator()(int i) const {
    const uint32_t kWrap = 8u * N1 - 1;  // 8 KB - 1
    uint32_t addr;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(addr) : "v"(b4 + 256u * i), "s"(kWrap), "v"(sbase));
    return *(const lds_u32 *)(size_t)addr;
  }
};

// One spectrum point x of a digit polynomial times its GGSW row's keys, added into the outputs A
// and B: the rows of a CMUX step accumulate in row order in every family.
__device__ __forceinline__ void lvl1_mac(double xr, double xi, double2 ka, double2 kB, double &ar, double &ai,
                                         double &br, double &bi) {
  ar = __fma_rn(xr, ka.x, __fma_rn(-xi, ka.y, ar));
  ai = __fma_rn(xr, ka.y, __fma_rn(xi, ka.x, ai));
  br = __fma_rn(xr, kB.x, __fma_rn(-xi, kB.y, br));
  bi = __fma_rn(xr, kB.y, __fma_rn(xi, kB.x, bi));
}

// A rotation's output from one wave's registers: v(p, i) = centred coefficient acc_coef(lane, i) of
// poly p (0 mask, 1 body). mode 0: extract_lwe_locally (coefficient 0; detector.rs:561) into
// ext[g], the mask reversed through st (4 KB of the wave's LDS); mode 1: the full RLWE into
// rlwe_out[g]. (v is a callable, not an int[2][16]: decoding all 32 values ahead of the branch on
// mode changed the register allocation of br1f's CMUX loop, which then re-materialised its FP64
// constants every step.)
template <typename V>
__device__ __forceinline__ void lvl1_store_wave(V v, int *st, size_t g, int mode, uint32_t *__restrict__ ext,
                                                uint64_t *__restrict__ rlwe_out, int lane) {
  if (mode == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) st[acc_coef(lane, i)] = v(0, i);
    wave_lds_sync();
    uint32_t *o = ext + g * (N1 + 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = acc_coef(lane, i);
      o[j] = Lvl1Int::to_u32(j == 0 ? st[0] : -st[N1 - j]);
    }
    if (lane == 0) o[N1] = Lvl1Int::to_u32(v(1, 0));
  } else {
    uint64_t *o = rlwe_out + g * 2 * N1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      o[acc_coef(lane, i)] = Lvl1Int::to_u32(v(0, i));
      o[N1 + acc_coef(lane, i)] = Lvl1Int::to_u32(v(1, i));
    }
  }
}

}  // namespace omr
