// Device key and clue generation from the same seeded ChaCha12
// streams as the host generators (rng.hpp, keygen.hip), so every clue and every key row is
// bit-identical to theirs whichever device, shard or thread count produces it:
//   omr_gen_clues_device             Sender::gen_clues (sender.rs:27-32, key_gen/clue.rs:27-34)
//   omr_keygen_detection_key_device  SecretKeyPack::generate_detector (key_gen/secret.rs:118-178)
//   omr_sender_gen_clues_device      the same clues under a table of public clue keys (sender_kernels.hpp)
//   omr_clue_open_device             SecretKeyPack::decrypt_clue (secret.rs:267-270) for a whole board
// and the seeded detection key (include/omr_gpu.h): its generator, the mask rows and the expansion.
//
// Stream consumption is data dependent (rejection-sampled uniforms, Gaussians that draw a sign
// word only when non-zero), so each workgroup first expands its stream into LDS with every
// thread computing ChaCha blocks, then:
//   * uniforms: draw j is speculatively taken from words (2j, 2j+1); a workgroup vote detects a
//     rejection (probability 1.5e-5 per draw mod q1, 1.5e-11 mod q2) and only then one thread
//     compacts the draws sequentially (uniform_draws);
//   * Gaussians: every thread evaluates the sample that would start at each word position
//     (value and words used, packed), then one thread walks the chain of start positions.
// RLWE rows then compute a*s with the device NTT (kernels.hpp) — the product mod q is unique,
// so the result equals the host's exact-integer NTT product.
#include <string>
#include <vector>

#include "hip_util.hpp"
#include "host_ring.hpp"
#include "kernels.hpp"
#include "rng.hpp"
#include "sender.hpp"

using namespace omr;

namespace {

constexpr int CDT_LDS = 64;  // CDT tables up to this size are searched from LDS
constexpr int SLACK = 32;    // rejected uniform draws a row may absorb before it reports overrun

// Fill w[0, 16 * nblk) with the words of Stream(seed, dom, stream) (rng.hpp).
__device__ void fill_words(uint32_t *w, int nblk, uint64_t seed, uint32_t dom, uint64_t stream) {
  const uint32_t key[8] = {(uint32_t)seed, (uint32_t)(seed >> 32), 0x6b657967u, dom, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) {
    uint32_t o[16];
    chacha_block(12, key, (uint64_t)b, stream, o);
#pragma unroll
    for (int i = 0; i < 16; ++i) w[16 * b + i] = o[i];
  }
}

__device__ __forceinline__ uint64_t word_pair(const uint32_t *w, int j) {
  return (((uint64_t)w[2 * j + 1]) << 32) | w[2 * j];
}

// COUNT draws of Stream::uniform(Q) (rng.hpp; MASK = the bit length of Q) over the words w of a row
// stream in LDS. Every thread of the workgroup calls it after the barrier that follows the fill. On
// return word_pair(w, j) & MASK is accepted draw j for j < COUNT, visible to every thread, and the
// result is the number of stream words the draws consumed. Draw j is speculatively words (2j, 2j+1);
// only when the workgroup vote finds a rejected draw does thread 0 compact the accepted draws in place,
// sequentially. A row that rejects more than SLACK draws sets *overrun.
template <uint64_t Q, uint64_t MASK, int COUNT>
__device__ int uniform_draws(uint32_t *w, int *overrun) {
  static_assert(Q - 1 <= MASK && MASK < 2 * Q, "mask = bit length of q (Stream::uniform)");
  __shared__ int used;
  int rej = 0;
  for (int j = threadIdx.x; j < COUNT; j += blockDim.x) rej |= (word_pair(w, j) & MASK) >= Q;
  if (!__syncthreads_or(rej)) return 2 * COUNT;
  if (threadIdx.x == 0) {
    int d = 0, cnt = 0;
    while (cnt < COUNT && d < COUNT + SLACK) {
      const uint64_t v = word_pair(w, d) & MASK;
      ++d;
      if (v < Q) {  // cnt < d: the words overwritten have been consumed
        w[2 * cnt] = (uint32_t)v;
        w[2 * cnt + 1] = (uint32_t)(v >> 32);
        ++cnt;
      }
    }
    if (cnt < COUNT) atomicOr(overrun, 1);
    used = 2 * d;
  }
  __syncthreads();
  return used;
}

// Gaussian::sample started at word p (rng.hpp): upper_bound of next64() >> 1 in the CDT, sign
// from one more word when non-zero. Returns (sample << 2) | words used.
__device__ __forceinline__ int gauss_packed(const uint32_t *w, int p, const uint64_t *tab, int n) {
  const uint64_t u = ((((uint64_t)w[p + 1]) << 32) | w[p]) >> 1;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] <= u) lo = mid + 1;
    else hi = mid;
  }
  const int k = lo >= n ? n - 1 : lo;
  if (k == 0) return 2;
  return (((w[p + 2] & 1u) ? -k : k) * 4) | 3;
}

// Replace w[p0, p0 + span) by the packed sample starting at each position (all threads), so
// that one thread can then walk the chain in one LDS read per sample.
__device__ __forceinline__ void pack_gaussians(uint32_t *w, int nw, int p0, int span, const uint64_t *tab, int n) {
  constexpr int MAXK = 32;
  int v[MAXK];
  const int T = blockDim.x;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    const int p = p0 + threadIdx.x + k * T;
    v[k] = (k * T < span && p < p0 + span && p + 2 < nw) ? gauss_packed(w, p, tab, n) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    const int p = p0 + threadIdx.x + k * T;
    if (k * T < span && p < p0 + span && p + 2 < nw) w[p] = (uint32_t)v[k];
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// Clues: u = A*r + e1, v = B*r + e2 over Z_2048[X]/(X^512+1), r binary (keygen.hip
// omr_gen_clues). One 64-thread workgroup per message.
// ------------------------------------------------------------------------------------------
constexpr int CLUE_WORDS = 16 * 101;  // 16 (r) + 3 * 519 Gaussian words at most, + slack

__global__ __launch_bounds__(64) void gen_clues_kernel(const uint16_t *__restrict__ pk,
                                                       const uint64_t *__restrict__ cdt, int cdt_n,
                                                       uint64_t seed, uint64_t first, size_t count,
                                                       uint16_t *__restrict__ clue_a,
                                                       uint16_t *__restrict__ clue_b) {
  __shared__ uint32_t w[CLUE_WORDS];
  __shared__ int32_t A[N0], B[N0], es[N0 + CLUES];
  __shared__ uint64_t tab[CDT_LDS];
  const size_t m = blockIdx.x;
  const int tid = threadIdx.x;
  if (m >= count) return;
  for (int i = tid; i < N0; i += 64) {
    A[i] = pk[i];
    B[i] = pk[N0 + i];
  }
  for (int i = tid; i < cdt_n; i += 64) tab[i] = cdt[i];
  fill_words(w, CLUE_WORDS / 16, seed, DOM_CLUE, first + m);
  __syncthreads();
  pack_gaussians(w, CLUE_WORDS, 16, 3 * (N0 + CLUES), tab, cdt_n);
  if (tid == 0) {
    int p = 16;
    for (int i = 0; i < N0 + CLUES; ++i) {
      const int v = (int)w[p];
      es[i] = v >> 2;
      p += v & 3;
    }
  }
  __syncthreads();
  // r = words 0..15, bit b of word k is r[32k + b]
  int acc[N0 / 64];
#pragma unroll
  for (int j = 0; j < N0 / 64; ++j) acc[j] = es[tid + 64 * j];
  int accb = tid < CLUES ? es[N0 + tid] : 0;
  for (int k = 0; k < N0 / 32; ++k) {
    uint32_t bits = __builtin_amdgcn_readfirstlane(w[k]);
    while (bits) {
      const int t = 32 * k + __builtin_ctz(bits);
      bits &= bits - 1;
#pragma unroll
      for (int j = 0; j < N0 / 64; ++j) {
        const int d = tid + 64 * j - t;  // u[o] += A[o - t] (o >= t), -= A[o - t + 512]
        const int a = A[d & (N0 - 1)];
        acc[j] += d >= 0 ? a : -a;
      }
      if (tid < CLUES) {
        const int d = tid - t;
        const int b = B[d & (N0 - 1)];
        accb += d >= 0 ? b : -b;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < N0 / 64; ++j) clue_a[m * N0 + tid + 64 * j] = (uint16_t)(acc[j] & (Q0 - 1));
  if (tid < CLUES) clue_b[m * CLUES + tid] = (uint16_t)(accb & (Q0 - 1));
}

#include "sender_kernels.hpp"  // sender_clues_kernel, clue_open_kernel

// ------------------------------------------------------------------------------------------
// RLWE key rows (keygen.hip ggsw_row): a uniform, b = a*s + e (- sigma_scale * sigma_g(s)),
// plus mg in coefficient 0 of component comp. 256 threads per row.
// ------------------------------------------------------------------------------------------
struct RowJob {
  uint64_t seed;
  uint32_t domain;              // plain rows: mask then noise; seeded rows: the noise, from word 0
  uint64_t mask_seed;           // seeded rows: Stream(mask_seed, mask_domain, row) draws the mask
  uint32_t mask_domain;
  int rows;                     // rows in this launch
  int dsplit;                   // comp = (row % (2 dsplit)) >= dsplit
  const uint64_t *mg;           // [rows] gadget value added in coefficient 0 (0: none)
  const int8_t *s;              // seeded rows: the ternary coefficients of s (a-gadget rows: - mg s)
  const double *s_hat;          // NTT(s), centred, device NTT order
  const double *tw, *itw;       // device NTT twiddles (kernels.hpp convention)
  double ninv;                  // N^-1 mod q, centred
  const uint64_t *cdt;          // Gaussian CDT (<= CDT_LDS entries)
  int cdt_n;
  const int8_t *sigma_s;        // trace key: [TRACE_STEPS][N] sigma_g(s); null otherwise
  const uint64_t *sigma_scale;  // trace key: [rows] 2^(2j) mod q
  int *overrun;                 // set when a row rejects more than SLACK uniform draws
};

template <int LEVEL>
struct Lvl {
  static constexpr uint64_t Q = LEVEL == 1 ? Q1 : Q2;
  static constexpr uint64_t MASK = LEVEL == 1 ? (1ull << 27) - 1 : (1ull << 50) - 1;  // bit length of q
};

// Plain rows (a, b) at out + row * 2N; seeded rows (SEEDED) write the body alone, at out + row * N, of
// the row whose mask is the public stream's: a = mask, and the a-gadget goes into b as - mg s.
template <int LEVEL, typename OUT, bool SEEDED>
__global__ __launch_bounds__(256) void rlwe_rows_kernel(RowJob job, OUT *__restrict__ out) {
  using M = Mod<LEVEL>;
  constexpr int N = M::N, T = 256, E = N / T;
  constexpr uint64_t Q = Lvl<LEVEL>::Q, MASK = Lvl<LEVEL>::MASK;
  using NTT = WgNtt<M, T, E>;
  constexpr int NWM = 2 * N + 2 * SLACK;  // the words N uniform draws can consume
  constexpr int NW = NWM + 3 * N + 16;    // and N Gaussians after them
  static_assert(NWM % 16 == 0 && NW % 16 == 0 && NTT::LDS_DOUBLES * 2 <= NW, "word buffer doubles as NTT space");
  __shared__ uint32_t w[NW];
  __shared__ int32_t es[N];
  __shared__ uint64_t tab[CDT_LDS];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (row >= job.rows) return;
  OUT *oa = out + (size_t)row * 2 * N, *ob = SEEDED ? out + (size_t)row * N : oa + N;
  for (int i = tid; i < job.cdt_n; i += T) tab[i] = job.cdt[i];
  if (SEEDED) {
    fill_words(w, NWM / 16, job.mask_seed, job.mask_domain, (uint64_t)row);
    fill_words(w + NWM, (NW - NWM) / 16, job.seed, job.domain, (uint64_t)row);
  } else {
    fill_words(w, NW / 16, job.seed, job.domain, (uint64_t)row);
  }
  __syncthreads();
  const int after = uniform_draws<Q, MASK, N>(w, job.overrun);
  uint64_t a[E];
#pragma unroll
  for (int e = 0; e < E; ++e) a[e] = word_pair(w, tid + e * T) & MASK;
  // the Gaussians follow the uniforms in a plain row's stream and open a seeded row's noise stream
  uint32_t *wg = SEEDED ? w + NWM : w;
  const int g0 = SEEDED ? 0 : after;
  pack_gaussians(wg, SEEDED ? NW - NWM : NW, g0, 3 * N, tab, job.cdt_n);
  if (tid == 0) {
    int p = g0;
    for (int i = 0; i < N; ++i) {
      const int v = (int)wg[p];
      es[i] = v >> 2;
      p += v & 3;
    }
  }
  __syncthreads();  // the word buffer becomes the NTT exchange space
  // a * s = INTT(NTT(a) . NTT(s)) / N, coefficient tid + e T on return
  double *lds = reinterpret_cast<double *>(w);
  double x[E];
#pragma unroll
  for (int e = 0; e < E; ++e) x[e] = from_u64<M>(a[e]);
  NTT::fwd(x, lds, job.tw, tid);
#pragma unroll
  for (int e = 0; e < E; ++e) x[e] = canon<M>(mm<M>(canon<M>(x[e]), job.s_hat[tid * E + e]));
  NTT::inv(x, lds, job.itw, tid);
  const bool comp1 = (row % (2 * job.dsplit)) >= job.dsplit;
  const uint64_t mg = job.mg ? job.mg[row] : 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = tid + e * T;
    uint64_t b = to_u64<M>(canon<M>(mm<M>(canon<M>(x[e]), job.ninv)));
    b += es[j] < 0 ? Q - (uint64_t)(-es[j]) : (uint64_t)es[j];
    b = b >= Q ? b - Q : b;
    if (job.sigma_s) {  // - sigma_g(s) * 2^(2j)
      const int sg = job.sigma_s[(size_t)(row / DT) * N + j];
      const uint64_t sc = job.sigma_scale[row];
      if (sg) {
        const uint64_t c = sg < 0 ? Q - sc : sc;
        b = b >= c ? b - c : b + Q - c;
      }
    }
    if (SEEDED && !comp1 && mg) {  // - mg s
      const int sj = job.s[j];
      if (sj) {
        const uint64_t c = sj < 0 ? Q - mg : mg;
        b = b >= c ? b - c : b + Q - c;
      }
    }
    uint64_t av = a[e];
    if (j == 0 && mg) {
      if (comp1) b = (b + mg) % Q;
      else if (!SEEDED) av = (av + mg) % Q;
    }
    if (!SEEDED) oa[j] = (OUT)av;
    ob[j] = (OUT)b;
  }
}

// ------------------------------------------------------------------------------------------
// Key-switching key rows (keygen.hip): LWE(670) of s1[i] * 2^j under s_int. 64 threads per row.
// Plain rows a[670], b at out + row * 671; seeded rows (SEEDED) write b alone, at out + row: the mask
// from Stream(mask_seed, DOM_KSK_MASK, row), the Gaussian from word 0 of Stream(seed, DOM_KSK_NOISE, row).
// ------------------------------------------------------------------------------------------
constexpr int KSK_WORDS = 16 * 88;  // 2 (670 + SLACK) + 3 words, whole blocks
static_assert(2 * (NI + SLACK) + 3 <= KSK_WORDS, "KSK word buffer");

template <bool SEEDED>
__global__ __launch_bounds__(64) void ksk_rows_kernel(uint64_t seed, uint64_t mask_seed,
                                                      const uint8_t *__restrict__ sint,
                                                      const int8_t *__restrict__ s1,
                                                      const uint64_t *__restrict__ cdt, int cdt_n,
                                                      int rows, uint32_t *__restrict__ out,
                                                      int *overrun) {
  constexpr uint64_t MASK = Lvl<1>::MASK;
  __shared__ uint32_t w[KSK_WORDS];
  __shared__ uint32_t wn[16];
  __shared__ uint64_t part[64];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (row >= rows) return;
  uint32_t *o = out + (size_t)row * (NI + 1);
  fill_words(w, KSK_WORDS / 16, SEEDED ? mask_seed : seed, SEEDED ? DOM_KSK_MASK : DOM_KSK, (uint64_t)row);
  if (SEEDED) fill_words(wn, 1, seed, DOM_KSK_NOISE, (uint64_t)row);
  __syncthreads();
  const int after = uniform_draws<Q1, MASK, NI>(w, overrun);
  uint64_t sum = 0;
#pragma unroll 1
  for (int c = tid; c < NI; c += 64) {
    const uint64_t v = word_pair(w, c) & MASK;
    if (!SEEDED) o[c] = (uint32_t)v;
    if (sint[c]) sum += v;
  }
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    sum = 0;
#pragma unroll 4
    for (int t = 0; t < 64; ++t) sum += part[t];
    const int e = (SEEDED ? gauss_packed(wn, 0, cdt, cdt_n) : gauss_packed(w, after, cdt, cdt_n)) >> 2;
    uint64_t b = sum % Q1;
    b = (b + (e < 0 ? Q1 - (uint64_t)(-e) : (uint64_t)e)) % Q1;
    const uint64_t s = s1[row / KS_DIGITS] < 0 ? Q1 - 1 : (uint64_t)s1[row / KS_DIGITS];
    const uint64_t m = s * ((1ull << (row % KS_DIGITS)) % Q1) % Q1;
    (SEEDED ? out[row] : o[NI]) = (uint32_t)((b + m) % Q1);
  }
}

// ------------------------------------------------------------------------------------------
// Masks of seeded rows, and the expansion. Row r of the launch gets the first N accepted draws of
// Stream(seed, dom, first + r).uniform(q) at out + r * stride; with EXPAND also its body, body + r * N,
// behind them: the row (a, b) of the standard layout (stride 2N). 256 threads per RLWE row; the body is
// copied with 16-byte loads and stores before the stream is computed, the masks written with 16-byte stores.
// ------------------------------------------------------------------------------------------
template <int LEVEL, typename OUT, bool EXPAND>
__global__ __launch_bounds__(256) void mask_rows_kernel(uint64_t seed, uint32_t dom, uint64_t first, int rows,
                                                        const OUT *__restrict__ body, OUT *__restrict__ out,
                                                        size_t stride, int *overrun) {
  constexpr int N = Mod<LEVEL>::N, T = 256, V = 16 / (int)sizeof(OUT), PASSES = N / V / T;
  constexpr uint64_t Q = Lvl<LEVEL>::Q, MASK = Lvl<LEVEL>::MASK;
  constexpr int NW = 2 * N + 2 * SLACK;
  static_assert(NW % 16 == 0 && PASSES * V * T == N, "whole blocks, whole 16-byte pieces");
  __shared__ __attribute__((aligned(16))) uint32_t w[NW];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (row >= rows) return;
  uint4 *oa = reinterpret_cast<uint4 *>(out + (size_t)row * stride);
  if (EXPAND) {  // the body first: its loads and stores are in flight while the stream is computed
    const uint4 *ib = reinterpret_cast<const uint4 *>(body + (size_t)row * N);
#pragma unroll
    for (int k = 0; k < PASSES; ++k) oa[N / V + tid + k * T] = ib[tid + k * T];
  }
  fill_words(w, NW / 16, seed, dom, first + (uint64_t)row);
  __syncthreads();
  uniform_draws<Q, MASK, N>(w, overrun);
  const uint4 *w4 = reinterpret_cast<const uint4 *>(w);
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int i = tid + k * T;  // draws [V i, V i + V)
    uint4 v;
    if (LEVEL == 1) {
      const uint4 lo = w4[2 * i], hi = w4[2 * i + 1];
      constexpr uint32_t M = (uint32_t)MASK;
      v = make_uint4(lo.x & M, lo.z & M, hi.x & M, hi.z & M);
    } else {
      const uint4 p = w4[i];
      constexpr uint32_t MH = (uint32_t)(MASK >> 32);
      v = make_uint4(p.x, p.y & MH, p.z, p.w & MH);
    }
    oa[i] = v;
  }
}

// The same for key-switching rows, 64 threads per row: 670 masks at out + r * 670, or with EXPAND the row
// a[670], b at out + r * 671. A row is 2,684 bytes, so rows are not 16-byte aligned: 4-byte stores, 256
// contiguous bytes per wave.
template <bool EXPAND>
__global__ __launch_bounds__(64) void ksk_mask_rows_kernel(uint64_t seed, uint64_t first, int rows,
                                                           const uint32_t *__restrict__ body,
                                                           uint32_t *__restrict__ out, int *overrun) {
  constexpr uint64_t MASK = Lvl<1>::MASK;
  __shared__ uint32_t w[KSK_WORDS];
  const int row = blockIdx.x, tid = threadIdx.x;
  if (row >= rows) return;
  uint32_t *o = out + (size_t)row * (NI + (EXPAND ? 1 : 0));
  fill_words(w, KSK_WORDS / 16, seed, DOM_KSK_MASK, first + (uint64_t)row);
  __syncthreads();
  uniform_draws<Q1, MASK, NI>(w, overrun);
  for (int c = tid; c < NI; c += 64) o[c] = (uint32_t)(word_pair(w, c) & MASK);
  if (EXPAND && tid == 0) o[NI] = body[row];
}

std::vector<double> centred_vec(const std::vector<uint64_t> &v, uint64_t q) {
  std::vector<double> r(v.size());
  for (size_t i = 0; i < v.size(); ++i) r[i] = centred(v[i], q);
  return r;
}

}  // namespace

extern "C" omr_status omr_gen_clues_device(const omr_secret_key_pack *sk, uint64_t seed, uint64_t first,
                                           size_t count, uint16_t *d_clue_a, uint16_t *d_clue_b,
                                           void *stream) {
  if (!sk || (count && (!d_clue_a || !d_clue_b)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_gen_clues_device: NULL argument");
  if (count == 0) return OMR_OK;
  hipStream_t st = (hipStream_t)stream;
  const Gaussian g(SIGMA_CLUE);
  if (g.table().size() > (size_t)CDT_LDS)
    return set_error(OMR_ERR_DEVICE, "omr_gen_clues_device: CDT table too large");
  std::vector<uint16_t> pk(sk->pk_a, sk->pk_a + N0);
  pk.insert(pk.end(), sk->pk_b, sk->pk_b + N0);
  DevBuf<uint16_t> dpk;
  DevBuf<uint64_t> dcdt;
  HIP_TRY(dpk.upload(pk, st));
  HIP_TRY(dcdt.upload(g.table(), st));
  constexpr size_t CHUNK = 1u << 20;
  for (size_t off = 0; off < count; off += CHUNK) {
    const size_t n = std::min(CHUNK, count - off);
    gen_clues_kernel<<<(unsigned)n, 64, 0, st>>>(dpk, dcdt, (int)g.table().size(), seed, first + off, n,
                                                d_clue_a + off * N0, d_clue_b + off * CLUES);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  return OMR_OK;
}

// The sender's mixed-recipient board in one launch per 2^20 messages: the key table, the Gaussian table
// and the error word are the handle's, uploaded once by omr_sender_create (keygen.hip).
extern "C" omr_status omr_sender_gen_clues_device(omr_sender *s, const uint32_t *d_recipient, uint64_t seed,
                                                  uint64_t first, size_t count, uint16_t *d_clue_a,
                                                  uint16_t *d_clue_b, void *stream) {
  if (!s || (count && (!d_clue_a || !d_clue_b)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_gen_clues_device: NULL argument");
  if (s->device < 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_gen_clues_device: the sender was created without a device");
  if (count == 0) return OMR_OK;
  if (s->cdt_n > CDT_LDS) return set_error(OMR_ERR_DEVICE, "omr_sender_gen_clues_device: CDT table too large");
  std::lock_guard<std::mutex> lk(s->mu);
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  constexpr size_t CHUNK = 1u << 20;
  for (size_t off = 0; off < count; off += CHUNK) {
    const size_t n = std::min(CHUNK, count - off);
    sender_clues_kernel<<<(unsigned)n, 64, 0, st>>>(s->d_keys, (uint32_t)s->n_keys,
                                                   d_recipient ? d_recipient + off : nullptr, s->d_cdt, s->cdt_n, seed,
                                                   first + off, n, off, d_clue_a + off * N0, d_clue_b + off * CLUES,
                                                   s->d_err);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long bad = SENDER_NO_ERROR;
  HIP_TRY(hipMemcpyAsync(&bad, s->d_err, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad != SENDER_NO_ERROR) {  // rearm the error word: the sender stays usable
    const unsigned long long none = SENDER_NO_ERROR;
    HIP_TRY(hipMemcpyAsync(s->d_err, &none, sizeof(none), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sender_gen_clues_device: recipient of message " +
                                                   std::to_string(bad) + " is not a key of the table");
  }
  return OMR_OK;
}

extern "C" omr_status omr_clue_open_device(const omr_secret_key_pack *sk, const uint16_t *d_clue_a,
                                           const uint16_t *d_clue_b, size_t count, uint8_t *d_values,
                                           uint8_t *d_pertinent, uint8_t *d_max_abs_noise, void *stream) {
  if (!sk || (!d_values && !d_pertinent && !d_max_abs_noise))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_open_device: NULL secret key pack or no output requested");
  if (count == 0) return OMR_OK;
  if (!d_clue_a || !d_clue_b) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_open_device: NULL clues");
  if ((uintptr_t)d_clue_a & 15)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_clue_open_device: d_clue_a not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  S0Bits s0{};
  for (int i = 0; i < N0; ++i) s0.w[i >> 5] |= (uint32_t)(sk->s0[i] & 1u) << (i & 31);
  constexpr size_t PER_WG = (size_t)OPEN_WAVES * OPEN_PER_WAVE, CHUNK = PER_WG << 20;  // 2^20 workgroups per launch
  for (size_t off = 0; off < count; off += CHUNK) {
    const size_t n = std::min(CHUNK, count - off);
    clue_open_kernel<<<(unsigned)((n + PER_WG - 1) / PER_WG), 64 * OPEN_WAVES, 0, st>>>(
        s0, d_clue_a + off * N0, d_clue_b + off * CLUES, n, d_values ? d_values + off * CLUES : nullptr,
        d_pertinent ? d_pertinent + off : nullptr, d_max_abs_noise ? d_max_abs_noise + off : nullptr);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  return OMR_OK;
}

namespace {

// Both device key generators: the plain key (mask_seed NULL; rows (a, b)) and the bodies of the seeded
// key (keygen.hip keygen_rows), bit-identical to the host's.
omr_status keygen_device(const omr_secret_key_pack *sk, uint64_t seed, const uint64_t *mask_seed, uint32_t *d_bsk1,
                         uint32_t *d_ksk, uint64_t *d_bsk2, uint64_t *d_tk, hipStream_t st, const std::string &who) {
  const bool sd = mask_seed != nullptr;
  const uint64_t ms = sd ? *mask_seed : 0;
  const Gaussian g1(SIGMA_BR1), gks(SIGMA_KS), g2(SIGMA_BR2), gt(SIGMA_TRACE);
  for (const Gaussian *g : {&g1, &g2, &gt})
    if (g->table().size() > (size_t)CDT_LDS) return set_error(OMR_ERR_DEVICE, who + ": CDT table too large");
  const HostNtt &T1 = ntt1(), &T2 = ntt2();
  // per-row gadget values (BlindRotationKey::generate: s_i * B^k * 2^drop in component k / D + k)
  std::vector<uint64_t> mg1((size_t)N0 * 2 * D1), mg2((size_t)NI * 2 * D2);
  for (size_t row = 0; row < mg1.size(); ++row) {
    const int r = (int)(row % (2 * D1)), k = r < D1 ? r : r - D1;
    mg1[row] = sk->s0[row / (2 * D1)] ? (1ull << (DROP1 + k * LOGB1)) : 0;
  }
  for (size_t row = 0; row < mg2.size(); ++row) {
    const int r = (int)(row % (2 * D2)), k = r < D2 ? r : r - D2;
    mg2[row] = sk->sint[row / (2 * D2)] ? (1ull << (DROP2 + k * LOGB2)) : 0;
  }
  // trace key: sigma_g(s2) per automorphism, 2^(2j) per digit (TraceKey::new)
  std::vector<int8_t> sgs((size_t)TRACE_STEPS * N2);
  std::vector<uint64_t> tscale((size_t)TRACE_STEPS * DT);
  for (int k = 0; k < TRACE_STEPS; ++k) {
    const uint32_t g = (uint32_t)(N2 >> k) + 1;
    for (int i = 0; i < N2; ++i) {
      const uint32_t e = (uint32_t)(((uint64_t)i * g) % (2 * N2));
      if (e < (uint32_t)N2) sgs[(size_t)k * N2 + e] = sk->s2[i];
      else sgs[(size_t)k * N2 + e - N2] = (int8_t)-sk->s2[i];
    }
    for (int j = 0; j < DT; ++j) tscale[(size_t)k * DT + j] = (1ull << (2 * j)) % Q2;
  }
  DevBuf<double> dtw1, ditw1, dtw2, ditw2, ds1, ds2;
  DevBuf<uint64_t> dmg1, dmg2, dscale, dc1, dcks, dc2, dct;
  DevBuf<int8_t> dsgs, dsk1, dsk2;
  DevBuf<uint8_t> dsint;
  DevBuf<int> dover;
  const int zero = 0;
  HIP_TRY(dtw1.upload(centred_vec(T1.w, Q1), st));
  HIP_TRY(ditw1.upload(centred_vec(T1.iw, Q1), st));
  HIP_TRY(dtw2.upload(centred_vec(T2.w, Q2), st));
  HIP_TRY(ditw2.upload(centred_vec(T2.iw, Q2), st));
  HIP_TRY(ds1.upload(centred_vec(sk->s1_ntt, Q1), st));
  HIP_TRY(ds2.upload(centred_vec(sk->s2_ntt, Q2), st));
  HIP_TRY(dmg1.upload(mg1, st));
  HIP_TRY(dmg2.upload(mg2, st));
  HIP_TRY(dscale.upload(tscale, st));
  HIP_TRY(dsgs.upload(sgs, st));
  HIP_TRY(dsk1.upload(sk->s1, N1, st));
  HIP_TRY(dsk2.upload(sk->s2, N2, st));
  HIP_TRY(dsint.upload(sk->sint, NI, st));
  HIP_TRY(dc1.upload(g1.table(), st));
  HIP_TRY(dcks.upload(gks.table(), st));
  HIP_TRY(dc2.upload(g2.table(), st));
  HIP_TRY(dct.upload(gt.table(), st));
  HIP_TRY(dover.upload(&zero, 1, st));
  RowJob j1{seed, sd ? DOM_BSK1_NOISE : DOM_BSK1, ms, DOM_BSK1_MASK, N0 * 2 * D1, D1, dmg1, dsk1, ds1, dtw1, ditw1,
            centred(T1.ninv, Q1), dc1, (int)g1.table().size(), nullptr, nullptr, dover};
  if (sd) rlwe_rows_kernel<1, uint32_t, true><<<j1.rows, 256, 0, st>>>(j1, d_bsk1);
  else rlwe_rows_kernel<1, uint32_t, false><<<j1.rows, 256, 0, st>>>(j1, d_bsk1);
  HIP_TRY(hipGetLastError());
  if (sd)
    ksk_rows_kernel<true><<<N1 * KS_DIGITS, 64, 0, st>>>(seed, ms, dsint, dsk1, dcks, (int)gks.table().size(),
                                                         N1 * KS_DIGITS, d_ksk, dover);
  else
    ksk_rows_kernel<false><<<N1 * KS_DIGITS, 64, 0, st>>>(seed, ms, dsint, dsk1, dcks, (int)gks.table().size(),
                                                          N1 * KS_DIGITS, d_ksk, dover);
  HIP_TRY(hipGetLastError());
  RowJob j2{seed, sd ? DOM_BSK2_NOISE : DOM_BSK2, ms, DOM_BSK2_MASK, NI * 2 * D2, D2, dmg2, dsk2, ds2, dtw2, ditw2,
            centred(T2.ninv, Q2), dc2, (int)g2.table().size(), nullptr, nullptr, dover};
  if (sd) rlwe_rows_kernel<2, uint64_t, true><<<j2.rows, 256, 0, st>>>(j2, d_bsk2);
  else rlwe_rows_kernel<2, uint64_t, false><<<j2.rows, 256, 0, st>>>(j2, d_bsk2);
  HIP_TRY(hipGetLastError());
  RowJob jt{seed, sd ? DOM_TK_NOISE : DOM_TK, ms, DOM_TK_MASK, TRACE_STEPS * DT, 1, nullptr, dsk2, ds2, dtw2, ditw2,
            centred(T2.ninv, Q2), dct, (int)gt.table().size(), dsgs, dscale, dover};
  if (sd) rlwe_rows_kernel<2, uint64_t, true><<<jt.rows, 256, 0, st>>>(jt, d_tk);
  else rlwe_rows_kernel<2, uint64_t, false><<<jt.rows, 256, 0, st>>>(jt, d_tk);
  HIP_TRY(hipGetLastError());
  int over = 0;
  HIP_TRY(hipMemcpyAsync(&over, dover, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (over) return set_error(OMR_ERR_DEVICE, who + ": uniform stream overrun");
  return OMR_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// Memory of the current device (anything else, pageable host memory included, is staged).
bool device_memory(const void *p) {
  hipPointerAttribute_t at;
  int cur = -1;
  if (hipPointerGetAttributes(&at, p) != hipSuccess || hipGetDevice(&cur) != hipSuccess) {
    (void)hipGetLastError();  // an unregistered host pointer is an error to some runtimes
    return false;
  }
  return at.type == hipMemoryTypeDevice && at.device == cur;
}

// Mask rows [first, first + rows) of component `comp` at d_out (rows of c.masks words), or with d_body
// (the launch's first body row, device memory) the expanded rows (c.row_elems words).
omr_status launch_mask_rows(int comp, uint64_t mask_seed, size_t first, size_t rows, const void *d_body,
                            void *d_out, int *d_over, hipStream_t st) {
  if (rows == 0) return OMR_OK;
  const unsigned g = (unsigned)rows;
  const int n = (int)rows;
  if (comp == OMR_KEY_KSK) {
    if (d_body) ksk_mask_rows_kernel<true><<<g, 64, 0, st>>>(mask_seed, first, n, (const uint32_t *)d_body, (uint32_t *)d_out, d_over);
    else ksk_mask_rows_kernel<false><<<g, 64, 0, st>>>(mask_seed, first, n, nullptr, (uint32_t *)d_out, d_over);
  } else if (comp == OMR_KEY_BSK1) {
    if (d_body)
      mask_rows_kernel<1, uint32_t, true><<<g, 256, 0, st>>>(mask_seed, DOM_BSK1_MASK, first, n, (const uint32_t *)d_body,
                                                             (uint32_t *)d_out, (size_t)2 * N1, d_over);
    else
      mask_rows_kernel<1, uint32_t, false><<<g, 256, 0, st>>>(mask_seed, DOM_BSK1_MASK, first, n, nullptr, (uint32_t *)d_out,
                                                              (size_t)N1, d_over);
  } else {
    const uint32_t dom = key_component(comp)->mask_dom;
    if (d_body)
      mask_rows_kernel<2, uint64_t, true><<<g, 256, 0, st>>>(mask_seed, dom, first, n, (const uint64_t *)d_body,
                                                             (uint64_t *)d_out, (size_t)2 * N2, d_over);
    else
      mask_rows_kernel<2, uint64_t, false><<<g, 256, 0, st>>>(mask_seed, dom, first, n, nullptr, (uint64_t *)d_out,
                                                              (size_t)N2, d_over);
  }
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// One component of a seeded key -> rows (mask, body) at d_out. A body in device memory is read in place;
// any other goes through a device staging buffer in pieces of at most 64 MiB.
template <typename T>
omr_status expand_component_device(int comp, uint64_t mask_seed, const T *body, T *d_out, int *d_over, hipStream_t st) {
  const KeyComponent &c = *key_component(comp);
  if (device_memory(body)) {
    if (!aligned16(body))
      return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_expand_detection_key_device: device body not 16-byte aligned");
    return launch_mask_rows(comp, mask_seed, 0, c.rows, body, d_out, d_over, st);
  }
  const size_t chunk = std::min(c.rows, std::max<size_t>(1, ((size_t)64 << 20) / (c.body() * sizeof(T))));
  DevBuf<T> tmp;
  HIP_TRY(tmp.alloc(chunk * c.body()));
  for (size_t p0 = 0; p0 < c.rows; p0 += chunk) {
    const size_t n = std::min(chunk, c.rows - p0);
    HIP_TRY(hipMemcpyAsync(tmp, body + p0 * c.body(), n * c.body() * sizeof(T), hipMemcpyDefault, st));
    OMR_TRY(launch_mask_rows(comp, mask_seed, p0, n, tmp.get(), d_out + p0 * c.row_elems, d_over, st));
    HIP_TRY(hipStreamSynchronize(st));  // the staging buffer is reused, and freed on return
  }
  return OMR_OK;
}

omr_status take_overrun(DevBuf<int> &dover, hipStream_t st, const char *who) {
  int over = 0;
  HIP_TRY(hipMemcpyAsync(&over, dover, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (over) return set_error(OMR_ERR_DEVICE, std::string(who) + ": uniform stream overrun");
  return OMR_OK;
}

}  // namespace

extern "C" omr_status omr_keygen_detection_key_device(const omr_secret_key_pack *sk, uint64_t seed,
                                                      uint32_t *d_bsk1, uint32_t *d_ksk,
                                                      uint64_t *d_bsk2, uint64_t *d_tk, void *stream) {
  if (!sk || !d_bsk1 || !d_ksk || !d_bsk2 || !d_tk)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_keygen_detection_key_device: NULL argument");
  return keygen_device(sk, seed, nullptr, d_bsk1, d_ksk, d_bsk2, d_tk, (hipStream_t)stream,
                       "omr_keygen_detection_key_device");
}

extern "C" omr_status omr_keygen_seeded_key_device(const omr_secret_key_pack *sk, uint64_t seed, uint64_t mask_seed,
                                                   uint32_t *d_bsk1_b, uint32_t *d_ksk_b, uint64_t *d_bsk2_b,
                                                   uint64_t *d_tk_b, void *stream) {
  if (!sk || !d_bsk1_b || !d_ksk_b || !d_bsk2_b || !d_tk_b)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_keygen_seeded_key_device: NULL argument");
  return keygen_device(sk, seed, &mask_seed, d_bsk1_b, d_ksk_b, d_bsk2_b, d_tk_b, (hipStream_t)stream,
                       "omr_keygen_seeded_key_device");
}

extern "C" omr_status omr_expand_detection_key_device(const omr_seeded_key_view *key, uint32_t *d_bsk1, uint32_t *d_ksk,
                                                      uint64_t *d_bsk2, uint64_t *d_tk, void *stream) {
  if (!key || !key->bsk1_b || !key->ksk_b || !key->bsk2_b || !key->trace_key_b || !d_bsk1 || !d_ksk || !d_bsk2 || !d_tk)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_expand_detection_key_device: NULL argument");
  if (!aligned16(d_bsk1) || !aligned16(d_bsk2) || !aligned16(d_tk))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_expand_detection_key_device: output not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DevBuf<int> dover;
  const int zero = 0;
  HIP_TRY(dover.upload(&zero, 1, st));
  OMR_TRY(expand_component_device(OMR_KEY_BSK1, key->mask_seed, key->bsk1_b, d_bsk1, dover, st));
  OMR_TRY(expand_component_device(OMR_KEY_KSK, key->mask_seed, key->ksk_b, d_ksk, dover, st));
  OMR_TRY(expand_component_device(OMR_KEY_BSK2, key->mask_seed, key->bsk2_b, d_bsk2, dover, st));
  OMR_TRY(expand_component_device(OMR_KEY_TRACE, key->mask_seed, key->trace_key_b, d_tk, dover, st));
  return take_overrun(dover, st, "omr_expand_detection_key_device");
}

extern "C" omr_status omr_key_masks_device(uint64_t mask_seed, int component, size_t first_row, size_t rows,
                                           void *d_out, void *stream) {
  const KeyComponent *c = key_component(component);
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_masks_device: no such component");
  if (first_row > c->rows || rows > c->rows - first_row)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_masks_device: row range beyond the component");
  if (rows == 0) return OMR_OK;
  if (!d_out || !aligned16(d_out))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_masks_device: d_out is NULL or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DevBuf<int> dover;
  const int zero = 0;
  HIP_TRY(dover.upload(&zero, 1, st));
  OMR_TRY(launch_mask_rows(component, mask_seed, first_row, rows, nullptr, d_out, dover, st));
  return take_overrun(dover, st, "omr_key_masks_device");
}
