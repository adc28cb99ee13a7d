// Digest encoding kernels: encode_pertinent_indices (detector.rs:223-339) and
// encode_pertinent_payloads (detector.rs:341-453). Each workgroup folds a chunk of messages into
// one partial RLWE digest in registers; a second kernel sums the chunk partials mod q2 (the
// reference's rayon `.reduce(add_element_wise)`, :333-336 / :445-448).
#pragma once

#include <climits>

#include "kernels.hpp"
#include "weights.hpp"

namespace omr {

struct EncodeLayout {  // RetrievalParams (retrieval_params.rs:50-106)
  int index_slots, slots_per_bucket, slots_per_segment, segment_per_cipher;
};

__device__ __forceinline__ double centred_lift(uint32_t v) {
  // v < half_p ? v : q - p + v  (detector.rs:294,431), as a centred residue
  return v < (uint32_t)(P + 1) / 2 ? (double)v : (double)v - (double)P;
}

// What the four encode kernels share. Each workgroup keeps its partial digest as accA / accB, ENC_E
// residues of either polynomial per thread, and folds one message at a time into it.
using EncM = Mod<2>;
using EncNtt = WgNtt<EncM, ENC_T, ENC_E>;

__device__ __forceinline__ void encode_init(double (&accA)[ENC_E], double (&accB)[ENC_E]) {
#pragma unroll
  for (int e = 0; e < ENC_E; ++e) accA[e] = accB[e] = 0.0;
}

// acc += pv * NTT(x) mod q2: pv is one message's pertinency ciphertext [2][N2], canonical; x its slots.
__device__ __forceinline__ void encode_fold(const uint64_t *__restrict__ pv, double (&x)[ENC_E], double *xch,
                                            const double *__restrict__ tw, double (&accA)[ENC_E],
                                            double (&accB)[ENC_E]) {
  using M = EncM;
  const int tid = threadIdx.x;
  EncNtt::fwd(x, xch, tw, tid);
  const uint64_t *pa = pv + tid * ENC_E;
  const uint64_t *pb = pa + N2;
#pragma unroll
  for (int e = 0; e < ENC_E; ++e) {
    accA[e] = red<M>(accA[e] + mm<M>(from_u64<M>(pa[e]), x[e]));
    accB[e] = red<M>(accB[e] + mm<M>(from_u64<M>(pb[e]), x[e]));
  }
}

// The workgroup's partial, canonical, at its place (blockIdx.y, blockIdx.x) of partial [n_ct][chunks][2][N2].
__device__ __forceinline__ void encode_store(uint64_t *__restrict__ partial, const double (&accA)[ENC_E],
                                             const double (&accB)[ENC_E]) {
  using M = EncM;
  uint64_t *o = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * N2 + threadIdx.x * ENC_E;
#pragma unroll
  for (int e = 0; e < ENC_E; ++e) {
    o[e] = to_u64<M>(canon<M>(accA[e]));
    o[N2 + e] = to_u64<M>(canon<M>(accB[e]));
  }
}

// grid (chunks, n_ct); partial [n_ct][chunks][2][N2] canonical u64.
__global__ __launch_bounds__(ENC_T) void encode_indices_kernel(
    const uint64_t *__restrict__ pv, int D, uint64_t offset, EncodeLayout ly, uint64_t seed,
    uint32_t first_ct, int per_wg, const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  constexpr int T = ENC_T, E = ENC_E;
  __shared__ double xch[EncNtt::LDS_DOUBLES];
  __shared__ uint8_t buckets[ENC_T][8];
  const int tid = threadIdx.x;
  const uint32_t ct = first_ct + blockIdx.y;
  const int m0 = blockIdx.x * per_wg;
  const int mcount = min(per_wg, D - m0);
  double accA[E], accB[E];
  encode_init(accA, accB);
  // per_wg may exceed ENC_T (large D): the bucket choices are staged ENC_T messages at a time
#pragma unroll 1
  for (int mb = 0; mb < mcount; mb += ENC_T) {
    const int cnt = min(ENC_T, mcount - mb);
    __syncthreads();  // every thread has finished reading the previous block's buckets
    if (tid < cnt) {
      uint32_t w[16];
      bucket_words(seed, ct, offset + m0 + mb + tid, w);
      for (int s = 0; s < ly.segment_per_cipher && s < 8; ++s) buckets[tid][s] = (uint8_t)bucket_of(w[s]);
    }
    __syncthreads();
#pragma unroll 1
    for (int mi = mb; mi < mb + cnt; ++mi) {
      const uint64_t gi = offset + m0 + mi;
      double x[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int pos = tid + e * T;
        const int s = pos / ly.slots_per_segment;
        double v = 0.0;
        if (s < ly.segment_per_cipher) {
          const int within = pos - s * ly.slots_per_segment;
          const int bk = within / ly.slots_per_bucket;
          const int slot = within - bk * ly.slots_per_bucket;
          if (bk == buckets[mi - mb][s]) {
            if (slot == ly.index_slots) {
              v = 1.0;
            } else {
              uint64_t t = gi;  // base-257 digit `slot` of gi (little endian)
              for (int q = 0; q < slot; ++q) t /= (uint64_t)P;
              v = centred_lift((uint32_t)(t % (uint64_t)P));
            }
          }
        }
        x[e] = v;
      }
      encode_fold(pv + (size_t)(m0 + mi) * 2 * N2, x, xch, tw, accA, accB);
    }
  }
  encode_store(partial, accA, accB);
}

// The payload encode (detector.rs:341-453), written once over a weight source. Ciphertext blockIdx.y holds
// per_ct combinations of PAYLOAD_LEN slots each: slot l of combination j is payload[l] * w_j mod 257, w_j
// the combination's weight for the message being folded. A source hands out those weights a round of at
// most ROUND consecutive messages at a time: stage(g0, cnt) prepares the round that starts at global
// message g0, and weight(j, i) is combination j's weight for the round's message i < cnt. A STAGED source
// keeps the round in LDS of its own (the kernel declares its Lds), filled between two barriers.

// The table of omr_payload_weights' layout: row [all] of each combination, read where it lies.
struct TableWeights {
  static constexpr bool STAGED = false;
  static constexpr int ROUND = INT_MAX;  // nothing to stage: a workgroup's messages are one round
  const uint16_t *__restrict__ rows;  // the ciphertext's first row: per_ct rows of `all`
  uint64_t all;
  const uint16_t *at;
  __device__ __forceinline__ void stage(uint64_t g0, int) { at = rows + g0; }
  __device__ __forceinline__ uint32_t weight(int j, int i) const { return at[(size_t)j * all + i]; }
};

// Indexed weights (weights.hpp, indexed_weight_block): no table. The ciphertext holds the combinations
// combo0 + j, j < per_ct; one at or beyond `combos` is padding with weight 0. Per round, thread
// t < per_ct * nblk computes the one ChaCha12 block of (combination t / nblk, 16-message block t % nblk)
// into LDS, nblk <= ENC_T / 16 + 1 being the 16-message blocks that the round's global indices touch.
constexpr int ENC_W_PER_CT = N2 / PAYLOAD_LEN;        // 3: the most combinations a ciphertext holds
constexpr int ENC_W_BLOCKS = ENC_T / 16 + 1;          // 9
static_assert(ENC_W_PER_CT * ENC_W_BLOCKS <= ENC_T, "one thread per staged weight block");
// One staged block: combination `combo`'s weights for the 16 messages of block blk, zeros for padding. The
// body of IndexedWeights::stage below, for encode_payloads_indexed_len_kernel's strided staging; stage keeps
// its own text because calling this from it reordered encode_payloads_indexed_kernel's listing.
__device__ __forceinline__ void indexed_weights_stage_block(const WeightKey &key, uint32_t combos, uint64_t combo,
                                                            uint64_t blk, uint16_t *dst) {
  if (combo < (uint64_t)combos) {
    indexed_weight_block(key, (uint32_t)combo, blk, dst);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) dst[i] = 0;
  }
}
struct IndexedWeights {  // its kernel reads wts itself (see there): no ROUND, no weight()
  using Lds = uint16_t[ENC_W_PER_CT][ENC_W_BLOCKS * 16];
  Lds &wts;
  const WeightKey &key;
  uint32_t combos;
  uint64_t combo0;
  int per_ct;
  int lane0;  // the round's first message's place in its 16-message block: message i's weight is wts[j][lane0 + i]
  __device__ __forceinline__ void stage(uint64_t g0, int cnt) {
    const int tid = threadIdx.x;
    const uint64_t blk0 = g0 >> 4;
    const int nblk = (int)(((g0 + cnt - 1) >> 4) - blk0) + 1;
    lane0 = (int)(g0 & 15);
    if (tid < per_ct * nblk) {
      const int j = tid / nblk, b = tid - j * nblk;
      // the padding rule below is also indexed_weights_stage_block's (above): change the two together
      uint16_t *dst = &wts[j][b * 16];
      if (combo0 + j < (uint64_t)combos) {
        indexed_weight_block(key, (uint32_t)(combo0 + j), blk0 + b, dst);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[i] = 0;
      }
    }
  }
};

// The reference's weights found through a seek (weights.hpp, "Reference payload weights by seek"): the same
// bits as TableWeights over omr_payload_weights' table. Row j of the board starts at draw j * all, so the
// round's messages g0 .. g0 + cnt - 1 of combination j are the draws n0 = j * all + g0 onward, at the raw
// positions pos(n0) .. pos(n0 + cnt - 1) <= pos(n0) + cnt - 1 + OMR_WEIGHT_SEEK_MAX: with the first one
// anywhere in its block, at most ENC_SEEK_WORDS raw words in ENC_SEEK_BLOCKS ChaCha blocks from block
// pos(n0) >> 4. Thread t < per_ct * ENC_SEEK_BLOCKS computes block t % ENC_SEEK_BLOCKS of combination
// t / ENC_SEEK_BLOCKS and writes each accepted word to the place of its draw, wts[j][draw - n0]: the LDS
// holds the round's weights in message order (rejected words dropped).
constexpr int ENC_SEEK_WORDS = ENC_T + 15 + OMR_WEIGHT_SEEK_MAX;  // 175: the most raw words one staged row spans
constexpr int ENC_SEEK_BLOCKS = (ENC_SEEK_WORDS + 15) / 16;       // 11
static_assert(ENC_SEEK_BLOCKS * 16 >= ENC_SEEK_WORDS, "the staged blocks cover the raw span of a row");
static_assert(ENC_W_PER_CT * ENC_SEEK_BLOCKS <= ENC_T, "one thread per staged raw block");
struct SeekWeights {
  static constexpr bool STAGED = true;
  static constexpr int ROUND = ENC_T;
  using Lds = uint16_t[ENC_W_PER_CT][ENC_T];
  Lds &wts;
  const WeightKey &key;
  const omr_weight_seek &seek;
  uint64_t all;
  uint32_t combos;
  uint64_t combo0;
  int per_ct;
  __device__ __forceinline__ void stage(uint64_t g0, int cnt) {
    const int tid = threadIdx.x;
    if (tid < per_ct * ENC_SEEK_BLOCKS) {
      const int j = tid / ENC_SEEK_BLOCKS, b = tid - j * ENC_SEEK_BLOCKS;
      if (combo0 + j < (uint64_t)combos) {
        const uint64_t n0 = (combo0 + j) * all + g0;  // the row's first staged draw
        const uint64_t blk = (seek_pos(seek, n0) >> 4) + b;
        if (blk <= seek_pos(seek, n0 + cnt - 1) >> 4) {
          uint32_t w[16];
          chacha_block(12, key.k, blk, 0, w);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            uint64_t draw;
            const bool accepted = seek_draw_at(seek, blk * 16 + i, &draw);
            const uint64_t at = draw - n0;  // wraps to a large value for a draw before n0
            if (accepted && at < (uint64_t)cnt) wts[j][at] = weight_of_word(w[i]);
          }
        }
      } else {
        for (int i = b; i < cnt; i += ENC_SEEK_BLOCKS) wts[j][i] = 0;
      }
    }
  }
  __device__ __forceinline__ uint32_t weight(int j, int i) const { return wts[j][i]; }
};

// One message's slots: payload [PAYLOAD_LEN] u16 times weight(j) per combination j < per_ct, zero beyond.
template <typename Weight>
__device__ __forceinline__ void payload_slots(const uint16_t *__restrict__ payload, int per_ct, Weight weight,
                                              double (&x)[ENC_E]) {
#pragma unroll
  for (int e = 0; e < ENC_E; ++e) {
    const int pos = threadIdx.x + e * ENC_T;
    const int j = pos / PAYLOAD_LEN;
    double v = 0.0;
    if (j < per_ct) {
      const int l = pos - j * PAYLOAD_LEN;
      const uint32_t w = weight(j);
      v = centred_lift(((uint32_t)payload[l] * w) % (uint32_t)P);
    }
    x[e] = v;
  }
}

// grid (chunks, n_ct): workgroup (chunk, c) folds the messages [chunk * per_wg, +per_wg) of the D given
// (pv [D][2][N2], payloads [D][612] u16, global index offset + m) into ciphertext c's partial. per_wg may
// exceed ENC_T (large D): the source's weights come a round at a time.
template <typename Src>
__device__ __forceinline__ void encode_payloads_body(const uint64_t *__restrict__ pv,
                                                     const uint16_t *__restrict__ payloads, int D, uint64_t offset,
                                                     int per_ct, int per_wg, const double *__restrict__ tw,
                                                     uint64_t *__restrict__ partial, Src &src) {
  __shared__ double xch[EncNtt::LDS_DOUBLES];
  const int m0 = blockIdx.x * per_wg;
  const int mcount = min(per_wg, D - m0);
  double accA[ENC_E], accB[ENC_E];
  encode_init(accA, accB);
#pragma unroll 1
  for (int mb = 0, cnt; mb < mcount; mb += cnt) {
    cnt = min(Src::ROUND, mcount - mb);
    if (Src::STAGED) __syncthreads();  // every thread has finished reading the previous round's weights
    src.stage(offset + m0 + mb, cnt);
    if (Src::STAGED) __syncthreads();
#pragma unroll 1
    for (int i = 0; i < cnt; ++i) {
      const int m = m0 + mb + i;
      double x[ENC_E];
      payload_slots(payloads + (size_t)m * PAYLOAD_LEN, per_ct, [&](int j) { return src.weight(j, i); }, x);
      encode_fold(pv + (size_t)m * 2 * N2, x, xch, tw, accA, accB);
    }
  }
  encode_store(partial, accA, accB);
}

// weights [n_ct * per_ct][all] u16 (global index).
__global__ __launch_bounds__(ENC_T) void encode_payloads_kernel(
    const uint64_t *__restrict__ pv, const uint16_t *__restrict__ payloads, int D, uint64_t offset,
    uint64_t all, const uint16_t *__restrict__ weights, int per_ct, int per_wg,
    const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  TableWeights src{weights + (size_t)blockIdx.y * per_ct * all, all, nullptr};
  encode_payloads_body(pv, payloads, D, offset, per_ct, per_wg, tw, partial, src);
}

// Ciphertext first_ct + blockIdx.y holds the combinations (first_ct + blockIdx.y) * per_ct + j, j < per_ct.
// encode_payloads_body and payload_slots written out: through them this kernel alone measured 2.2 % slower
// at 503 ciphertexts of 16,384 messages (115.1 against 112.6 ms; profiles/encode_shared/time.json), the
// other two a little faster. It shares the source, the fold and the store.
__global__ __launch_bounds__(ENC_T) void encode_payloads_indexed_kernel(
    const uint64_t *__restrict__ pv, const uint16_t *__restrict__ payloads, int D, uint64_t offset,
    WeightKey key, uint32_t combos, uint32_t first_ct, int per_ct, int per_wg,
    const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  __shared__ double xch[EncNtt::LDS_DOUBLES];
  __shared__ IndexedWeights::Lds wts;
  IndexedWeights src{wts, key, combos, ((uint64_t)first_ct + blockIdx.y) * (uint64_t)per_ct, per_ct, 0};
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * per_wg;
  const int mcount = min(per_wg, D - m0);
  double accA[ENC_E], accB[ENC_E];
  encode_init(accA, accB);
#pragma unroll 1
  for (int mb = 0; mb < mcount; mb += ENC_T) {
    const int cnt = min(ENC_T, mcount - mb);
    __syncthreads();  // every thread has finished reading the previous round's weights
    src.stage(offset + m0 + mb, cnt);
    __syncthreads();
#pragma unroll 1
    for (int mi = mb; mi < mb + cnt; ++mi) {
      const int m = m0 + mi;
      const int wi = src.lane0 + (mi - mb);
      double x[ENC_E];
#pragma unroll
      for (int e = 0; e < ENC_E; ++e) {
        const int pos = tid + e * ENC_T;
        const int j = pos / PAYLOAD_LEN;
        double v = 0.0;
        if (j < per_ct) {
          const int l = pos - j * PAYLOAD_LEN;
          const uint32_t w = wts[j][wi];
          v = centred_lift(((uint32_t)payloads[(size_t)m * PAYLOAD_LEN + l] * w) % (uint32_t)P);
        }
        x[e] = v;
      }
      encode_fold(pv + (size_t)m * 2 * N2, x, xch, tw, accA, accB);
    }
  }
  encode_store(partial, accA, accB);
}

// The indexed payload encode with the payload length as an argument (include/omr_gpu.h, "Payload length as a
// board parameter"): payloads [D][L] u16, 1 <= L <= OMR_PAYLOAD_LEN_MAX. Ciphertext ct = first_ct + blockIdx.y
// is stripe ct % stripes of group ct / stripes, which holds the combinations (ct / stripes) * per_ct + j,
// j < per_ct <= 16. One stripe: slot j * L + l is word l of combination j. Several stripes (per_ct = 1): slot i
// is word N2 * stripe + i while that is below L. Every other slot is zero.
//
// A thread's ENC_E slots tid + ENC_T * e are the same for every message, so each is decoded once, before the
// message loop, into one word: the combination's row offset in the staged weights (high half), the payload
// word (low half), or ENC_LEN_ZERO. The loop itself has no division. The weights are IndexedWeights' blocks
// for up to 16 combinations: 16 x 9 blocks are more than the ENC_T threads, so staging is a strided loop.
constexpr int ENC_LEN_PER_CT = OMR_PAYLOAD_PER_CT_MAX;  // 16
constexpr int ENC_LEN_ROW = ENC_W_BLOCKS * 16;          // 144 staged weights per combination
constexpr uint32_t ENC_LEN_ZERO = 0xFFFFFFFFu;
static_assert(ENC_LEN_PER_CT * ENC_LEN_ROW < 65536 && OMR_PAYLOAD_LEN_MAX <= 65536, "a slot decodes to two u16 halves");
static_assert(OMR_PAYLOAD_LEN_MAX <= 8 * N2, "at most 8 stripes");
__global__ __launch_bounds__(ENC_T) void encode_payloads_indexed_len_kernel(
    const uint64_t *__restrict__ pv, const uint16_t *__restrict__ payloads, int D, uint64_t offset,
    WeightKey key, uint32_t combos, uint32_t first_ct, int L, int per_ct, int stripes, int per_wg,
    const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  __shared__ double xch[EncNtt::LDS_DOUBLES];
  __shared__ uint16_t wts[ENC_LEN_PER_CT * ENC_LEN_ROW];
  const int tid = threadIdx.x;
  const uint64_t ct = (uint64_t)first_ct + blockIdx.y;
  const uint64_t combo0 = ct / (uint32_t)stripes * (uint32_t)per_ct;
  const int word0 = (int)(ct % (uint32_t)stripes) * N2;  // the stripe's first payload word
  uint32_t at[ENC_E];
#pragma unroll
  for (int e = 0; e < ENC_E; ++e) {
    const int pos = tid + e * ENC_T;
    if (stripes == 1) {
      const int j = pos / L;
      at[e] = j < per_ct ? (uint32_t)(j * ENC_LEN_ROW) << 16 | (uint32_t)(pos - j * L) : ENC_LEN_ZERO;
    } else {
      at[e] = word0 + pos < L ? (uint32_t)(word0 + pos) : ENC_LEN_ZERO;
    }
  }
  const int m0 = blockIdx.x * per_wg;
  const int mcount = min(per_wg, D - m0);
  double accA[ENC_E], accB[ENC_E];
  encode_init(accA, accB);
#pragma unroll 1
  for (int mb = 0; mb < mcount; mb += ENC_T) {
    const int cnt = min(ENC_T, mcount - mb);
    const uint64_t g0 = offset + m0 + mb, blk0 = g0 >> 4;
    const int nblk = (int)(((g0 + cnt - 1) >> 4) - blk0) + 1;  // <= ENC_W_BLOCKS
    const int lane0 = (int)(g0 & 15);
    __syncthreads();  // every thread has finished reading the previous round's weights
#pragma unroll 1
    for (int t = tid; t < per_ct * nblk; t += ENC_T) {
      const int j = t / nblk, b = t - j * nblk;
      indexed_weights_stage_block(key, combos, combo0 + j, blk0 + b, &wts[j * ENC_LEN_ROW + b * 16]);
    }
    __syncthreads();
#pragma unroll 1
    for (int mi = mb; mi < mb + cnt; ++mi) {
      const int m = m0 + mi;
      const int wi = lane0 + (mi - mb);
      const uint16_t *__restrict__ pay = payloads + (size_t)m * L;
      double x[ENC_E];
#pragma unroll
      for (int e = 0; e < ENC_E; ++e) {
        double v = 0.0;
        if (at[e] != ENC_LEN_ZERO) {
          const uint32_t w = wts[(at[e] >> 16) + wi];
          v = centred_lift(((uint32_t)pay[at[e] & 0xFFFFu] * w) % (uint32_t)P);
        }
        x[e] = v;
      }
      encode_fold(pv + (size_t)m * 2 * N2, x, xch, tw, accA, accB);
    }
  }
  encode_store(partial, accA, accB);
}

// The indexed weights in omr_payload_weights's layout, out [rows][all] u16: one thread per (row,
// 16-message block); rows at or beyond `combos` are zero.
__global__ void indexed_weights_table_kernel(WeightKey key, uint64_t all, uint32_t combos, uint32_t rows,
                                             uint16_t *__restrict__ out) {
  const uint64_t nblk = (all + 15) >> 4;
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (uint64_t)rows * nblk) return;
  const uint32_t j = (uint32_t)(idx / nblk);
  const uint64_t b = idx - (uint64_t)j * nblk;
  uint16_t w[16];
  if (j < combos) {
    indexed_weight_block(key, j, b, w);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = 0;
  }
  const uint64_t g0 = b << 4;
  uint16_t *o = out + (uint64_t)j * all + g0;
  for (int i = 0; i < 16 && g0 + i < all; ++i) o[i] = w[i];
}

// As encode_payloads_indexed_kernel; the seek covers combos * all draws.
__global__ __launch_bounds__(ENC_T) void encode_payloads_seek_kernel(
    const uint64_t *__restrict__ pv, const uint16_t *__restrict__ payloads, int D, uint64_t offset, uint64_t all,
    WeightKey key, omr_weight_seek seek, uint32_t combos, uint32_t first_ct, int per_ct, int per_wg,
    const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  __shared__ SeekWeights::Lds wts;
  SeekWeights src{wts, key, seek, all, combos, ((uint64_t)first_ct + blockIdx.y) * (uint64_t)per_ct, per_ct};
  encode_payloads_body(pv, payloads, D, offset, per_ct, per_wg, tw, partial, src);
}

// The builders' scan (omr_weight_seek_build_device): one ChaCha12 block of the reference stream per thread
// and grid-stride step, its 16 words compared with the zone. A rejected word at a raw position <= last takes
// a slot of the list with one atomic; only the first SEEK_LIST slots exist, and the count says whether
// the list is complete (weights.hpp, SEEK_LIST). hits[0] is the count, hits[1 ..] the list.
constexpr int SEEK_SCAN_T = 256;
__global__ __launch_bounds__(SEEK_SCAN_T) void weight_seek_scan_kernel(WeightKey key, uint64_t nblk, uint64_t last,
                                                                      uint32_t zone,
                                                                      unsigned long long *__restrict__ hits) {
  const uint64_t stride = (uint64_t)gridDim.x * SEEK_SCAN_T;
  for (uint64_t b = (uint64_t)blockIdx.x * SEEK_SCAN_T + threadIdx.x; b < nblk; b += stride) {
    uint32_t w[16];
    chacha_block(12, key.k, b, 0, w);
    bool any = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) any = any || weight_rejected(w[i], zone);
    if (!any) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint64_t r = b * 16 + i;
      if (weight_rejected(w[i], zone) && r <= last) {
        const unsigned long long slot = atomicAdd(&hits[0], 1ull);
        if (slot < SEEK_LIST) hits[1 + slot] = r;
      }
    }
  }
}

// out[c][t] = (ADD ? out[c][t] : 0) + sum_chunk partial[c][chunk][t] mod q2: every partial is canonical
// (< q2), and so is out when it is added to, so the running sum stays canonical with one conditional
// subtraction per term, for any chunk count.
template <bool ADD>
__device__ __forceinline__ void sum_partials(const uint64_t *__restrict__ partial, int chunks, int n_ct,
                                             uint64_t *__restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n_ct * 2 * N2) return;
  const size_t c = idx / (2 * N2), t = idx % (2 * N2);
  uint64_t s = ADD ? out[idx] : 0;
  for (int k = 0; k < chunks; ++k) {
    s += partial[((size_t)c * chunks + k) * 2 * N2 + t];
    s = s >= Q2 ? s - Q2 : s;
  }
  out[idx] = s;
}
__global__ void reduce_partials_kernel(const uint64_t *__restrict__ partial, int chunks,
                                       int n_ct, uint64_t *__restrict__ out) {
  sum_partials<false>(partial, chunks, n_ct, out);
}
// The digest session's running sum, and omr_digest_merge with chunks = 1.
__global__ void accumulate_partials_kernel(const uint64_t *__restrict__ partial, int chunks,
                                           int n_ct, uint64_t *__restrict__ digest) {
  sum_partials<true>(partial, chunks, n_ct, digest);
}

}  // namespace omr
