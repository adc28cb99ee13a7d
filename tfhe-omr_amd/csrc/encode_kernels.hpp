// Digest encoding kernels: encode_pertinent_indices (detector.rs:223-339) and
// encode_pertinent_payloads (detector.rs:341-453). Each workgroup folds a chunk of messages into
// one partial RLWE digest in registers; a second kernel sums the chunk partials mod q2 (the
// reference's rayon `.reduce(add_element_wise)`, :333-336 / :445-448).
#pragma once

#include "kernels.hpp"

namespace omr {

struct EncodeLayout {  // RetrievalParams (retrieval_params.rs:50-106)
  int index_slots, slots_per_bucket, slots_per_segment, segment_per_cipher;
};

__device__ __forceinline__ double centred_lift(uint32_t v) {
  // v < half_p ? v : q - p + v  (detector.rs:294,431), as a centred residue
  return v < (uint32_t)(P + 1) / 2 ? (double)v : (double)v - (double)P;
}

// grid (chunks, n_ct); partial [n_ct][chunks][2][N2] canonical u64.
__global__ __launch_bounds__(ENC_T) void encode_indices_kernel(
    const uint64_t *__restrict__ pv, int D, uint64_t offset, EncodeLayout ly, uint64_t seed,
    uint32_t first_ct, int per_wg, const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  using M = Mod<2>;
  constexpr int T = ENC_T, E = ENC_E, N = N2;
  using NTT = WgNtt<M, T, E>;
  __shared__ double xch[NTT::LDS_DOUBLES];
  __shared__ uint8_t buckets[ENC_T][8];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x, cti = blockIdx.y;
  const uint32_t ct = first_ct + cti;
  const int m0 = chunk * per_wg;
  const int mcount = min(per_wg, D - m0);
  double accA[E], accB[E];
#pragma unroll
  for (int e = 0; e < E; ++e) accA[e] = accB[e] = 0.0;
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
      NTT::fwd(x, xch, tw, tid);
      const uint64_t *pa = pv + (size_t)(m0 + mi) * 2 * N + tid * E;
      const uint64_t *pb = pa + N;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        accA[e] = red<M>(accA[e] + mm<M>(from_u64<M>(pa[e]), x[e]));
        accB[e] = red<M>(accB[e] + mm<M>(from_u64<M>(pb[e]), x[e]));
      }
    }
  }
  uint64_t *o = partial + ((size_t)cti * gridDim.x + chunk) * 2 * N + tid * E;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    o[e] = to_u64<M>(canon<M>(accA[e]));
    o[N + e] = to_u64<M>(canon<M>(accB[e]));
  }
}

// grid (chunks, n_ct). weights [n_ct*per_ct][all] u16 (global index), payloads [D][612] u16.
__global__ __launch_bounds__(ENC_T) void encode_payloads_kernel(
    const uint64_t *__restrict__ pv, const uint16_t *__restrict__ payloads, int D, uint64_t offset,
    uint64_t all, const uint16_t *__restrict__ weights, int per_ct, int per_wg,
    const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  using M = Mod<2>;
  constexpr int T = ENC_T, E = ENC_E, N = N2;
  using NTT = WgNtt<M, T, E>;
  __shared__ double xch[NTT::LDS_DOUBLES];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x, c = blockIdx.y;
  const int m0 = chunk * per_wg;
  const int mcount = min(per_wg, D - m0);
  double accA[E], accB[E];
#pragma unroll
  for (int e = 0; e < E; ++e) accA[e] = accB[e] = 0.0;
#pragma unroll 1
  for (int mi = 0; mi < mcount; ++mi) {
    const int m = m0 + mi;
    const uint64_t gi = offset + m;
    double x[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int pos = tid + e * T;
      const int j = pos / PAYLOAD_LEN;
      double v = 0.0;
      if (j < per_ct) {
        const int l = pos - j * PAYLOAD_LEN;
        const uint32_t w = weights[(size_t)(c * per_ct + j) * all + gi];
        v = centred_lift(((uint32_t)payloads[(size_t)m * PAYLOAD_LEN + l] * w) % (uint32_t)P);
      }
      x[e] = v;
    }
    NTT::fwd(x, xch, tw, tid);
    const uint64_t *pa = pv + (size_t)m * 2 * N + tid * E;
    const uint64_t *pb = pa + N;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      accA[e] = red<M>(accA[e] + mm<M>(from_u64<M>(pa[e]), x[e]));
      accB[e] = red<M>(accB[e] + mm<M>(from_u64<M>(pb[e]), x[e]));
    }
  }
  uint64_t *o = partial + ((size_t)c * gridDim.x + chunk) * 2 * N + tid * E;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    o[e] = to_u64<M>(canon<M>(accA[e]));
    o[N + e] = to_u64<M>(canon<M>(accB[e]));
  }
}

// encode_payloads_kernel with indexed weights (common.hpp, indexed_weight_block): the same grid, the
// same accumulation and the same partials, and no weight table. Ciphertext first_ct + blockIdx.y holds
// the combinations (first_ct + blockIdx.y) * per_ct + j, j < per_ct; one at or beyond `combos` is padding
// with weight 0. Per staged block of at most ENC_T messages, thread t < per_ct * nblk computes the one
// ChaCha12 block of (combination t / nblk, 16-message block t % nblk) into LDS, nblk <= ENC_T / 16 + 1
// being the 16-message blocks that the staged range of global indices touches.
constexpr int ENC_W_PER_CT = N2 / PAYLOAD_LEN;        // 3: the most combinations a ciphertext holds
constexpr int ENC_W_BLOCKS = ENC_T / 16 + 1;          // 9
static_assert(ENC_W_PER_CT * ENC_W_BLOCKS <= ENC_T, "one thread per staged weight block");
__global__ __launch_bounds__(ENC_T) void encode_payloads_indexed_kernel(
    const uint64_t *__restrict__ pv, const uint16_t *__restrict__ payloads, int D, uint64_t offset,
    WeightKey key, uint32_t combos, uint32_t first_ct, int per_ct, int per_wg,
    const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  using M = Mod<2>;
  constexpr int T = ENC_T, E = ENC_E, N = N2;
  using NTT = WgNtt<M, T, E>;
  __shared__ double xch[NTT::LDS_DOUBLES];
  __shared__ uint16_t wts[ENC_W_PER_CT][ENC_W_BLOCKS * 16];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x, c = blockIdx.y;
  const int m0 = chunk * per_wg;
  const int mcount = min(per_wg, D - m0);
  const uint64_t combo0 = ((uint64_t)first_ct + (uint64_t)c) * (uint64_t)per_ct;
  double accA[E], accB[E];
#pragma unroll
  for (int e = 0; e < E; ++e) accA[e] = accB[e] = 0.0;
  // per_wg may exceed ENC_T (large D): the weights are staged ENC_T messages at a time
#pragma unroll 1
  for (int mb = 0; mb < mcount; mb += ENC_T) {
    const int cnt = min(ENC_T, mcount - mb);
    const uint64_t g0 = offset + m0 + mb;
    const uint64_t blk0 = g0 >> 4;
    const int nblk = (int)(((g0 + cnt - 1) >> 4) - blk0) + 1;
    const int lane0 = (int)(g0 & 15);  // the first staged message's place in its 16-message block
    __syncthreads();  // every thread has finished reading the previous block's weights
    if (tid < per_ct * nblk) {
      const int j = tid / nblk, b = tid - j * nblk;
      uint16_t *dst = &wts[j][b * 16];
      if (combo0 + j < (uint64_t)combos) {
        indexed_weight_block(key, (uint32_t)(combo0 + j), blk0 + b, dst);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[i] = 0;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int mi = mb; mi < mb + cnt; ++mi) {
      const int m = m0 + mi;
      const int wi = lane0 + (mi - mb);
      double x[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int pos = tid + e * T;
        const int j = pos / PAYLOAD_LEN;
        double v = 0.0;
        if (j < per_ct) {
          const int l = pos - j * PAYLOAD_LEN;
          const uint32_t w = wts[j][wi];
          v = centred_lift(((uint32_t)payloads[(size_t)m * PAYLOAD_LEN + l] * w) % (uint32_t)P);
        }
        x[e] = v;
      }
      NTT::fwd(x, xch, tw, tid);
      const uint64_t *pa = pv + (size_t)m * 2 * N + tid * E;
      const uint64_t *pb = pa + N;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        accA[e] = red<M>(accA[e] + mm<M>(from_u64<M>(pa[e]), x[e]));
        accB[e] = red<M>(accB[e] + mm<M>(from_u64<M>(pb[e]), x[e]));
      }
    }
  }
  uint64_t *o = partial + ((size_t)c * gridDim.x + chunk) * 2 * N + tid * E;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    o[e] = to_u64<M>(canon<M>(accA[e]));
    o[N + e] = to_u64<M>(canon<M>(accB[e]));
  }
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

// encode_payloads_indexed_kernel with the reference's weights found through a seek (common.hpp,
// "Reference payload weights by seek"): the same grid, accumulation and partials, the same bits as
// encode_payloads_kernel over omr_payload_weights' table. Row j of the board starts at draw j * all, so the
// staged messages g0 .. g0 + cnt - 1 of combination j are the draws n0 = j * all + g0 onward, at the raw
// positions pos(n0) .. pos(n0 + cnt - 1) <= pos(n0) + cnt - 1 + OMR_WEIGHT_SEEK_MAX: with the first one
// anywhere in its block, at most ENC_SEEK_WORDS raw words in ENC_SEEK_BLOCKS ChaCha blocks from block
// pos(n0) >> 4. Thread t < per_ct * ENC_SEEK_BLOCKS computes block t % ENC_SEEK_BLOCKS of combination
// t / ENC_SEEK_BLOCKS and writes each accepted word to the place of its draw, wts[j][draw - n0]: the LDS
// holds the staged messages' weights in message order (rejected words dropped), and the accumulation
// loop is the indexed kernel's.
constexpr int ENC_SEEK_WORDS = ENC_T + 15 + OMR_WEIGHT_SEEK_MAX;  // 175: the most raw words one staged row spans
constexpr int ENC_SEEK_BLOCKS = (ENC_SEEK_WORDS + 15) / 16;       // 11
static_assert(ENC_SEEK_BLOCKS * 16 >= ENC_SEEK_WORDS, "the staged blocks cover the raw span of a row");
static_assert(ENC_W_PER_CT * ENC_SEEK_BLOCKS <= ENC_T, "one thread per staged raw block");
__global__ __launch_bounds__(ENC_T) void encode_payloads_seek_kernel(
    const uint64_t *__restrict__ pv, const uint16_t *__restrict__ payloads, int D, uint64_t offset, uint64_t all,
    WeightKey key, omr_weight_seek seek, uint32_t combos, uint32_t first_ct, int per_ct, int per_wg,
    const double *__restrict__ tw, uint64_t *__restrict__ partial) {
  using M = Mod<2>;
  constexpr int T = ENC_T, E = ENC_E, N = N2;
  using NTT = WgNtt<M, T, E>;
  __shared__ double xch[NTT::LDS_DOUBLES];
  __shared__ uint16_t wts[ENC_W_PER_CT][ENC_T];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x, c = blockIdx.y;
  const int m0 = chunk * per_wg;
  const int mcount = min(per_wg, D - m0);
  const uint64_t combo0 = ((uint64_t)first_ct + (uint64_t)c) * (uint64_t)per_ct;
  double accA[E], accB[E];
#pragma unroll
  for (int e = 0; e < E; ++e) accA[e] = accB[e] = 0.0;
  // per_wg may exceed ENC_T (large D): the weights are staged ENC_T messages at a time
#pragma unroll 1
  for (int mb = 0; mb < mcount; mb += ENC_T) {
    const int cnt = min(ENC_T, mcount - mb);
    const uint64_t g0 = offset + m0 + mb;
    __syncthreads();  // every thread has finished reading the previous block's weights
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
    __syncthreads();
#pragma unroll 1
    for (int mi = mb; mi < mb + cnt; ++mi) {
      const int m = m0 + mi;
      const int wi = mi - mb;
      double x[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int pos = tid + e * T;
        const int j = pos / PAYLOAD_LEN;
        double v = 0.0;
        if (j < per_ct) {
          const int l = pos - j * PAYLOAD_LEN;
          const uint32_t w = wts[j][wi];
          v = centred_lift(((uint32_t)payloads[(size_t)m * PAYLOAD_LEN + l] * w) % (uint32_t)P);
        }
        x[e] = v;
      }
      NTT::fwd(x, xch, tw, tid);
      const uint64_t *pa = pv + (size_t)m * 2 * N + tid * E;
      const uint64_t *pb = pa + N;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        accA[e] = red<M>(accA[e] + mm<M>(from_u64<M>(pa[e]), x[e]));
        accB[e] = red<M>(accB[e] + mm<M>(from_u64<M>(pb[e]), x[e]));
      }
    }
  }
  uint64_t *o = partial + ((size_t)c * gridDim.x + chunk) * 2 * N + tid * E;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    o[e] = to_u64<M>(canon<M>(accA[e]));
    o[N + e] = to_u64<M>(canon<M>(accB[e]));
  }
}

// The builders' scan (omr_weight_seek_build_device): one ChaCha12 block of the reference stream per thread
// and grid-stride step, its 16 words compared with the zone. A rejected word at a raw position <= last takes
// a slot of the list with one atomic; only the first SEEK_LIST slots exist, and the count says whether
// the list is complete (common.hpp, SEEK_LIST). hits[0] is the count, hits[1 ..] the list.
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

// out[c][t] = sum_chunk partial[c][chunk][t] mod q2: every partial is canonical (< q2), so the
// running sum stays canonical with one conditional subtraction per term, for any chunk count.
__global__ void reduce_partials_kernel(const uint64_t *__restrict__ partial, int chunks,
                                       int n_ct, uint64_t *__restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n_ct * 2 * N2) return;
  const size_t c = idx / (2 * N2), t = idx % (2 * N2);
  uint64_t s = 0;
  for (int k = 0; k < chunks; ++k) {
    s += partial[((size_t)c * chunks + k) * 2 * N2 + t];
    s = s >= Q2 ? s - Q2 : s;
  }
  out[idx] = s;
}

// digest[c][t] = (digest[c][t] + sum_chunk partial[c][chunk][t]) mod q2 (the digest session's
// running sum, and omr_digest_merge with chunks = 1): canonical in, canonical out, as above.
__global__ void accumulate_partials_kernel(const uint64_t *__restrict__ partial, int chunks,
                                           int n_ct, uint64_t *__restrict__ digest) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)n_ct * 2 * N2) return;
  const size_t c = idx / (2 * N2), t = idx % (2 * N2);
  uint64_t s = digest[idx];
  for (int k = 0; k < chunks; ++k) {
    s += partial[((size_t)c * chunks + k) * 2 * N2 + t];
    s = s >= Q2 ? s - Q2 : s;
  }
  digest[idx] = s;
}

}  // namespace omr
