// Digest session (include/omr_gpu.h, omr_digest_*): the reference's board flow, detect every message,
// encode_pertinent_indices per index ciphertext, encode_pertinent_payloads (examples/omr.rs:160-203,
// detector.rs:223-453), run piece by piece inside the library. Per piece of at most the context's
// detect batch: detect into the session's pertinency buffer, both encode kernels over it, and the
// chunk partials added to the running digest mod q2. The digest is an exact sum mod q2 of
// per-message terms, so any partition of the board into updates gives the same bits. A session whose
// bitmap is enabled (omr_digest_enable_bitmap) folds each piece into the bitmap digest as well.
// omr_digest_read_compact hands the digest out in compact form (compact.hpp) and leaves it as it is.
// A session from omr_digest_begin_indexed holds no weight table: its payload encode computes the indexed
// weights (weights.hpp) in the kernel; one from omr_digest_begin_seek holds the seek of its board and the
// kernel finds the reference's weights through it; one from omr_digest_begin_indexed_len has the payload length
// as a parameter of its board ("Payload length as a board parameter"): its updates take payloads [D][len] and
// its payload digest has that layout's ciphertexts; everything else is shared.
//
// The session owns its buffers (weights, digest, pertinency chunk, host staging) and borrows the
// context's detect / encode scratch under the context mutex (ctx.hpp), like any other call.
#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "compact.hpp"
#include "ctx.hpp"
#include "digest_ranges.hpp"

using namespace omr;

struct omr_digest {
  omr_ctx *ctx;
  hipStream_t st;  // NULL: HIP's null stream
  size_t all;
  uint64_t index_seed;
  omr_retrieval_params rp;
  DevBuf<uint16_t> table;        // [payload_ct * cmb_count_per_cipher][all]; only a table session has them
  PayloadWeights weights;        // TABLE, INDEXED, SEEK, INDEXED_LEN: omr_digest_begin, _begin_indexed, _begin_seek,
                                 // _begin_indexed_len; weights.len is the words per payload of the updates
  omr_payload_layout ly;         // the payload digest's layout: rp's counts at 612 words, or the length's own
  DevBuf<uint64_t> digest;       // [index_ct + payload_ct][2][N2], canonical
  DevBuf<uint64_t> pv;           // pertinency ciphertexts of one piece, grown lazily
  DevBuf<uint64_t> merge_stage;  // omr_digest_merge's and omr_digest_merge_bitmap's upload
  DevBuf<uint64_t> bitmap;       // [n_bmp][2][N2], canonical; empty until omr_digest_enable_bitmap
  DevBuf<uint32_t> compact;      // omr_digest_read_compact's packed digest, then bitmap (grown on demand)
  uint32_t n_bmp = 0;            // omr_bitmap_ct_count(all) once the bitmap is enabled, else 0
  bool started = false;          // an update or a merge has been accepted: too late to enable the bitmap
  DevBuf<uint16_t> s_clue_a, s_clue_b, s_payloads;  // host updates' staging, grown together
  DigestRanges ranges;
  bool poisoned = false;  // a device-side failure may have reached the digest
  std::mutex mu;

  omr_digest(omr_ctx *c, hipStream_t s, size_t n, uint64_t seed) : ctx(c), st(s), all(n), index_seed(seed), ranges(n) {}
  uint32_t n_idx() const { return rp.max_encode_indices_cipher_count; }
  uint32_t n_pay() const { return rp.cmb_cipher_count; }
  size_t digest_elems() const { return (size_t)(n_idx() + n_pay()) * 2 * N2; }
};

namespace {

omr_status poisoned_error(const char *who) {
  return set_error(OMR_ERR_DEVICE, std::string(who) + ": an earlier device failure invalidated this session's digest");
}

// Room for pieces of B messages; a buffer is reallocated only once the stream is done with it.
omr_status ensure_piece(omr_digest *dg, size_t B, bool host) {
  const bool grow_pv = !dg->pv.fits(B * 2 * N2);
  const bool grow_stage = host && !(dg->s_clue_a.fits(B * N0) && dg->s_clue_b.fits(B * CLUES) &&
                                    dg->s_payloads.fits(B * dg->weights.len));
  if (!grow_pv && !grow_stage) return OMR_OK;
  HIP_TRY(hipStreamSynchronize(dg->st));
  if (grow_pv) HIP_TRY(dg->pv.reserve(B * 2 * N2));
  if (grow_stage) {
    HIP_TRY(dg->s_clue_a.reserve(B * N0));
    HIP_TRY(dg->s_clue_b.reserve(B * CLUES));
    HIP_TRY(dg->s_payloads.reserve(B * dg->weights.len));
  }
  return OMR_OK;
}

// One piece on the session's stream, the context mutex held: (stage,) detect, encode, accumulate.
omr_status run_piece(omr_digest *dg, const uint16_t *ca, const uint16_t *cb, const uint16_t *pay, size_t n,
                     size_t offset, bool host) {
  omr_ctx *c = dg->ctx;
  hipStream_t st = dg->st;
  if (host) {
    HIP_TRY(hipMemcpyAsync(dg->s_clue_a, ca, n * N0 * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dg->s_clue_b, cb, n * CLUES * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dg->s_payloads, pay, n * dg->weights.len * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    ca = dg->s_clue_a, cb = dg->s_clue_b, pay = dg->s_payloads;
  }
  OMR_TRY(detect_device(c, ca, cb, n, dg->pv, st));
  if (dg->n_bmp) OMR_TRY(encode_bitmap(c, dg->pv, n, offset, dg->all, dg->bitmap, st, true));
  OMR_TRY(encode_indices(c, dg->pv, n, offset, dg->all, dg->index_seed, 0, dg->n_idx(), dg->digest, st, true));
  uint64_t *pay_digest = dg->digest + (size_t)dg->n_idx() * 2 * N2;
  return encode_payloads(c, dg->pv, pay, n, offset, dg->all, dg->weights, 0, dg->n_pay(), dg->rp.cmb_count_per_cipher,
                         pay_digest, st, true);
}

omr_status digest_update(omr_digest *dg, const uint16_t *ca, const uint16_t *cb, const uint16_t *pay, size_t D,
                         size_t offset, bool host, const char *who) {
  if (!dg) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL session");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error(who);
  if (D && (!ca || !cb || !pay)) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (!dg->ranges.can_insert(offset, D))
    return set_error(OMR_ERR_INVALID_ARGUMENT,
                     std::string(who) + ": the range reaches beyond the board or overlaps one already folded in");
  if (D == 0) return OMR_OK;
  omr_ctx *c = dg->ctx;
  std::lock_guard<std::mutex> cl(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const size_t B = std::min(D, c->batch);
  omr_status s;
  OMR_TRY(ensure_piece(dg, B, host));  // nothing enqueued yet: the session stays usable
  dg->started = true;
  try {
    dg->ranges.insert(offset, D);
  } catch (const std::bad_alloc &) {
    return set_error(OMR_ERR_OUT_OF_MEMORY, std::string(who) + ": range bookkeeping");
  }
  for (size_t o = 0; o < D; o += B) {
    const size_t n = std::min(B, D - o);
    if ((s = run_piece(dg, ca + o * N0, cb + o * CLUES, pay + o * dg->weights.len, n, offset + o, host)) != OMR_OK) {
      dg->poisoned = true;  // part of the range may already be in the digest
      return s;
    }
  }
  if (!host) return OMR_OK;
  // as omr_detect_batch: the stream has finished with the host buffers, a failed hand-off is reported
  if (hipStreamSynchronize(dg->st) != hipSuccess) {
    dg->poisoned = true;
    return set_error(OMR_ERR_DEVICE, std::string(who) + ": stream synchronisation failed");
  }
  if ((s = take_handoff_error(c)) != OMR_OK) dg->poisoned = true;
  return s;
}

// omr_digest_begin, omr_digest_begin_indexed, omr_digest_begin_seek and omr_digest_begin_indexed_len: only the
// table session draws and uploads weights; the seek session scans the stream for its rejections on the device;
// only the INDEXED_LEN session reads payload_len, the others' payloads are 612 words in rp's layout.
omr_status digest_begin(omr_ctx *c, size_t all, size_t pertinent, uint64_t index_seed, const uint8_t weight_seed[32],
                        void *stream, omr_digest **out, PayloadWeights::Kind kind, const char *who,
                        size_t payload_len = PAYLOAD_LEN) {
  if (!c || !weight_seed || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  *out = nullptr;
  omr_retrieval_params rp;
  omr_status s;
  OMR_TRY(omr_get_retrieval_params(all, pertinent, &rp));
  omr_payload_layout ly{PAYLOAD_LEN, rp.combination_count, rp.cmb_count_per_cipher, 1, rp.cmb_cipher_count};
  if (kind == PayloadWeights::INDEXED_LEN) {
    OMR_TRY(omr_get_payload_layout(pertinent, payload_len, &ly));
    if (ly.payload_ct > 65535)  // one piece encodes them all in one launch, the grid's y extent
      return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": more than 65,535 payload ciphertexts");
    rp.cmb_count_per_cipher = ly.cmb_count_per_cipher, rp.cmb_cipher_count = ly.payload_ct;
  }
  HIP_TRY(hipSetDevice(c->device));
  try {
    std::unique_ptr<omr_digest> dg(new omr_digest(c, (hipStream_t)stream, all, index_seed));
    dg->rp = rp;
    dg->ly = ly;
    PayloadWeights &pw = dg->weights;
    pw.kind = kind;
    pw.combos = rp.combination_count;
    pw.len = ly.payload_len;
    if (kind != PayloadWeights::TABLE) {
      pw.key = weight_key(weight_seed);
      if (kind == PayloadWeights::SEEK)
        OMR_TRY(resolve_seek(weight_seed, nullptr, rp.combination_count, all, who,
                             [stream](const uint8_t *seed, uint64_t draws, omr_weight_seek *sk) {
                               return omr_weight_seek_build_device(seed, draws, sk, stream);
                             },
                             &pw.seek));
    } else {
      std::vector<uint16_t> w((size_t)rp.cmb_cipher_count * rp.cmb_count_per_cipher * all);
      if ((s = omr_payload_weights(weight_seed, all, rp.combination_count, rp.cmb_cipher_count,
                                   rp.cmb_count_per_cipher, w.data())) != OMR_OK)
        return s;
      HIP_TRY(dg->table.upload_sync(w));
      pw.d_table = dg->table;
    }
    HIP_TRY(dg->digest.alloc(dg->digest_elems()));
    HIP_TRY(hipMemsetAsync(dg->digest, 0, dg->digest_elems() * sizeof(uint64_t), dg->st));
    HIP_TRY(hipStreamSynchronize(dg->st));
    *out = dg.release();
  } catch (const std::bad_alloc &) {
    return set_error(OMR_ERR_OUT_OF_MEMORY, std::string(who) + ": host allocation failed");
  }
  return OMR_OK;
}

}  // namespace

extern "C" omr_status omr_digest_begin(omr_ctx *c, size_t all, size_t pertinent, uint64_t index_seed,
                                       const uint8_t weight_seed[32], void *stream, omr_digest **out) {
  return digest_begin(c, all, pertinent, index_seed, weight_seed, stream, out, PayloadWeights::TABLE, "omr_digest_begin");
}

extern "C" omr_status omr_digest_begin_indexed(omr_ctx *c, size_t all, size_t pertinent, uint64_t index_seed,
                                               const uint8_t weight_seed[32], void *stream, omr_digest **out) {
  return digest_begin(c, all, pertinent, index_seed, weight_seed, stream, out, PayloadWeights::INDEXED,
                      "omr_digest_begin_indexed");
}

extern "C" omr_status omr_digest_begin_indexed_len(omr_ctx *c, size_t all, size_t pertinent, uint64_t index_seed,
                                                   const uint8_t weight_seed[32], size_t payload_len, void *stream,
                                                   omr_digest **out) {
  return digest_begin(c, all, pertinent, index_seed, weight_seed, stream, out, PayloadWeights::INDEXED_LEN,
                      "omr_digest_begin_indexed_len", payload_len);
}

extern "C" omr_status omr_digest_begin_seek(omr_ctx *c, size_t all, size_t pertinent, uint64_t index_seed,
                                            const uint8_t weight_seed[32], void *stream, omr_digest **out) {
  return digest_begin(c, all, pertinent, index_seed, weight_seed, stream, out, PayloadWeights::SEEK, "omr_digest_begin_seek");
}

extern "C" omr_status omr_digest_update(omr_digest *dg, const uint16_t *ca, const uint16_t *cb,
                                        const uint16_t *payloads, size_t D, size_t offset) {
  return digest_update(dg, ca, cb, payloads, D, offset, true, "omr_digest_update");
}

extern "C" omr_status omr_digest_update_device(omr_digest *dg, const uint16_t *ca, const uint16_t *cb,
                                               const uint16_t *payloads, size_t D, size_t offset) {
  return digest_update(dg, ca, cb, payloads, D, offset, false, "omr_digest_update_device");
}

extern "C" omr_status omr_digest_merge(omr_digest *dg, const uint64_t *idx_cts, const uint64_t *pay_cts) {
  if (!dg || (!idx_cts && !pay_cts)) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_merge: NULL argument");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error("omr_digest_merge");
  const size_t ni = (size_t)dg->n_idx() * 2 * N2, np = (size_t)dg->n_pay() * 2 * N2;
  for (size_t i = 0; idx_cts && i < ni; ++i)
    if (idx_cts[i] >= Q2) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_merge: index digest value >= q2");
  for (size_t i = 0; pay_cts && i < np; ++i)
    if (pay_cts[i] >= Q2) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_merge: payload digest value >= q2");
  HIP_TRY(hipSetDevice(dg->ctx->device));
  dg->started = true;
  if (!dg->merge_stage.fits(ni + np)) {
    HIP_TRY(hipStreamSynchronize(dg->st));
    HIP_TRY(dg->merge_stage.reserve(ni + np));
  }
  // both uploads first: a failure there leaves the digest as it was
  if (idx_cts)
    HIP_TRY(hipMemcpyAsync(dg->merge_stage, idx_cts, ni * sizeof(uint64_t), hipMemcpyHostToDevice, dg->st));
  if (pay_cts)
    HIP_TRY(hipMemcpyAsync(dg->merge_stage + ni, pay_cts, np * sizeof(uint64_t), hipMemcpyHostToDevice, dg->st));
  omr_status s = OMR_OK;
  if (idx_cts) s = accumulate_partials(dg->merge_stage, 1, dg->n_idx(), dg->digest, dg->st);
  if (s == OMR_OK && pay_cts) s = accumulate_partials(dg->merge_stage + ni, 1, dg->n_pay(), dg->digest + ni, dg->st);
  if (s == OMR_OK && hipStreamSynchronize(dg->st) != hipSuccess)  // the host arrays may be reused
    s = set_error(OMR_ERR_DEVICE, "omr_digest_merge: stream synchronisation failed");
  if (s != OMR_OK) dg->poisoned = true;
  return s;
}

extern "C" omr_status omr_digest_read(omr_digest *dg, uint64_t *idx_cts, uint64_t *pay_cts) {
  if (!dg) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_read: NULL session");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error("omr_digest_read");
  std::lock_guard<std::mutex> cl(dg->ctx->mu);
  HIP_TRY(hipSetDevice(dg->ctx->device));
  HIP_TRY(hipStreamSynchronize(dg->st));
  omr_status s;
  if ((s = take_handoff_error(dg->ctx)) != OMR_OK) {
    dg->poisoned = true;
    return s;
  }
  const size_t ni = (size_t)dg->n_idx() * 2 * N2, np = (size_t)dg->n_pay() * 2 * N2;
  if (idx_cts) HIP_TRY(hipMemcpy(idx_cts, dg->digest, ni * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (pay_cts) HIP_TRY(hipMemcpy(pay_cts, dg->digest + ni, np * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_digest_read_compact(omr_digest *dg, int bits, void *idx_packed, void *pay_packed,
                                              void *bitmap_packed) {
  if (!dg) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_read_compact: NULL session");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error("omr_digest_read_compact");
  if (!compact_bits_ok(bits))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_read_compact: bits must be in [16, 32]");
  if (bitmap_packed && !dg->n_bmp)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_read_compact: the bitmap is not enabled");
  omr_ctx *c = dg->ctx;
  std::lock_guard<std::mutex> cl(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(dg->st));
  omr_status s;
  if ((s = take_handoff_error(c)) != OMR_OK) {
    dg->poisoned = true;
    return s;
  }
  // the stream is idle here, so the packed buffer may grow; the running digest is only read
  const size_t ctb = compact_ct_bytes(bits), ni = dg->n_idx(), np = dg->n_pay(), nd = ni + np;
  const size_t nb = bitmap_packed ? dg->n_bmp : 0;
  const bool want_digest = idx_packed || pay_packed;
  if (!want_digest && !nb) return OMR_OK;
  HIP_TRY(dg->compact.reserve((nd + nb) * ctb / sizeof(uint32_t)));
  uint8_t *d_digest = (uint8_t *)dg->compact.get(), *d_bitmap = d_digest + nd * ctb;
  if (want_digest)
    OMR_TRY(launch_compact(dg->digest, nd, bits, c->tab.tb.itw2, compact_grid(c->cp.grid, c->ho.num_cu, nd), d_digest, dg->st));
  if (nb)
    OMR_TRY(launch_compact(dg->bitmap, nb, bits, c->tab.tb.itw2, compact_grid(c->cp.grid, c->ho.num_cu, nb), d_bitmap, dg->st));
  HIP_TRY(hipStreamSynchronize(dg->st));
  if (idx_packed) HIP_TRY(hipMemcpy(idx_packed, d_digest, ni * ctb, hipMemcpyDeviceToHost));
  if (pay_packed) HIP_TRY(hipMemcpy(pay_packed, d_digest + ni * ctb, np * ctb, hipMemcpyDeviceToHost));
  if (nb) HIP_TRY(hipMemcpy(bitmap_packed, d_bitmap, nb * ctb, hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_digest_enable_bitmap(omr_digest *dg) {
  if (!dg) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_enable_bitmap: NULL session");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error("omr_digest_enable_bitmap");
  if (dg->n_bmp) return OMR_OK;
  if (dg->started)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_enable_bitmap: the session already has updates or merges");
  uint32_t n;
  OMR_TRY(omr_bitmap_ct_count(dg->all, &n));
  HIP_TRY(hipSetDevice(dg->ctx->device));
  const size_t elems = (size_t)n * 2 * N2;
  HIP_TRY(dg->bitmap.alloc(elems));
  HIP_TRY(hipMemsetAsync(dg->bitmap, 0, elems * sizeof(uint64_t), dg->st));
  HIP_TRY(hipStreamSynchronize(dg->st));
  dg->n_bmp = n;
  return OMR_OK;
}

extern "C" omr_status omr_digest_merge_bitmap(omr_digest *dg, const uint64_t *cts) {
  if (!dg || !cts) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_merge_bitmap: NULL argument");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error("omr_digest_merge_bitmap");
  if (!dg->n_bmp) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_merge_bitmap: the bitmap is not enabled");
  const size_t nb = (size_t)dg->n_bmp * 2 * N2;
  for (size_t i = 0; i < nb; ++i)
    if (cts[i] >= Q2) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_merge_bitmap: value >= q2");
  HIP_TRY(hipSetDevice(dg->ctx->device));
  dg->started = true;
  if (!dg->merge_stage.fits(nb)) {
    HIP_TRY(hipStreamSynchronize(dg->st));
    HIP_TRY(dg->merge_stage.reserve(nb));
  }
  // the upload first: a failure there leaves the bitmap as it was
  HIP_TRY(hipMemcpyAsync(dg->merge_stage, cts, nb * sizeof(uint64_t), hipMemcpyHostToDevice, dg->st));
  omr_status s = accumulate_partials(dg->merge_stage, 1, dg->n_bmp, dg->bitmap, dg->st);
  if (s == OMR_OK && hipStreamSynchronize(dg->st) != hipSuccess)  // the host array may be reused
    s = set_error(OMR_ERR_DEVICE, "omr_digest_merge_bitmap: stream synchronisation failed");
  if (s != OMR_OK) dg->poisoned = true;
  return s;
}

extern "C" omr_status omr_digest_read_bitmap(omr_digest *dg, uint64_t *cts) {
  if (!dg || !cts) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_read_bitmap: NULL argument");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error("omr_digest_read_bitmap");
  if (!dg->n_bmp) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_read_bitmap: the bitmap is not enabled");
  std::lock_guard<std::mutex> cl(dg->ctx->mu);
  HIP_TRY(hipSetDevice(dg->ctx->device));
  HIP_TRY(hipStreamSynchronize(dg->st));
  omr_status s;
  if ((s = take_handoff_error(dg->ctx)) != OMR_OK) {
    dg->poisoned = true;
    return s;
  }
  HIP_TRY(hipMemcpy(cts, dg->bitmap, (size_t)dg->n_bmp * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_digest_get_info(omr_digest *dg, omr_digest_info *info) {
  if (!dg || !info) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_get_info: NULL argument");
  std::lock_guard<std::mutex> lk(dg->mu);
  if (dg->poisoned) return poisoned_error("omr_digest_get_info");
  info->index_ct = dg->n_idx();
  info->payload_ct = dg->n_pay();
  info->combination_count = dg->rp.combination_count;
  info->cmb_count_per_cipher = dg->rp.cmb_count_per_cipher;
  info->all_payloads_count = dg->all;
  info->messages = dg->ranges.covered();
  info->pv_capacity_messages = dg->pv.capacity() / (2 * (size_t)N2);
  return OMR_OK;
}

extern "C" omr_status omr_digest_get_payload_layout(omr_digest *dg, omr_payload_layout *layout) {
  if (!dg || !layout) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_get_payload_layout: NULL argument");
  std::lock_guard<std::mutex> lk(dg->mu);
  *layout = dg->ly;
  return OMR_OK;
}

extern "C" omr_status omr_digest_device_bytes(omr_digest *dg, size_t *total, size_t *weights) {
  if (!dg || !total || !weights) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_digest_device_bytes: NULL argument");
  std::lock_guard<std::mutex> lk(dg->mu);
  *weights = dg->table.capacity() * sizeof(uint16_t);
  *total = *weights + (dg->digest.capacity() + dg->pv.capacity() + dg->merge_stage.capacity() + dg->bitmap.capacity()) *
                          sizeof(uint64_t) +
           dg->compact.capacity() * sizeof(uint32_t) +
           (dg->s_clue_a.capacity() + dg->s_clue_b.capacity() + dg->s_payloads.capacity()) * sizeof(uint16_t);
  return OMR_OK;
}

extern "C" void omr_digest_destroy(omr_digest *dg) {
  if (!dg) return;
  (void)hipSetDevice(dg->ctx->device);
  (void)hipStreamSynchronize(dg->st);
  delete dg;
}
