// Encode (detector.rs:223-453): the index and payload encode kernels' launches over the context's
// partial-sum scratch, their reduction or accumulation, and the four encode entry points; the bitmap
// digest's kernel (bitmap_kernel.hpp, none in the reference) the same way, with its two entry points;
// the payload encode with indexed weights (none in the reference), at 612 words or at a length given by the
// caller, and the device table of those weights;
// the payload encode with the reference's weights by seek and the device builder of a seek.
#include <algorithm>

#include "bitmap_kernel.hpp"
#include "ctx.hpp"
#include "encode_kernels.hpp"

using namespace omr;

namespace {
// Messages per encode workgroup: at least 32 (128 from D = 16,384), and at most max_chunks
// (default 4,096) chunk partials per ciphertext (scratch n_ct x chunks x 32 KiB: 3.7 GB for 28
// ciphertexts at D = 2^20); above ENC_T messages the index kernel stages its buckets in blocks.
int encode_per_wg(size_t D, size_t max_chunks) {
  const size_t base = D >= 16384 ? 128 : 32;
  return (int)std::max(base, (D + max_chunks - 1) / max_chunks);
}
// The shared tail of the encode bodies: after the encode kernel's launch, reduce the chunk partials
// into the n_ct output ciphertexts (or add them to a running digest).
omr_status encode_finish(omr_ctx *c, int chunks, uint32_t n_ct, uint64_t *out, hipStream_t st, bool accumulate) {
  HIP_TRY(hipGetLastError());
  if (accumulate) return accumulate_partials(c->scr.partial, chunks, n_ct, out, st);
  const size_t tot = (size_t)n_ct * 2 * N2;
  reduce_partials_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(c->scr.partial, chunks, (int)n_ct, out);
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}
// The shared body of the index and payload encodes: D messages in chunks of encode_per_wg, `launch`
// enqueues the encode kernel on grid (chunks, n_ct) over the context's partials, which are then reduced.
template <typename Launch>
omr_status encode_chunked(omr_ctx *c, size_t D, uint32_t n_ct, uint64_t *out, hipStream_t st, bool accumulate,
                          Launch launch) {
  if (D == 0) {
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_ct * 2 * N2 * sizeof(uint64_t), st));
    return OMR_OK;
  }
  const int per_wg = encode_per_wg(D, c->enc_max_chunks);
  const int chunks = (int)((D + per_wg - 1) / per_wg);
  OMR_TRY(ensure_partial(c, (size_t)n_ct * chunks * 2 * N2));
  ScratchLease lease;
  OMR_TRY(lease.acquire(c, st));
  launch(dim3(chunks, n_ct), per_wg);
  OMR_TRY(encode_finish(c, chunks, n_ct, out, st, accumulate));
  return lease.release();
}
}  // namespace

omr_status omr::accumulate_partials(const uint64_t *partial, int chunks, uint32_t n_ct, uint64_t *digest,
                                    hipStream_t st) {
  const size_t tot = (size_t)n_ct * 2 * N2;
  accumulate_partials_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(partial, chunks, (int)n_ct, digest);
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

omr_status omr::encode_indices(omr_ctx *c, const uint64_t *pv, size_t D, size_t offset, size_t all, uint64_t seed,
                               uint32_t first_ct, uint32_t n_ct, uint64_t *out, hipStream_t st, bool accumulate) {
  omr_retrieval_params rp;
  OMR_TRY(omr_get_retrieval_params(all, 0, &rp));
  EncodeLayout ly{(int)rp.index_slots_per_bucket, (int)rp.slots_per_bucket,
                  (int)rp.slots_per_segment, (int)rp.segment_per_cipher};
  return encode_chunked(c, D, n_ct, out, st, accumulate, [&](dim3 grid, int per_wg) {
    encode_indices_kernel<<<grid, ENC_T, 0, st>>>(pv, (int)D, offset, ly, seed, first_ct, per_wg, c->tab.tb.tw2,
                                                  c->scr.partial);
  });
}

omr_status omr::encode_payloads(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads, size_t D, size_t offset,
                                size_t all, const PayloadWeights &w, uint32_t first_ct, uint32_t n_ct, uint32_t per_ct,
                                uint64_t *out, hipStream_t st, bool accumulate) {
  return encode_chunked(c, D, n_ct, out, st, accumulate, [&](dim3 grid, int per_wg) {
    const double *tw = c->tab.tb.tw2;
    uint64_t *partial = c->scr.partial;
    switch (w.kind) {
      case PayloadWeights::TABLE:
        encode_payloads_kernel<<<grid, ENC_T, 0, st>>>(pv, payloads, (int)D, offset, all, w.d_table, (int)per_ct,
                                                       per_wg, tw, partial);
        break;
      case PayloadWeights::INDEXED:
        encode_payloads_indexed_kernel<<<grid, ENC_T, 0, st>>>(pv, payloads, (int)D, offset, w.key, w.combos, first_ct,
                                                               (int)per_ct, per_wg, tw, partial);
        break;
      case PayloadWeights::SEEK:
        encode_payloads_seek_kernel<<<grid, ENC_T, 0, st>>>(pv, payloads, (int)D, offset, all, w.key, w.seek, w.combos,
                                                            first_ct, (int)per_ct, per_wg, tw, partial);
        break;
      case PayloadWeights::INDEXED_LEN:
        encode_payloads_indexed_len_kernel<<<grid, ENC_T, 0, st>>>(pv, payloads, (int)D, offset, w.key, w.combos,
                                                                   first_ct, (int)w.len, (int)per_ct,
                                                                   (int)payload_stripes(w.len), per_wg, tw, partial);
        break;
    }
  });
}

omr_status omr::encode_bitmap(omr_ctx *c, const uint64_t *pv, size_t D, size_t offset, size_t all, uint64_t *out,
                              hipStream_t st, bool accumulate) {
  uint32_t n_all;
  OMR_TRY(omr_bitmap_ct_count(all, &n_all));
  constexpr size_t CT = 2 * (size_t)N2;
  if (D == 0) {
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, n_all * CT * sizeof(uint64_t), st));
    return OMR_OK;
  }
  // touched ciphertexts [c0, c1] and, per touched ciphertext, its touched slices of BMP_SLICE messages:
  // only the first and the last can have fewer than all 128
  const size_t c0 = offset / BMP_PER_CT, c1 = (offset + D - 1) / BMP_PER_CT, touched = c1 - c0 + 1;
  auto slices = [&](size_t ct) {
    const size_t lo = std::max(offset, ct * (size_t)BMP_PER_CT), hi = std::min(offset + D, (ct + 1) * (size_t)BMP_PER_CT);
    return (hi - 1) / BMP_SLICE - lo / BMP_SLICE + 1;
  };
  const size_t most = touched > 2 ? BMP_PER_CT / BMP_SLICE : std::max(slices(c0), slices(c1));
  // Slices per workgroup: as many as leave about two workgroups per compute unit (each keeps 64 KiB of
  // loads in flight; the fastest grid at every size measured), and at least what the
  // partials knob asks for. The bits do not depend on it.
  const size_t wgs1 = touched * most * BMP_SPLIT, want = 2 * (size_t)std::max(c->ho.num_cu, 1);
  const size_t spw = std::max(std::max<size_t>(1, wgs1 / want), (most + c->enc_max_chunks - 1) / c->enc_max_chunks);
  const int chunks = (int)((most + spw - 1) / spw);
  if (touched > 65535) return set_error(OMR_ERR_INVALID_ARGUMENT, "encode_bitmap: more than 65,535 ciphertexts in one call");
  OMR_TRY(ensure_partial(c, touched * chunks * CT));
  ScratchLease lease;
  OMR_TRY(lease.acquire(c, st));
  if (!accumulate) {
    if (c0) HIP_TRY(hipMemsetAsync(out, 0, c0 * CT * sizeof(uint64_t), st));
    if (c1 + 1 < n_all) HIP_TRY(hipMemsetAsync(out + (c1 + 1) * CT, 0, (n_all - c1 - 1) * CT * sizeof(uint64_t), st));
  }
  encode_bitmap_kernel<<<dim3(chunks, (unsigned)touched, BMP_SPLIT), BMP_T, 0, st>>>(pv, D, offset, c0, (int)spw,
                                                                                    c->tab.tb.tw2, c->scr.partial);
  OMR_TRY(encode_finish(c, chunks, (uint32_t)touched, out + c0 * CT, st, accumulate));
  return lease.release();
}

namespace {
// The one argument check of the three payload device entries, `source` being the entry's own weight
// arguments: n_ct is the grid's y extent, D the kernels' int.
omr_status check_payload_args(const char *who, const omr_ctx *c, const uint64_t *pv, const uint16_t *payloads,
                              bool source, size_t D, size_t offset, size_t all, uint32_t n_ct, uint32_t per_ct,
                              const uint64_t *out) {
  if (!c || !out || !source || (D && (!pv || !payloads)) || n_ct == 0 || n_ct > 65535 || per_ct == 0 ||
      per_ct * PAYLOAD_LEN > (uint32_t)N2 || !range_on_board(offset, D, all) || D > (size_t)INT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad argument");
  return OMR_OK;
}
// The three entries after their checks. stream NULL: HIP's null stream.
omr_status encode_payloads_locked(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads, size_t D, size_t offset,
                                  size_t all, const PayloadWeights &w, uint32_t first_ct, uint32_t n_ct,
                                  uint32_t per_ct, uint64_t *out, void *stream) {
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return encode_payloads(c, pv, payloads, D, offset, all, w, first_ct, n_ct, per_ct, out, (hipStream_t)stream, false);
}
// The host-buffer entries' common path: pv (and the payloads [D][len], when the entry has them) uploaded,
// run(d_pv, d_payloads, d_out) = the device entry on c->stream, and its n_ct ciphertexts downloaded once it is done.
template <typename Run>
omr_status encode_from_host(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads, size_t D, uint32_t n_ct,
                            uint64_t *out, Run run, size_t len = PAYLOAD_LEN) {
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint64_t> dpv, dout;
  DevBuf<uint16_t> dpay;
  HIP_TRY(dpv.alloc(std::max<size_t>(D, 1) * 2 * N2));
  HIP_TRY(dout.alloc((size_t)n_ct * 2 * N2));
  HIP_TRY(hipMemcpy(dpv, pv, D * 2 * N2 * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (payloads) {
    HIP_TRY(dpay.alloc(std::max<size_t>(D, 1) * len));
    HIP_TRY(hipMemcpy(dpay, payloads, D * len * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  OMR_TRY(run((const uint64_t *)dpv, (const uint16_t *)dpay, (uint64_t *)dout));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, dout, (size_t)n_ct * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}
}  // namespace

extern "C" omr_status omr_encode_indices_device(omr_ctx *c, const uint64_t *pv, size_t D,
                                                size_t offset, size_t all, uint64_t seed,
                                                uint32_t first_ct, uint32_t n_ct, uint64_t *out,
                                                void *stream) {
  // n_ct is the grid's y extent, D the kernel's int
  if (!c || !out || (D && !pv) || n_ct == 0 || n_ct > 65535 || !range_on_board(offset, D, all) ||
      D > (size_t)INT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_indices_device: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // NULL: HIP's null stream
  return encode_indices(c, pv, D, offset, all, seed, first_ct, n_ct, out, (hipStream_t)stream, false);
}

extern "C" omr_status omr_encode_payloads_device(omr_ctx *c, const uint64_t *pv,
                                                 const uint16_t *payloads, size_t D, size_t offset,
                                                 size_t all, const uint16_t *weights, uint32_t n_ct,
                                                 uint32_t per_ct, uint64_t *out, void *stream) {
  OMR_TRY(check_payload_args("omr_encode_payloads_device", c, pv, payloads, weights || !D, D, offset, all, n_ct, per_ct,
                             out));
  PayloadWeights w;
  w.d_table = weights;
  return encode_payloads_locked(c, pv, payloads, D, offset, all, w, 0, n_ct, per_ct, out, stream);
}

extern "C" omr_status omr_encode_indices(omr_ctx *c, const uint64_t *pv, size_t D, size_t offset,
                                         size_t all, uint64_t seed, uint32_t ct, uint64_t *out) {
  if (!c || !out || (D && !pv)) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_indices");
  return encode_from_host(c, pv, nullptr, D, 1, out, [&](const uint64_t *dpv, const uint16_t *, uint64_t *dout) {
    return omr_encode_indices_device(c, dpv, D, offset, all, seed, ct, 1, dout, c->stream);
  });
}

extern "C" omr_status omr_encode_payloads(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads,
                                          size_t D, size_t offset, size_t all,
                                          const uint16_t *weights, uint32_t n_ct, uint32_t per_ct,
                                          uint64_t *out) {
  if (!c || !out || (D && (!pv || !payloads || !weights)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_payloads");
  HIP_TRY(hipSetDevice(c->device));
  const size_t wn = (size_t)n_ct * per_ct * all;
  DevBuf<uint16_t> dw;
  HIP_TRY(dw.alloc(std::max<size_t>(wn, 1)));
  HIP_TRY(hipMemcpy(dw, weights, wn * sizeof(uint16_t), hipMemcpyHostToDevice));
  auto run = [&](const uint64_t *dpv, const uint16_t *dpay, uint64_t *dout) {
    return omr_encode_payloads_device(c, dpv, dpay, D, offset, all, dw, n_ct, per_ct, dout, c->stream);
  };
  return encode_from_host(c, pv, payloads, D, n_ct, out, run);
}

extern "C" omr_status omr_encode_payloads_indexed_device(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads,
                                                         size_t D, size_t offset, size_t all, const uint8_t seed[32],
                                                         uint32_t combos, uint32_t first_ct, uint32_t n_ct,
                                                         uint32_t per_ct, uint64_t *out, void *stream) {
  OMR_TRY(check_payload_args("omr_encode_payloads_indexed_device", c, pv, payloads, seed != nullptr, D, offset, all,
                             n_ct, per_ct, out));
  PayloadWeights w;
  w.kind = PayloadWeights::INDEXED, w.key = weight_key(seed), w.combos = combos;
  return encode_payloads_locked(c, pv, payloads, D, offset, all, w, first_ct, n_ct, per_ct, out, stream);
}

extern "C" omr_status omr_encode_payloads_indexed(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads, size_t D,
                                                  size_t offset, size_t all, const uint8_t seed[32], uint32_t combos,
                                                  uint32_t first_ct, uint32_t n_ct, uint32_t per_ct, uint64_t *out) {
  if (!c || !out || !seed || (D && (!pv || !payloads)) || n_ct == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_payloads_indexed");
  auto run = [&](const uint64_t *dpv, const uint16_t *dpay, uint64_t *dout) {
    return omr_encode_payloads_indexed_device(c, dpv, dpay, D, offset, all, seed, combos, first_ct, n_ct, per_ct, dout,
                                              c->stream);
  };
  return encode_from_host(c, pv, payloads, D, n_ct, out, run);
}

extern "C" omr_status omr_encode_payloads_indexed_len_device(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads,
                                                             size_t D, size_t offset, size_t all,
                                                             const uint8_t seed[32], uint32_t combos, uint32_t len,
                                                             uint32_t per_ct, uint32_t first_ct, uint32_t n_ct,
                                                             uint64_t *out, void *stream) {
  // the checks of check_payload_args, with the length's own bound on per_ct in place of per_ct * 612 <= 2048
  if (!c || !out || !seed || (D && (!pv || !payloads)) || n_ct == 0 || n_ct > 65535 || !payload_len_ok(len) ||
      per_ct == 0 || per_ct > payload_per_max(len) || !range_on_board(offset, D, all) || D > (size_t)INT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_payloads_indexed_len_device: bad argument");
  PayloadWeights w;
  w.kind = PayloadWeights::INDEXED_LEN, w.key = weight_key(seed), w.combos = combos, w.len = len;
  return encode_payloads_locked(c, pv, payloads, D, offset, all, w, first_ct, n_ct, per_ct, out, stream);
}

extern "C" omr_status omr_encode_payloads_indexed_len(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads, size_t D,
                                                      size_t offset, size_t all, const uint8_t seed[32], uint32_t combos,
                                                      uint32_t len, uint32_t per_ct, uint32_t first_ct, uint32_t n_ct,
                                                      uint64_t *out) {
  // what sizes the uploads is checked here; the device entry checks the rest before anything is enqueued
  if (!c || !out || !seed || (D && (!pv || !payloads)) || n_ct == 0 || n_ct > 65535 || !payload_len_ok(len))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_payloads_indexed_len: bad argument");
  auto run = [&](const uint64_t *dpv, const uint16_t *dpay, uint64_t *dout) {
    return omr_encode_payloads_indexed_len_device(c, dpv, dpay, D, offset, all, seed, combos, len, per_ct, first_ct,
                                                  n_ct, dout, c->stream);
  };
  return encode_from_host(c, pv, payloads, D, n_ct, out, run, len);
}

extern "C" omr_status omr_indexed_weights_table_device(const uint8_t seed[32], size_t all, uint32_t combos,
                                                       uint32_t n_ct, uint32_t per_ct, uint16_t *d_out,
                                                       void *stream) {
  const uint64_t rows = (uint64_t)n_ct * per_ct, nblk = ((uint64_t)all + 15) >> 4;
  constexpr unsigned TB = 256;
  if (!seed || !d_out || all == 0 || rows == 0 || rows < combos || rows > UINT32_MAX ||
      (rows * nblk + TB - 1) / TB > (uint64_t)INT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_indexed_weights_table_device: bad argument");
  indexed_weights_table_kernel<<<(unsigned)((rows * nblk + TB - 1) / TB), TB, 0, (hipStream_t)stream>>>(
      weight_key(seed), all, combos, (uint32_t)rows, d_out);
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

extern "C" omr_status omr_encode_payloads_seek_device(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads,
                                                      size_t D, size_t offset, size_t all, const uint8_t seed[32],
                                                      const omr_weight_seek *seek, uint32_t combos, uint32_t first_ct,
                                                      uint32_t n_ct, uint32_t per_ct, uint64_t *out, void *stream) {
  OMR_TRY(check_payload_args("omr_encode_payloads_seek_device", c, pv, payloads, seed && seek, D, offset, all, n_ct,
                             per_ct, out));
  if (!seek_covers(seek, combos, all))
    return set_error(OMR_ERR_INVALID_ARGUMENT,
                     "omr_encode_payloads_seek_device: the seek does not cover combination_count * all draws");
  PayloadWeights w;
  w.kind = PayloadWeights::SEEK, w.key = weight_key(seed), w.seek = *seek, w.combos = combos;
  return encode_payloads_locked(c, pv, payloads, D, offset, all, w, first_ct, n_ct, per_ct, out, stream);
}

extern "C" omr_status omr_encode_payloads_seek(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads, size_t D,
                                               size_t offset, size_t all, const uint8_t seed[32],
                                               const omr_weight_seek *seek, uint32_t combos, uint32_t first_ct,
                                               uint32_t n_ct, uint32_t per_ct, uint64_t *out) {
  if (!c || !out || !seed || !seek || (D && (!pv || !payloads)) || n_ct == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_payloads_seek");
  auto run = [&](const uint64_t *dpv, const uint16_t *dpay, uint64_t *dout) {
    return omr_encode_payloads_seek_device(c, dpv, dpay, D, offset, all, seed, seek, combos, first_ct, n_ct, per_ct,
                                           dout, c->stream);
  };
  return encode_from_host(c, pv, payloads, D, n_ct, out, run);
}

// The device builder of a seek: weight_seek_scan_kernel over the raw words [0, draws + OMR_WEIGHT_SEEK_MAX] on
// the current device, then the few hits sorted and turned into at[] on the host (weights.hpp, seek_from_hits).
extern "C" omr_status omr_weight_seek_build_zone_device(const uint8_t seed[32], uint64_t draws, uint32_t zone,
                                                        omr_weight_seek *out, void *stream) {
  const char *who = "omr_weight_seek_build_device";
  if (!seed || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (draws >= SEEK_MAX_DRAWS) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": draws beyond 2^62");
  hipStream_t st = (hipStream_t)stream;
  const uint64_t last = draws + OMR_WEIGHT_SEEK_MAX, nblk = (last >> 4) + 1;
  constexpr uint64_t MAX_GRID = 256 * 8;  // 8 workgroups of 256 threads per CU: the rest is the grid-stride loop
  const unsigned grid = (unsigned)std::min<uint64_t>((nblk + SEEK_SCAN_T - 1) / SEEK_SCAN_T, MAX_GRID);
  DevBuf<unsigned long long> d_hits;  // the count, then SEEK_LIST slots
  unsigned long long hits[1 + SEEK_LIST] = {};
  HIP_TRY(d_hits.alloc(1 + SEEK_LIST));
  HIP_TRY(hipMemsetAsync(d_hits, 0, sizeof hits, st));
  weight_seek_scan_kernel<<<grid, SEEK_SCAN_T, 0, st>>>(weight_key(seed), nblk, last, zone, d_hits);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hits, d_hits, sizeof hits, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint64_t list[SEEK_LIST];
  std::copy(hits + 1, hits + 1 + SEEK_LIST, list);
  return seek_from_hits(list, hits[0], draws, zone, out, who);
}

extern "C" omr_status omr_weight_seek_build_device(const uint8_t seed[32], uint64_t draws, omr_weight_seek *out,
                                                   void *stream) {
  return omr_weight_seek_build_zone_device(seed, draws, OMR_WEIGHT_ZONE, out, stream);
}

extern "C" omr_status omr_encode_bitmap_device(omr_ctx *c, const uint64_t *pv, size_t D, size_t offset, size_t all,
                                               uint64_t *out, void *stream) {
  if (!c || !out || (D && !pv) || all == 0 || offset > all || D > all - offset || D > (size_t)INT32_MAX ||
      ((uintptr_t)pv & 15) != 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_bitmap_device: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // NULL: HIP's null stream
  return encode_bitmap(c, pv, D, offset, all, out, (hipStream_t)stream, false);
}

extern "C" omr_status omr_encode_bitmap(omr_ctx *c, const uint64_t *pv, size_t D, size_t offset, size_t all,
                                        uint64_t *out) {
  uint32_t n_ct;
  if (!c || !out || (D && !pv)) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_bitmap");
  OMR_TRY(omr_bitmap_ct_count(all, &n_ct));
  return encode_from_host(c, pv, nullptr, D, n_ct, out, [&](const uint64_t *dpv, const uint16_t *, uint64_t *dout) {
    return omr_encode_bitmap_device(c, dpv, D, offset, all, dout, c->stream);
  });
}
