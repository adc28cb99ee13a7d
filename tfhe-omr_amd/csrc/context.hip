// The detector context's life (struct omr_ctx, ctx.hpp): creation (tables, key conversion, bounds and
// guards), the scratch sizes, destruction, and the setters and getters of include/omr_gpu.h.
//
// Detector::new (detector.rs:85-110) -> omr_ctx_create: uploads the coefficient-domain keys,
// converts them on the GPU (BSK1 to the FFT domain x 1/512, BSK2 and the trace key to centred
// FP64 NTT-domain rows with N^-1 folded into the external-product keys and to FFT-domain limbs, the
// KSK to int8 limbs; key_convert.hpp, key_spectra.hpp) and builds the LUTs (:457-503; host_tables.hpp).
#include <algorithm>
#include <memory>
#include <vector>

#include "ctx.hpp"
#include "host_tables.hpp"
#include "key_convert.hpp"
#include "key_spectra.hpp"

using namespace omr;

namespace omr {

// Reallocating scratch: every stream that used it must be done first.
omr_status scratch_idle(omr_ctx *c) {
  if (c->scr.stream) HIP_TRY(hipEventSynchronize(c->scr.free));
  return OMR_OK;
}

omr_status ensure_batch(omr_ctx *c, size_t B) {
  const size_t ne = B * CLUES * (N1 + 1), nt = B * (N1 + 1), ni = B * (NI + 1);
  if (c->scr.ext.fits(ne) && c->scr.lwe1t.fits(nt) && c->scr.lwe_int.fits(ni)) return OMR_OK;
  OMR_TRY(scratch_idle(c));
  HIP_TRY(c->scr.ext.reserve(ne));
  HIP_TRY(c->scr.lwe1t.reserve(nt));
  HIP_TRY(c->scr.lwe_int.reserve(ni));
  return OMR_OK;
}

omr_status ensure_partial(omr_ctx *c, size_t elems) {
  if (c->scr.partial.fits(elems)) return OMR_OK;
  OMR_TRY(scratch_idle(c));
  HIP_TRY(c->scr.partial.reserve(elems));
  return OMR_OK;
}

omr_status stage_buffers(omr_ctx *c, size_t B) {
  HIP_TRY(c->scr.s_clue_a.reserve(B * N0));
  HIP_TRY(c->scr.s_clue_b.reserve(B * CLUES));
  HIP_TRY(c->scr.s_out.reserve(B * 2 * N2));
  return OMR_OK;
}

}  // namespace omr

// ------------------------------------------------------------------------------------------
// Context creation: tables, keys, bounds and guards (all on the context's stream)
// ------------------------------------------------------------------------------------------
namespace {

// Key conversion: `npoly` polynomials of N coefficients (host or device memory) go through a device
// staging buffer in chunks of 4,096 polynomials: copy, launch(staged, first polynomial, count),
// check, synchronise.
template <typename IN, typename Launch>
omr_status convert_chunked(const IN *src, size_t npoly, int N, hipStream_t st, Launch launch) {
  const size_t chunk = 4096;  // polynomials per upload
  DevBuf<IN> tmp;
  HIP_TRY(tmp.alloc(chunk * N));
  for (size_t p0 = 0; p0 < npoly; p0 += chunk) {
    const size_t n = std::min(chunk, npoly - p0);
    HIP_TRY(hipMemcpyAsync(tmp, src + p0 * N, n * N * sizeof(IN), hipMemcpyDefault, st));
    launch(tmp.get(), p0, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
  }
  return OMR_OK;
}

template <int LEVEL, typename IN, typename OUT>
omr_status convert_keys(const IN *host, size_t npoly, OUT *dev, double scale, const double *tw,
                        hipStream_t st) {
  constexpr int N = Mod<LEVEL>::N;
  constexpr int T = LEVEL == 1 ? BR1_T : BR2_T;
  return convert_chunked(host, npoly, N, st, [=](IN *tmp, size_t p0, size_t n) {
    key_to_ntt_kernel<LEVEL, IN, OUT><<<n, T, 0, st>>>(tmp, dev + p0 * N, n, scale, tw);
  });
}

omr_status convert_keys_cmux(const uint64_t *host, size_t npoly, double *dev, double scale, const double *tw2c,
                             hipStream_t st) {
  return convert_chunked(host, npoly, N2, st, [=](uint64_t *tmp, size_t p0, size_t n) {
    key_to_cmux_kernel<<<n, CmuxNtt::T, 0, st>>>(tmp, dev + p0 * N2, n, scale, tw2c);
  });
}

// BSK1 / BSK2 -> FFT-domain key spectra in double-double, rounded once (key_spectra.hpp).
template <int LEVEL, typename IN>
omr_status convert_keys_dd(const IN *host, size_t npoly, double2 *dev, hipStream_t st) {
  constexpr int N = LEVEL == 1 ? N1 : N2;
  DevBuf<CDD> tw;
  HIP_TRY(tw.upload_sync(dd_tree_twiddles(LEVEL == 1 ? 9 : 10)));
  const CDD *twp = tw;
  return convert_chunked(host, npoly, N, st, [=](IN *tmp, size_t p0, size_t n) {
    key_spectrum_dd_kernel<LEVEL><<<(unsigned)(n * (LEVEL == 1 ? 1 : 2)), KDD_T, 0, st>>>(
        tmp, dev + p0 * (LEVEL == 1 ? Fft512::N : 2 * Fft1024::n), n, twp);
  });
}

// Level 1's exact-NTT key (br1n_kernel / br1n_fallback_kernel), built on first need: when level 1
// is guarded (the exactness contract's re-run target) or run exactly. Callers hold c->mu (or own c).
omr_status ensure_bsk1n(omr_ctx *c) {
  if (c->keys.bsk1n) return OMR_OK;
  if (c->keys.bsk1_host.size() != BSK1_ELEMS)
    return set_error(OMR_ERR_DEVICE, "ensure_bsk1n: the coefficient-domain BSK1 is gone");
  DevBuf<double> key;
  HIP_TRY(key.alloc(BSK1_ELEMS));
  OMR_TRY((convert_keys<1, uint32_t, double>(c->keys.bsk1_host.data(), BSK1_ELEMS / N1, key, ninv_centred(N1, Q1),
                                             c->tab.tb.tw1, c->stream)));
  c->keys.bsk1n = std::move(key);
  std::vector<uint32_t>().swap(c->keys.bsk1_host);
  return OMR_OK;
}

omr_status create_tables(omr_ctx *c) {
  std::vector<double> tw1, itw1, tw2, itw2;
  twiddles(Q1, N1, 7, tw1, itw1);
  twiddles(Q2, N2, 22, tw2, itw2);
  auto lut1 = first_level_lut(), lut2 = second_level_lut(), tw2c = cmux_twiddles(tw2);
  std::vector<double> tabs;
  for (auto *v : {&tw1, &itw1, &tw2, &itw2, &lut1, &lut2, &tw2c}) tabs.insert(tabs.end(), v->begin(), v->end());
  omr_ctx::Tables &t = c->tab;
  HIP_TRY(t.tables.upload_sync(tabs));
  HIP_TRY(t.trace_tabs.upload_sync(trace_tables()));
  HIP_TRY(t.fft1.upload_sync(fft_twiddles()));
  HIP_TRY(t.fft2.upload_sync(fft2_twiddles()));
  t.tb.tw1 = t.tables;
  t.tb.itw1 = t.tables + N1;
  t.tb.tw2 = t.tables + 2 * N1;
  t.tb.itw2 = t.tables + 2 * N1 + N2;
  t.tb.lut1 = t.tables + 2 * N1 + 2 * N2;
  t.tb.lut2 = t.tables + 3 * N1 + 2 * N2;
  t.tb.tw2c = t.tables + 3 * N1 + 3 * N2;
  t.tb.trace_src = t.trace_tabs;
  t.tb.trace_perm = t.trace_tabs + TRACE_STEPS * N2;
  t.tb.fft1 = t.fft1;
  return OMR_OK;
}

// The coefficient-domain keys of the view (host or device memory) -> the kernels' forms.
omr_status create_keys(omr_ctx *c, const omr_detection_key_view *key) {
  omr_ctx::Keys &k = c->keys;
  HIP_TRY(k.bsk1f.alloc(BSK1_ELEMS / 2));
  HIP_TRY(k.bsk1l.alloc(BSK1_ELEMS / 2));
  HIP_TRY(k.bsk2.alloc(BSK2_ELEMS));
  HIP_TRY(k.bsk2f.alloc(BSK2_ELEMS));
  HIP_TRY(k.tk.alloc(TK_ELEMS));
  HIP_TRY(k.tkf.alloc(TK_ELEMS));
  HIP_TRY(k.kskb.alloc(KSKB_WORDS));
  const double ninv2 = ninv_centred(N2, Q2);
  hipStream_t st = c->stream;
  OMR_TRY(convert_keys_dd<1>(key->bsk1, BSK1_ELEMS / N1, k.bsk1f, st));
  bsk1_latency_layout_kernel<<<(unsigned)(BSK1_ELEMS / 2 / 256), 256, 0, st>>>(k.bsk1f, k.bsk1l, BSK1_ELEMS / 2);
  HIP_TRY(hipGetLastError());
  k.bsk1_host.resize(BSK1_ELEMS);  // for ensure_bsk1n (the view may point to host or device memory)
  HIP_TRY(hipMemcpy(k.bsk1_host.data(), key->bsk1, BSK1_ELEMS * sizeof(uint32_t), hipMemcpyDefault));
  OMR_TRY(convert_keys_cmux(key->bsk2, BSK2_ELEMS / N2, k.bsk2, ninv2, c->tab.tb.tw2c, st));
  OMR_TRY(convert_keys_dd<2>(key->bsk2, BSK2_ELEMS / N2, k.bsk2f, st));
  OMR_TRY(convert_keys_dd<2>(key->trace_key, TK_ELEMS / N2, k.tkf, st));
  OMR_TRY((convert_keys<2, uint64_t, double>(key->trace_key, TK_ELEMS / N2, k.tk, 1.0, c->tab.tb.tw2, st)));
  scale_even_rows_kernel<<<(TK_ELEMS / N2 + 1) / 2, 256, 0, st>>>(k.tk, TK_ELEMS / N2, ninv2);
  // the KSK goes to the device once, as the int8 limbs of the matrix-core key switch (88 MB)
  DevBuf<uint32_t> ksk;
  HIP_TRY(ksk.alloc(KSK_ELEMS + 64));
  HIP_TRY(hipMemcpyAsync(ksk, key->ksk, KSK_ELEMS * sizeof(uint32_t), hipMemcpyDefault, st));
  HIP_TRY(hipMemsetAsync(ksk + KSK_ELEMS, 0, 64 * sizeof(uint32_t), st));
  ksk_to_i8_kernel<<<(unsigned)((KSKB_WORDS + 255) / 256), 256, 0, st>>>(ksk, k.kskb);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return OMR_OK;
}

// kappa_r per key row (the a priori bound's key constants), the bounds they give, the guard's
// margin words and which levels the exactness contract guards.
omr_status create_bounds(omr_ctx *c) {
  const size_t rows1 = BSK1_ELEMS / 2 / Fft512::N, rows2 = BSK2_ELEMS / Fft1024::n, rowst = TK_ELEMS / Fft1024::n;
  omr_ctx::Exactness &x = c->ex;
  DevBuf<double> km;
  HIP_TRY(x.margin.alloc(GUARD_WORDS));
  HIP_TRY(km.alloc(rows1 + rows2 + rowst));
  HIP_TRY(hipMemsetAsync(x.margin, 0, GUARD_WORDS * sizeof(unsigned long long), c->stream));
  row_max_abs_kernel<<<(unsigned)rows1, 256, 0, c->stream>>>(c->keys.bsk1f, Fft512::N, km);
  row_max_abs_kernel<<<(unsigned)rows2, 256, 0, c->stream>>>(c->keys.bsk2f, Fft1024::n, km + rows1);
  row_max_abs_kernel<<<(unsigned)rowst, 256, 0, c->stream>>>(c->keys.tkf, Fft1024::n, km + rows1 + rows2);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<double> k1(rows1), k2(rows2), kt(rowst);
  HIP_TRY(hipMemcpy(k1.data(), km, rows1 * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(k2.data(), km + rows1, rows2 * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(kt.data(), km + rows1 + rows2, rowst * sizeof(double), hipMemcpyDeviceToHost));
  x.kappa[0] = *std::max_element(k1.begin(), k1.end());
  x.kappa[1] = *std::max_element(k2.begin(), k2.end());
  x.apriori[0] = apriori_bound(1, k1);
  x.apriori[1] = apriori_bound(2, k2);
  x.apriori_y = apriori_bound(3, k2);
  x.apriori_t = apriori_bound(4, kt);
  x.trace_fft = x.apriori_t < 0.5;
  // the exactness contract: a level whose bound does not prove every rounding exact is guarded
  // on every launch and checked against 1 - E (omr_ctx_exactness)
  for (int l = 0; l < 2; ++l) {
    x.guard_auto[l] = !(x.apriori[l] < 0.5);
    x.thr[l] = 1.0 - x.apriori[l];
  }
  // the FFT trace shares level 2's guard word and threshold
  if (x.trace_fft) x.thr[1] = 1.0 - std::max(x.apriori[1], x.apriori_t);
  return x.guard_auto[0] ? ensure_bsk1n(c) : OMR_OK;  // the re-run target of a guarded level 1
}

omr_status select_device(int device, const char *who) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": no such device");
  HIP_TRY(hipSetDevice(device));
  return OMR_OK;
}

// The creation path of both entry points: a context on the current device (`device`) from a full key
// in host or device memory.
omr_status create_ctx(const omr_detection_key_view *key, int device, omr_ctx **out) {
  // every early return destroys the half-built context (synchronised first, as omr_ctx_destroy does)
  std::unique_ptr<omr_ctx, decltype(&omr_ctx_destroy)> c(new omr_ctx(), &omr_ctx_destroy);
  c->device = device;
  omr_ctx::Handoff &h = c->ho;
  HIP_TRY(hipDeviceGetAttribute(&h.num_cu, hipDeviceAttributeMultiprocessorCount, device));
  int coop = 0;
  HIP_TRY(hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device));
  // OMR_COOPERATIVE=0: never use the cooperative multi-CU latency kernels (br2l_kernel and
  // trace_kernel run instead, bit-identical); see DESIGN.md §5a on the exit-time fault of
  // processes that made cooperative launches under rocprofv3
  h.coop = coop != 0 && !env_off("OMR_COOPERATIVE");
  h.br2y = !env_off("OMR_BR2Y");
  h.no_prefetch = env_off("OMR_PREFETCH");
  h.no_fast_handoff = env_off("OMR_FAST_HANDOFF");
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->scr.free, hipEventDisableTiming));
  // the context's error word (a two-CU hand-off timeout) and its pinned copy
  HIP_TRY(h.x_err.alloc(1));
  HIP_TRY(hipMemset(h.x_err, 0, sizeof(int)));
  HIP_TRY(hipHostMalloc((void **)&h.x_err_host, sizeof(int), hipHostMallocDefault));
  *h.x_err_host = 0;
  OMR_TRY(create_tables(c.get()));
  OMR_TRY(create_keys(c.get(), key));
  OMR_TRY(create_bounds(c.get()));
  HIP_TRY(c->scr.ks_part.alloc((size_t)KS_SPLIT * 64 * KSM_COLS * KSM_LIMBS));
  OMR_TRY(ensure_batch(c.get(), c->batch));
  *out = c.release();
  return OMR_OK;
}

}  // namespace

extern "C" omr_status omr_ctx_create(const omr_detection_key_view *key, int device, omr_ctx **out) {
  if (!key || !out || !key->bsk1 || !key->ksk || !key->bsk2 || !key->trace_key)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_create: NULL key component");
  OMR_TRY(select_device(device, "omr_ctx_create"));
  return create_ctx(key, device, out);
}

extern "C" omr_status omr_ctx_create_seeded(const omr_seeded_key_view *key, int device, omr_ctx **out) {
  if (!key || !out || !key->bsk1_b || !key->ksk_b || !key->bsk2_b || !key->trace_key_b)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_create_seeded: NULL key component");
  OMR_TRY(select_device(device, "omr_ctx_create_seeded"));
  // the expanded key lives until the context holds its own converted copy
  DevBuf<uint32_t> bsk1, ksk;
  DevBuf<uint64_t> bsk2, tk;
  HIP_TRY(bsk1.alloc(BSK1_ELEMS));
  HIP_TRY(ksk.alloc(KSK_ELEMS));
  HIP_TRY(bsk2.alloc(BSK2_ELEMS));
  HIP_TRY(tk.alloc(TK_ELEMS));
  OMR_TRY(omr_expand_detection_key_device(key, bsk1, ksk, bsk2, tk, nullptr));
  const omr_detection_key_view full{bsk1, ksk, bsk2, tk};
  return create_ctx(&full, device, out);
}

extern "C" void omr_ctx_destroy(omr_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->scr.stream) (void)hipEventSynchronize(c->scr.free);
  delete c;
}

// ------------------------------------------------------------------------------------------
// Setters and getters
// ------------------------------------------------------------------------------------------
extern "C" omr_status omr_ctx_set_batch(omr_ctx *c, size_t batch) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_batch: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->batch = batch ? batch : OMR_DEFAULT_BATCH;
  HIP_TRY(hipSetDevice(c->device));
  return ensure_batch(c, c->batch);
}

extern "C" omr_status omr_ctx_set_encode_chunks(omr_ctx *c, size_t max_chunks) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_encode_chunks: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->enc_max_chunks = max_chunks ? max_chunks : OMR_ENC_MAX_CHUNKS;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_set_latency_threshold(omr_ctx *c, size_t max_messages) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_latency_threshold: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->latency_max = max_messages;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_enable_timing(omr_ctx *c, int mode) {
  if (!c || mode < 0 || mode > 2) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_enable_timing: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  c->tm.mode = mode;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_set_rounding_guard(omr_ctx *c, int enable) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_rounding_guard: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (enable) OMR_TRY(ensure_bsk1n(c));  // a guarded level-1 launch may re-run exactly
  c->ex.guard = enable != 0;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_set_exact_level1(omr_ctx *c, int enable) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_exact_level1: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (enable) OMR_TRY(ensure_bsk1n(c));
  c->ex.exact1 = enable != 0;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_rounding_margin(omr_ctx *c, double observed[2], double apriori[2], double kappa[2],
                                              int reset) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_rounding_margin: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());  // every guarded launch on any stream has published
  unsigned long long w[2];
  HIP_TRY(hipMemcpy(w, c->ex.margin, sizeof(w), hipMemcpyDeviceToHost));
  for (int l = 0; l < 2; ++l) {
    if (observed) observed[l] = __builtin_bit_cast(double, w[l]);
    if (apriori) apriori[l] = c->ex.apriori[l];
    if (kappa) kappa[l] = c->ex.kappa[l];
  }
  if (reset) HIP_TRY(hipMemset(c->ex.margin, 0, 2 * sizeof(unsigned long long)));
  return OMR_OK;
}

extern "C" omr_status omr_ctx_exactness(omr_ctx *c, int guarded_out[2], uint64_t breaches[2]) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_exactness: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  if (guarded_out)
    for (int l = 0; l < 2; ++l) guarded_out[l] = guarded(c, l) ? 1 : 0;
  if (breaches) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long w[2];
    HIP_TRY(hipMemcpy(w, c->ex.margin + 4, sizeof(w), hipMemcpyDeviceToHost));
    breaches[0] = w[0];
    breaches[1] = w[1];
  }
  return OMR_OK;
}

extern "C" omr_status omr_fft_twiddles_dd(int level, double *out) {
  if ((level != 1 && level != 2) || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_fft_twiddles_dd: bad argument");
  const auto tw = dd_tree_twiddles(level == 1 ? 9 : 10);
  for (size_t i = 0; i < tw.size(); ++i) {
    out[4 * i] = tw[i].re.hi;
    out[4 * i + 1] = tw[i].re.lo;
    out[4 * i + 2] = tw[i].im.hi;
    out[4 * i + 3] = tw[i].im.lo;
  }
  return OMR_OK;
}

extern "C" omr_status omr_ctx_key_spectrum(omr_ctx *c, int level, size_t first, size_t count, double *out) {
  const size_t total = level == 1 ? BSK1_ELEMS / 2 : BSK2_ELEMS;  // double2 values
  if (!c || !out || (level != 1 && level != 2) || first > total || count > total - first)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_key_spectrum: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(out, (level == 1 ? c->keys.bsk1f : c->keys.bsk2f) + first, count * sizeof(double2),
                    hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_ctx_check(omr_ctx *c, void *stream) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_check: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (stream) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  } else {  // the null stream and the context's own (non-blocking) stream
    HIP_TRY(hipDeviceSynchronize());
  }
  return take_handoff_error(c);
}

extern "C" omr_status omr_ntt(int level, int inverse, uint64_t *polys, size_t n, int device) {
  if ((level != 1 && level != 2) || !polys || n == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ntt: bad argument");
  HIP_TRY(hipSetDevice(device));
  const uint64_t q = level == 1 ? Q1 : Q2;
  const int N = level == 1 ? N1 : N2;
  std::vector<double> tw, itw;
  twiddles(q, N, level == 1 ? 7 : 22, tw, itw);
  DevBuf<double> dt;
  DevBuf<uint64_t> dp;
  HIP_TRY(dt.alloc(2 * N));
  HIP_TRY(dp.alloc(n * N));
  HIP_TRY(hipMemcpy(dt, tw.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dt + N, itw.data(), N * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dp, polys, n * N * sizeof(uint64_t), hipMemcpyHostToDevice));
  const double ninv = ninv_centred(N, q);
  if (level == 1)
    ntt_u64_kernel<1><<<(unsigned)n, BR1_T>>>(dp, n, inverse, ninv, dt, dt + N);
  else
    ntt_u64_kernel<2><<<(unsigned)n, BR2_T>>>(dp, n, inverse, ninv, dt, dt + N);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(polys, dp, n * N * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}
