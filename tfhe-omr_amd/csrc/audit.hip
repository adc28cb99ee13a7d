// Auditor (include/omr_gpu.h, omr_auditor_* / omr_audit*): the client-side owner of the level-2 secret on
// one device and of audit_kernel (audit_kernels.hpp), which decrypts, decodes, classifies and
// noise-audits NttRlweCiphertexts where they are. The auditor owns NTT(s2), the inverse twiddles and,
// for the host entry point, the staging and result buffers; it needs no detector context. The CPU
// statement of the same results is omr_audit_cpu (retriever.hip). For compact ciphertexts (include/omr_gpu.h,
// "Compact ciphertexts") it also owns the forward twiddles: omr_compact_expand_device and
// omr_audit_compact run expand_kernel through compact.hpp, the latter in front of audit_kernel.
// The key audit (include/omr_gpu.h, "Key audit"; key_audit_kernels.hpp) runs here too: the auditor keeps a
// host copy of the pack's small secrets and, from its first key-audit call on, their device forms.
// struct omr_auditor itself is in auditor.hpp, shared with retrieve_device.hip (the mod-257 solver and
// retrieval), which decodes through audit_decode_to_device below.
#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "audit_kernels.hpp"
#include "auditor.hpp"
#include "compact.hpp"
#include "hip_util.hpp"
#include "host_tables.hpp"
#include "key_audit_kernels.hpp"

using namespace omr;

namespace {

constexpr size_t AUDIT_DEFAULT_STAGING = 2048;  // 64 MiB of ciphertexts

// audit_kernel over n device ciphertexts on st; any output may be NULL
omr_status launch_audit(omr_auditor *aud, const uint64_t *d_cts, size_t n, omr_ct_audit *d_records,
                        uint16_t *d_decoded, omr_audit_summary *d_summary, hipStream_t st) {
  const size_t want = aud->grid ? aud->grid : 2 * (size_t)aud->num_cu;
  // slices keep a workgroup's 32-bit histogram counters in range (AUDIT_MAX_PER_WORKGROUP)
  for (size_t o = 0; o < n;) {
    const unsigned grid = (unsigned)std::min(want, n - o);
    const size_t cnt = std::min(n - o, (size_t)grid * AUDIT_MAX_PER_WORKGROUP);
    audit_kernel<<<grid, BR2_T, 0, st>>>(d_cts + o * 2 * N2, cnt, aud->s2_ntt, aud->itw, aud->ninv,
                                         d_records ? d_records + o : nullptr,
                                         d_decoded ? d_decoded + o * N2 : nullptr, d_summary);
    HIP_TRY(hipGetLastError());
    o += cnt;
  }
  return OMR_OK;
}

}  // namespace

extern "C" omr_status omr_auditor_create(const omr_secret_key_pack *sk, int device, omr_auditor **out) {
  if (!sk || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_auditor_create: NULL argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  try {
    std::unique_ptr<omr_auditor> aud(new omr_auditor);
    aud->device = device;
    HIP_TRY(hipDeviceGetAttribute(&aud->num_cu, hipDeviceAttributeMultiprocessorCount, device));
    if (aud->num_cu <= 0) return set_error(OMR_ERR_DEVICE, "omr_auditor_create: no compute units reported");
    std::vector<double> s(N2), tw, itw;
    for (int j = 0; j < N2; ++j) s[j] = centred(sk->s2_ntt[j], Q2);
    twiddles(Q2, N2, 22, tw, itw);
    aud->ninv = ninv_centred(N2, Q2);
    HIP_TRY(aud->s2_ntt.upload_sync(s));
    HIP_TRY(aud->itw.upload_sync(itw));
    HIP_TRY(aud->tw.upload_sync(tw));
    HIP_TRY(hipStreamCreateWithFlags(&aud->st, hipStreamNonBlocking));
    aud->key.h_s0.assign(sk->s0, sk->s0 + N0);
    aud->key.h_s1.assign(sk->s1, sk->s1 + N1);
    aud->key.h_sint.assign(sk->sint, sk->sint + NI);
    aud->key.h_s2.assign(sk->s2, sk->s2 + N2);
    aud->key.h_s1_ntt = sk->s1_ntt;
    *out = aud.release();
  } catch (const std::bad_alloc &) {
    return set_error(OMR_ERR_OUT_OF_MEMORY, "omr_auditor_create: host allocation failed");
  }
  return OMR_OK;
}

extern "C" void omr_auditor_destroy(omr_auditor *aud) {
  if (!aud) return;
  (void)hipSetDevice(aud->device);
  (void)hipStreamSynchronize(aud->st);
  if (aud->solve.used) (void)hipEventSynchronize(aud->solve.free);
  delete aud;
}

extern "C" omr_status omr_auditor_set_grid(omr_auditor *aud, unsigned workgroups) {
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_auditor_set_grid: NULL auditor");
  std::lock_guard<std::mutex> lk(aud->mu);
  aud->grid = workgroups;
  return OMR_OK;
}

extern "C" omr_status omr_auditor_set_staging(omr_auditor *aud, size_t max_ciphertexts) {
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_auditor_set_staging: NULL auditor");
  std::lock_guard<std::mutex> lk(aud->mu);
  aud->staging = max_ciphertexts;
  return OMR_OK;
}

extern "C" omr_status omr_audit_device(omr_auditor *aud, const uint64_t *d_cts, size_t n, omr_ct_audit *d_records,
                                       uint16_t *d_decoded, omr_audit_summary *d_summary, void *hip_stream) {
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_device: NULL auditor");
  if (!d_records && !d_decoded && !d_summary)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_device: no output requested");
  if (n == 0) return OMR_OK;
  if (!d_cts) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_device: NULL ciphertexts");
  if ((uintptr_t)d_cts % 16) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_device: ciphertexts not 16-byte aligned");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  return launch_audit(aud, d_cts, n, d_records, d_decoded, d_summary, (hipStream_t)hip_stream);
}

namespace {

// The staging loop of every host entry point: n > 0 ciphertexts from host memory in pieces on aud->st, full
// (bits = 0, src u64 [n][2][N2]) or compact (src n x 512 bits bytes, expanded on the device in front of
// audit_kernel). The decoded values go to the host (`decoded`, through the auditor's piece buffer) or stay on
// the device (`d_decoded` u16 [n][2048], written in place); records and summary go to the host. Any output may
// be NULL. Returns after the stream has finished. The caller holds aud->mu and has selected the device.
omr_status audit_pieces(omr_auditor *aud, const void *src, size_t n, int bits, omr_ct_audit *records, uint16_t *decoded,
                        uint16_t *d_decoded, omr_audit_summary *summary, const std::string &name) {
  const size_t B = std::min(n, aud->staging ? aud->staging : AUDIT_DEFAULT_STAGING);
  const size_t src_bytes = bits ? compact_ct_bytes(bits) : 2 * N2 * sizeof(uint64_t);  // per ciphertext
  hipStream_t st = aud->st;
  // the stream is idle between calls (each one ends with a synchronisation), so growing is safe here
  HIP_TRY(aud->stage.reserve(B * 2 * N2));
  if (bits) HIP_TRY(aud->packed.reserve(B * src_bytes / sizeof(uint32_t)));
  if (records) HIP_TRY(aud->records.reserve(B));
  if (decoded) HIP_TRY(aud->decoded.reserve(B * N2));
  if (summary) {
    HIP_TRY(aud->summary.reserve(1));
    HIP_TRY(hipMemsetAsync(aud->summary, 0, sizeof(omr_audit_summary), st));
  }
  void *d_src = bits ? (void *)aud->packed.get() : (void *)aud->stage.get();
  omr_status s = OMR_OK;
  for (size_t o = 0; o < n && s == OMR_OK; o += B) {
    const size_t k = std::min(B, n - o);
    uint16_t *d_dec = d_decoded ? d_decoded + o * N2 : (decoded ? aud->decoded.get() : nullptr);
    hipError_t e = hipMemcpyAsync(d_src, (const uint8_t *)src + o * src_bytes, k * src_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && bits)
      s = launch_expand(aud->packed, k, bits, aud->tw, compact_grid(aud->grid, aud->num_cu, k), aud->stage, st);
    if (e == hipSuccess && s == OMR_OK)
      s = launch_audit(aud, aud->stage, k, records ? aud->records.get() : nullptr, d_dec,
                       summary ? aud->summary.get() : nullptr, st);
    if (e == hipSuccess && s == OMR_OK && records)
      e = hipMemcpyAsync(records + o, aud->records, k * sizeof(omr_ct_audit), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && s == OMR_OK && decoded)
      e = hipMemcpyAsync(decoded + o * N2, aud->decoded, k * N2 * sizeof(uint16_t), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) s = hip_error((name + ": staging copy").c_str(), e);
  }
  omr_audit_summary got;
  if (s == OMR_OK && summary) {
    const hipError_t e = hipMemcpyAsync(&got, aud->summary, sizeof got, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) s = hip_error((name + ": summary copy").c_str(), e);
  }
  // always drain the stream: the caller's buffers and the staging must be free on return
  const hipError_t e = hipStreamSynchronize(st);
  if (s == OMR_OK && e != hipSuccess) s = hip_error((name + ": stream synchronisation").c_str(), e);
  if (s == OMR_OK && summary) merge_summary(*summary, got);
  return s;
}

// omr_audit and omr_audit_compact: the argument checks, then the pieces with every result on the host.
omr_status audit_staged(omr_auditor *aud, const void *src, size_t n, int bits, omr_ct_audit *records,
                        uint16_t *decoded, omr_audit_summary *summary, const char *who) {
  const std::string name(who);
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, name + ": NULL auditor");
  if (bits && !compact_bits_ok(bits)) return set_error(OMR_ERR_INVALID_ARGUMENT, name + ": bits must be in [16, 32]");
  if (!records && !decoded && !summary) return set_error(OMR_ERR_INVALID_ARGUMENT, name + ": no output requested");
  if (n == 0) return OMR_OK;
  if (!src) return set_error(OMR_ERR_INVALID_ARGUMENT, name + ": NULL ciphertexts");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  return audit_pieces(aud, src, n, bits, records, decoded, nullptr, summary, name);
}

}  // namespace

// The decode of retrieval on the auditor (auditor.hpp): the same pieces, the decoded values kept in the
// caller's device buffer.
omr_status omr::audit_decode_to_device(omr_auditor *aud, const void *src, size_t n, int bits, uint16_t *d_decoded,
                                       omr_audit_summary *summary, const char *who) {
  if (n == 0) return OMR_OK;
  return audit_pieces(aud, src, n, bits, nullptr, nullptr, d_decoded, summary, who);
}

extern "C" omr_status omr_audit(omr_auditor *aud, const uint64_t *cts, size_t n, omr_ct_audit *records,
                                uint16_t *decoded, omr_audit_summary *summary) {
  return audit_staged(aud, cts, n, 0, records, decoded, summary, "omr_audit");
}

extern "C" omr_status omr_audit_compact(omr_auditor *aud, const void *packed, size_t n, int bits, omr_ct_audit *records,
                                        uint16_t *decoded, omr_audit_summary *summary) {
  if (!bits) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_compact: bits must be in [16, 32]");
  return audit_staged(aud, packed, n, bits, records, decoded, summary, "omr_audit_compact");
}

extern "C" omr_status omr_compact_expand_device(omr_auditor *aud, const void *d_packed, size_t n, int bits,
                                                uint64_t *d_cts, void *hip_stream) {
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_expand_device: NULL auditor");
  if (!compact_bits_ok(bits))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_expand_device: bits must be in [16, 32]");
  if (n == 0) return OMR_OK;
  if (!d_packed || !d_cts) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_expand_device: NULL argument");
  if ((uintptr_t)d_packed % 16 || (uintptr_t)d_cts % 16)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_expand_device: buffers not 16-byte aligned");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  return launch_expand(d_packed, n, bits, aud->tw, compact_grid(aud->grid, aud->num_cu, n), d_cts, (hipStream_t)hip_stream);
}

// ==========================================================================================
// Key audit (include/omr_gpu.h, "Key audit")
// ==========================================================================================

namespace {

// The device forms of the secrets, once per auditor (blocking uploads; the caller holds aud->mu and has
// selected the device).
omr_status ensure_key_material(omr_auditor *aud) {
  omr_auditor::KeyMaterial &k = aud->key;
  if (k.ready) return OMR_OK;
  std::vector<double> s(N1), tw, itw;
  for (int j = 0; j < N1; ++j) s[j] = centred(k.h_s1_ntt[j], Q1);
  twiddles(Q1, N1, 7, tw, itw);
  k.ninv1 = ninv_centred(N1, Q1);
  // sigma_g(s2) for the 11 trace steps, as keygen_rows builds it: 22 KiB
  std::vector<int8_t> sigma((size_t)TRACE_STEPS * N2);
  for (int t = 0; t < TRACE_STEPS; ++t) {
    const uint32_t g = (uint32_t)(N2 >> t) + 1;
    for (int i = 0; i < N2; ++i) {
      const uint32_t e = (uint32_t)(((uint64_t)i * g) % (2 * N2));
      if (e < (uint32_t)N2) sigma[(size_t)t * N2 + e] = k.h_s2[i];
      else sigma[(size_t)t * N2 + e - N2] = (int8_t)-k.h_s2[i];
    }
  }
  HIP_TRY(k.s1_ntt.upload_sync(s));
  HIP_TRY(k.tw1.upload_sync(tw));
  HIP_TRY(k.itw1.upload_sync(itw));
  HIP_TRY(k.s1.upload_sync(k.h_s1));
  HIP_TRY(k.s2.upload_sync(k.h_s2));
  HIP_TRY(k.s0.upload_sync(k.h_s0));
  HIP_TRY(k.sint.upload_sync(k.h_sint));
  HIP_TRY(k.sigma.upload_sync(sigma));
  HIP_TRY(k.summary.alloc(1));
  k.ready = true;
  return OMR_OK;
}

// The kernels over `rows` device rows of a valid component starting at component row first_row.
omr_status launch_key_audit(omr_auditor *aud, int comp, const void *d_rows, size_t first_row, size_t rows, uint64_t limit,
                            uint64_t *d_row_max, omr_key_audit_summary *d_summary, hipStream_t st) {
  const omr_auditor::KeyMaterial &k = aud->key;
  if (comp == OMR_KEY_KSK) {
    // four rows (waves) per workgroup at a time; default four workgroups per compute unit
    const size_t want = aud->grid ? aud->grid : 4 * (size_t)aud->num_cu;
    const unsigned grid = (unsigned)std::min(want, (rows + KSK_AUDIT_WAVES - 1) / KSK_AUDIT_WAVES);
    key_audit_ksk_kernel<<<grid, 64 * KSK_AUDIT_WAVES, 0, st>>>((const uint32_t *)d_rows, first_row, rows, k.sint, k.s1, limit,
                                                              d_row_max, d_summary);
  } else {
    const unsigned grid = (unsigned)std::min(aud->grid ? aud->grid : 2 * (size_t)aud->num_cu, rows);
    if (comp == OMR_KEY_BSK1) {
      const KeyAuditSecrets sec{k.tw1, k.itw1, k.s1_ntt, k.ninv1, k.s1, k.s0, nullptr};
      key_audit_rlwe_kernel<1, uint32_t><<<grid, 256, 0, st>>>((const uint32_t *)d_rows, comp, first_row, rows, sec, limit,
                                                               d_row_max, d_summary);
    } else {
      const KeyAuditSecrets sec{aud->tw, aud->itw, aud->s2_ntt, aud->ninv, k.s2, k.sint, k.sigma};
      key_audit_rlwe_kernel<2, uint64_t><<<grid, 256, 0, st>>>((const uint64_t *)d_rows, comp, first_row, rows, sec, limit,
                                                               d_row_max, d_summary);
    }
  }
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// Memory of the current device (anything else, pageable host memory included, is staged).
bool on_current_device(const void *p) {
  hipPointerAttribute_t at;
  int cur = -1;
  if (hipPointerGetAttributes(&at, p) != hipSuccess || hipGetDevice(&cur) != hipSuccess) {
    (void)hipGetLastError();  // an unregistered host pointer is an error to some runtimes
    return false;
  }
  return at.type == hipMemoryTypeDevice && at.device == cur;
}

// UINT64_MAX stands for the generators' support K
uint64_t key_limit(int comp, uint64_t l) {
  if (l == UINT64_MAX) (void)omr_key_noise_support(comp, &l);
  return l;
}

// A full key on the auditor's own stream: device components where they are, host components in pieces
// through the staging buffer. The caller holds aud->mu and has selected the device.
omr_status audit_key_locked(omr_auditor *aud, const omr_detection_key_view *key, const uint64_t *limit,
                            omr_key_audit_summary *out, const char *who) {
  OMR_TRY(ensure_key_material(aud));
  hipStream_t st = aud->st;
  const void *p[4] = {key->bsk1, key->ksk, key->bsk2, key->trace_key};
  for (int c = 0; c < 4; ++c) {
    if (!p[c]) continue;
    const KeyAuditShape sh = key_audit_shape(c);
    const size_t row_bytes = (size_t)sh.row_elems * (sh.level == 1 ? 4 : 8);
    const uint64_t lim = key_limit(c, limit ? limit[c] : UINT64_MAX);
    const omr_key_audit_summary init = key_summary_init();
    omr_key_audit_summary got;
    omr_status s = OMR_OK;
    hipError_t e = hipMemcpyAsync(aud->key.summary, &init, sizeof init, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && on_current_device(p[c])) {
      if ((uintptr_t)p[c] % (sh.level == 1 ? 4 : 16)) s = set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": device component misaligned");
      else s = launch_key_audit(aud, c, p[c], 0, sh.rows, lim, nullptr, aud->key.summary, st);
    } else if (e == hipSuccess) {
      // the stream is idle between calls and synchronised after every piece, so growing is safe here
      const size_t cts = aud->staging ? aud->staging : AUDIT_DEFAULT_STAGING;
      const size_t B = std::min(sh.rows, std::max<size_t>(1, cts * 2 * N2 * sizeof(uint64_t) / row_bytes));
      e = aud->stage.reserve((B * row_bytes + 7) / 8);
      for (size_t o = 0; o < sh.rows && e == hipSuccess && s == OMR_OK; o += B) {
        const size_t n = std::min(B, sh.rows - o);
        e = hipMemcpyAsync(aud->stage, (const uint8_t *)p[c] + o * row_bytes, n * row_bytes, hipMemcpyDefault, st);
        if (e == hipSuccess) s = launch_key_audit(aud, c, aud->stage.get(), o, n, lim, nullptr, aud->key.summary, st);
        if (e == hipSuccess && s == OMR_OK) e = hipStreamSynchronize(st);  // the staging buffer is reused
      }
    }
    if (e == hipSuccess && s == OMR_OK) e = hipMemcpyAsync(&got, aud->key.summary, sizeof got, hipMemcpyDeviceToHost, st);
    // always drain the stream: the caller's buffers and the staging must be free on return
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (s == OMR_OK && e != hipSuccess) s = hip_error((std::string(who) + ": key audit").c_str(), e);
    if (s != OMR_OK) return s;
    merge_key_summary(out[c], got);
  }
  return OMR_OK;
}

template <typename W, uint64_t Q>
omr_status launch_count(const void *d_words, size_t n, uint64_t *d_count, hipStream_t st) {
  const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
  count_noncanonical_kernel<W, Q><<<grid, 256, 0, st>>>((const W *)d_words, n, (unsigned long long *)d_count);
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// the four word arrays of a key (full or bodies) in device memory -> counts on the host
omr_status validate_device(const void *const p[4], const size_t n[4], int device, uint64_t *noncanonical, const char *who) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": no such device");
  HIP_TRY(hipSetDevice(device));
  DevBuf<uint64_t> cnt;
  HIP_TRY(cnt.alloc(4));
  HIP_TRY(hipMemsetAsync(cnt, 0, 4 * sizeof(uint64_t), nullptr));
  for (int c = 0; c < 4; ++c)
    if (p[c]) OMR_TRY(omr_key_count_noncanonical_device(c < 2 ? 1 : 2, p[c], n[c], cnt.get() + c, nullptr));
  uint64_t got[4];
  HIP_TRY(hipMemcpy(got, cnt, sizeof got, hipMemcpyDeviceToHost));  // orders after the null stream's kernels
  for (int c = 0; c < 4; ++c)
    if (p[c]) noncanonical[c] = got[c];
  return OMR_OK;
}

}  // namespace

extern "C" omr_status omr_audit_key_rows_device(omr_auditor *aud, int component, const void *d_rows, size_t first_row,
                                                size_t rows, uint64_t limit, uint64_t *d_row_max,
                                                omr_key_audit_summary *d_summary, void *hip_stream) {
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_device: NULL auditor");
  const KeyAuditShape sh = key_audit_shape(component);
  if (!sh.rows) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_device: no such component");
  if (first_row > sh.rows || rows > sh.rows - first_row)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_device: row range beyond the component");
  if (!d_row_max && !d_summary) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_device: no output requested");
  if (rows == 0) return OMR_OK;
  if (!d_rows) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_device: NULL rows");
  if ((uintptr_t)d_rows % (component == OMR_KEY_KSK ? 4 : 16))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_rows_device: rows misaligned");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  OMR_TRY(ensure_key_material(aud));
  return launch_key_audit(aud, component, d_rows, first_row, rows, key_limit(component, limit), d_row_max,
                          d_summary, (hipStream_t)hip_stream);
}

extern "C" omr_status omr_audit_key(omr_auditor *aud, const omr_detection_key_view *key, const uint64_t limit[4],
                                    omr_key_audit_summary out[4]) {
  if (!aud || !key || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key: NULL argument");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  return audit_key_locked(aud, key, limit, out, "omr_audit_key");
}

extern "C" omr_status omr_audit_key_seeded(omr_auditor *aud, const omr_seeded_key_view *key, const uint64_t limit[4],
                                           omr_key_audit_summary out[4]) {
  if (!aud || !key || !out || !key->bsk1_b || !key->ksk_b || !key->bsk2_b || !key->trace_key_b)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_audit_key_seeded: NULL argument");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  // the expanded key lives for this call only
  DevBuf<uint32_t> bsk1, ksk;
  DevBuf<uint64_t> bsk2, tk;
  HIP_TRY(bsk1.alloc(BSK1_ELEMS));
  HIP_TRY(ksk.alloc(KSK_ELEMS));
  HIP_TRY(bsk2.alloc(BSK2_ELEMS));
  HIP_TRY(tk.alloc(TK_ELEMS));
  OMR_TRY(omr_expand_detection_key_device(key, bsk1, ksk, bsk2, tk, aud->st));
  const omr_detection_key_view full{bsk1, ksk, bsk2, tk};
  return audit_key_locked(aud, &full, limit, out, "omr_audit_key_seeded");
}

extern "C" omr_status omr_key_count_noncanonical_device(int level, const void *d_words, size_t n, uint64_t *d_count,
                                                        void *hip_stream) {
  if (level != 1 && level != 2) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_count_noncanonical_device: level must be 1 or 2");
  if (n == 0) return OMR_OK;
  if (!d_words || !d_count) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_count_noncanonical_device: NULL argument");
  if (level == 1) return launch_count<uint32_t, Q1>(d_words, n, d_count, (hipStream_t)hip_stream);
  return launch_count<uint64_t, Q2>(d_words, n, d_count, (hipStream_t)hip_stream);
}

extern "C" omr_status omr_key_validate_device(const omr_detection_key_view *key, int device, uint64_t noncanonical[4]) {
  if (!key || !noncanonical) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_validate_device: NULL argument");
  const void *const p[4] = {key->bsk1, key->ksk, key->bsk2, key->trace_key};
  const size_t n[4] = {BSK1_ELEMS, KSK_ELEMS, BSK2_ELEMS, TK_ELEMS};
  return validate_device(p, n, device, noncanonical, "omr_key_validate_device");
}

extern "C" omr_status omr_key_validate_seeded_device(const omr_seeded_key_view *key, int device, uint64_t noncanonical[4]) {
  if (!key || !noncanonical) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_key_validate_seeded_device: NULL argument");
  const void *const p[4] = {key->bsk1_b, key->ksk_b, key->bsk2_b, key->trace_key_b};
  const size_t n[4] = {BSK1_ELEMS / 2, (size_t)N1 * KS_DIGITS, BSK2_ELEMS / 2, TK_ELEMS / 2};
  return validate_device(p, n, device, noncanonical, "omr_key_validate_seeded_device");
}
