// Auditor (include/omr_gpu.h, omr_auditor_* / omr_audit*): the client-side owner of the level-2 secret on
// one device and of audit_kernel (audit_kernels.hpp), which decrypts, decodes, classifies and
// noise-audits NttRlweCiphertexts where they are. The auditor owns NTT(s2), the inverse twiddles and,
// for the host entry point, the staging and result buffers; it needs no detector context. The CPU
// statement of the same results is omr_audit_cpu (retriever.hip). For compact ciphertexts (include/omr_gpu.h,
// "Compact ciphertexts") it also owns the forward twiddles: omr_compact_expand_device and
// omr_audit_compact run expand_kernel through compact.hpp, the latter in front of audit_kernel.
#include <algorithm>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "audit_kernels.hpp"
#include "compact.hpp"
#include "hip_util.hpp"
#include "host_tables.hpp"

using namespace omr;

struct omr_auditor {
  int device = 0;
  int num_cu = 0;
  unsigned grid = 0;    // workgroups; 0: two per compute unit (audit_kernel), six (expand_kernel)
  size_t staging = 0;   // ciphertexts per piece of omr_audit; 0: AUDIT_DEFAULT_STAGING
  double ninv = 0.0;    // N2^-1 mod q2, centred
  DevBuf<double> s2_ntt, itw, tw;  // tw: the forward twiddles, for expand_kernel only
  // omr_audit's own stream and buffers (grown on demand, reused by later calls)
  hipStream_t st = nullptr;
  DevBuf<uint64_t> stage;
  DevBuf<uint32_t> packed;  // omr_audit_compact's piece of compact ciphertexts, expanded into `stage`
  DevBuf<omr_ct_audit> records;
  DevBuf<uint16_t> decoded;
  DevBuf<omr_audit_summary> summary;
  std::mutex mu;

  ~omr_auditor() {
    if (st) (void)hipStreamDestroy(st);
  }
};

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

// The host entry points: n ciphertexts from host memory in pieces, full (bits = 0, src u64 [n][2][N2]) or
// compact (src n x 512 bits bytes, expanded on the device in front of audit_kernel).
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
    hipError_t e = hipMemcpyAsync(d_src, (const uint8_t *)src + o * src_bytes, k * src_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && bits)
      s = launch_expand(aud->packed, k, bits, aud->tw, compact_grid(aud->grid, aud->num_cu, k), aud->stage, st);
    if (e == hipSuccess && s == OMR_OK)
      s = launch_audit(aud, aud->stage, k, records ? aud->records.get() : nullptr,
                       decoded ? aud->decoded.get() : nullptr, summary ? aud->summary.get() : nullptr, st);
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

}  // namespace

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
