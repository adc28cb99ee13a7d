// Compact ciphertexts (include/omr_gpu.h, "Compact ciphertexts"): NttRlweCiphertexts switched from q2 to
// Q = 2^bits and bit-packed for the wire, 512 bits bytes each instead of 32,768. This unit owns the two
// kernels (compact_kernels.hpp) and their launches (compact.hpp), the context's entry points
// (omr_compact_cts_device, omr_compact_cts and their knobs), the CPU statement of both directions
// (omr_compact_cts_cpu, omr_compact_expand_cpu) and the residual bound. The digest session's
// omr_digest_read_compact is in digest.hip, the auditor's expansion in audit.hip.
#include <algorithm>
#include <mutex>
#include <vector>

#include "compact.hpp"
#include "compact_kernels.hpp"
#include "ctx.hpp"
#include "host_ring.hpp"
#include "host_tables.hpp"

using namespace omr;

namespace {

constexpr size_t COMPACT_DEFAULT_STAGING = 2048;  // 64 MiB of ciphertexts
constexpr size_t COMPACT_MAX_LAUNCH = (size_t)1 << 30;
// default grid: a multiple of the three workgroups per compute unit that both kernels' register budgets keep
// resident (three waves per SIMD), so that a striding grid runs in even rounds; four or two per compute
// unit measured 12-15 % slower for expand_kernel (profiles/compact/grid_sweep.json)
constexpr size_t COMPACT_WG_PER_CU = 6;

omr_status bad_bits(const char *who) {
  return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": bits must be in [16, 32]");
}

// One ciphertext of the CPU statement: coefficient form by the host NTT, the definition's quotient, the
// byte stream.
void compact_one(const uint64_t *ct, int bits, uint8_t *out) {
  const HostNtt &T = ntt2();
  std::vector<uint64_t> x(N2);
  std::vector<uint32_t> y(N2);
  for (int h = 0; h < 2; ++h) {
    for (int j = 0; j < N2; ++j) x[j] = ct[h * N2 + j] % Q2;
    T.inv(x.data());
    for (int j = 0; j < N2; ++j) y[j] = compact_rescale_wide(x[j], bits);
    compact_pack_bytes(y.data(), bits, out + (size_t)h * 256 * bits);
  }
}

void expand_one(const uint8_t *packed, int bits, uint64_t *ct) {
  const HostNtt &T = ntt2();
  std::vector<uint32_t> y(N2);
  for (int h = 0; h < 2; ++h) {
    compact_unpack_bytes(packed + (size_t)h * 256 * bits, bits, y.data());
    for (int j = 0; j < N2; ++j) ct[h * N2 + j] = compact_unscale(y[j], bits);
    T.fwd(ct + h * N2);
  }
}

}  // namespace

unsigned omr::compact_grid(unsigned grid, int num_cu, size_t n) {
  const size_t want = grid ? grid : COMPACT_WG_PER_CU * (size_t)std::max(num_cu, 1);
  return (unsigned)std::min(want, n);
}

omr_status omr::launch_compact(const uint64_t *d_cts, size_t n, int bits, const double *d_itw, unsigned grid,
                               void *d_out, hipStream_t st) {
  static const double ninv = ninv_centred(N2, Q2);
  for (size_t o = 0; o < n; o += COMPACT_MAX_LAUNCH) {
    const size_t k = std::min(COMPACT_MAX_LAUNCH, n - o);
    compact_kernel<<<(unsigned)std::min<size_t>(grid, k), BR2_T, 0, st>>>(
        d_cts + o * 2 * N2, k, bits, compact_magic(bits), d_itw, ninv, (uint32_t *)((uint8_t *)d_out + o * compact_ct_bytes(bits)));
    HIP_TRY(hipGetLastError());
  }
  return OMR_OK;
}

omr_status omr::launch_expand(const void *d_packed, size_t n, int bits, const double *d_tw, unsigned grid,
                              uint64_t *d_cts, hipStream_t st) {
  for (size_t o = 0; o < n; o += COMPACT_MAX_LAUNCH) {
    const size_t k = std::min(COMPACT_MAX_LAUNCH, n - o);
    expand_kernel<<<(unsigned)std::min<size_t>(grid, k), BR2_T, 0, st>>>(
        (const uint32_t *)((const uint8_t *)d_packed + o * compact_ct_bytes(bits)), k, bits, d_tw, d_cts + o * 2 * N2);
    HIP_TRY(hipGetLastError());
  }
  return OMR_OK;
}

extern "C" omr_status omr_compact_ct_bytes(int bits, size_t *bytes) {
  if (!bytes) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_ct_bytes: NULL argument");
  if (!compact_bits_ok(bits)) return bad_bits("omr_compact_ct_bytes");
  *bytes = compact_ct_bytes(bits);
  return OMR_OK;
}

extern "C" omr_status omr_compact_residual_bound(const omr_secret_key_pack *sk, int bits, uint64_t *R) {
  if (!sk || !R) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_residual_bound: NULL argument");
  if (!compact_bits_ok(bits)) return bad_bits("omr_compact_residual_bound");
  uint64_t l1 = 0;
  for (int j = 0; j < N2; ++j) l1 += (uint64_t)(sk->s2[j] < 0 ? -sk->s2[j] : sk->s2[j]);
  // p (1 + l1) (q2 + Q) < 2^9 2^12 2^51: a 128-bit product; the divisor 2 Q is a power of two
  const u128 num = (u128)P * (1 + l1) * (Q2 + ((uint64_t)1 << bits));
  const u128 den = (u128)2 << bits;
  *R = (uint64_t)((num + den - 1) / den);
  return OMR_OK;
}

extern "C" omr_status omr_compact_cts_cpu(const uint64_t *cts, size_t n, int bits, void *out, int nthreads) {
  if (!compact_bits_ok(bits)) return bad_bits("omr_compact_cts_cpu");
  if (n == 0) return OMR_OK;
  if (!cts || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_cts_cpu: NULL argument");
  const size_t ctb = compact_ct_bytes(bits);
  parallel_for(n, nthreads, [&](size_t m) { compact_one(cts + m * 2 * N2, bits, (uint8_t *)out + m * ctb); });
  return OMR_OK;
}

extern "C" omr_status omr_compact_expand_cpu(const void *packed, size_t n, int bits, uint64_t *cts_out, int nthreads) {
  if (!compact_bits_ok(bits)) return bad_bits("omr_compact_expand_cpu");
  if (n == 0) return OMR_OK;
  if (!packed || !cts_out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_expand_cpu: NULL argument");
  const size_t ctb = compact_ct_bytes(bits);
  parallel_for(n, nthreads, [&](size_t m) { expand_one((const uint8_t *)packed + m * ctb, bits, cts_out + m * 2 * N2); });
  return OMR_OK;
}

extern "C" omr_status omr_ctx_set_compact_grid(omr_ctx *c, unsigned workgroups) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_compact_grid: NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  c->cp.grid = workgroups;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_set_compact_staging(omr_ctx *c, size_t max_ciphertexts) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_compact_staging: NULL context");
  std::lock_guard<std::mutex> lk(c->mu);
  c->cp.staging = max_ciphertexts;
  return OMR_OK;
}

extern "C" omr_status omr_compact_cts_device(omr_ctx *c, const uint64_t *d_cts, size_t n, int bits, void *d_out,
                                             void *hip_stream) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_cts_device: NULL context");
  if (!compact_bits_ok(bits)) return bad_bits("omr_compact_cts_device");
  if (n == 0) return OMR_OK;
  if (!d_cts || !d_out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_cts_device: NULL argument");
  if ((uintptr_t)d_cts % 16 || (uintptr_t)d_out % 16)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_cts_device: buffers not 16-byte aligned");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return launch_compact(d_cts, n, bits, c->tab.tb.itw2, compact_grid(c->cp.grid, c->ho.num_cu, n), d_out,
                        (hipStream_t)hip_stream);
}

extern "C" omr_status omr_compact_cts(omr_ctx *c, const uint64_t *cts, size_t n, int bits, void *out) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_cts: NULL context");
  if (!compact_bits_ok(bits)) return bad_bits("omr_compact_cts");
  if (n == 0) return OMR_OK;
  if (!cts || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_compact_cts: NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const size_t B = std::min(n, c->cp.staging ? c->cp.staging : COMPACT_DEFAULT_STAGING), ctb = compact_ct_bytes(bits);
  hipStream_t st = c->stream;
  // the context's own stream is idle between host calls (each ends with a synchronisation): growing is safe
  HIP_TRY(c->cp.stage.reserve(B * 2 * N2));
  HIP_TRY(c->cp.packed.reserve(B * ctb / sizeof(uint32_t)));
  omr_status s = OMR_OK;
  for (size_t o = 0; o < n && s == OMR_OK; o += B) {
    const size_t k = std::min(B, n - o);
    hipError_t e = hipMemcpyAsync(c->cp.stage, cts + o * 2 * N2, k * 2 * N2 * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
      s = launch_compact(c->cp.stage, k, bits, c->tab.tb.itw2, compact_grid(c->cp.grid, c->ho.num_cu, k), c->cp.packed, st);
    if (e == hipSuccess && s == OMR_OK)
      e = hipMemcpyAsync((uint8_t *)out + o * ctb, c->cp.packed, k * ctb, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) s = hip_error("omr_compact_cts: staging copy", e);
  }
  // always drain the stream: the caller's buffers and the staging must be free on return
  const hipError_t e = hipStreamSynchronize(st);
  if (s == OMR_OK && e != hipSuccess) s = hip_error("omr_compact_cts: stream synchronisation", e);
  return s;
}
