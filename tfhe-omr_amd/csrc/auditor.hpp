// The auditor (include/omr_gpu.h, omr_auditor_*): the client-side owner of the level-2 secret on one device.
// Shared by the translation units that run on it: audit.hip (audit_kernel, compact expansion, key audit) and
// retrieve_device.hip (the mod-257 solver and retrieval). Calls on one auditor are serialised by `mu`.
#pragma once

#include <mutex>
#include <vector>

#include "hip_util.hpp"

struct omr_auditor {
  int device = 0;
  int num_cu = 0;
  unsigned grid = 0;    // workgroups; 0: two per compute unit (audit_kernel), six (expand_kernel)
  size_t staging = 0;   // ciphertexts per piece of omr_audit; 0: AUDIT_DEFAULT_STAGING
  double ninv = 0.0;    // N2^-1 mod q2, centred
  omr::DevBuf<double> s2_ntt, itw, tw;  // tw: the forward twiddles, for expand_kernel only
  // omr_audit's own stream and buffers (grown on demand, reused by later calls)
  hipStream_t st = nullptr;
  omr::DevBuf<uint64_t> stage;
  omr::DevBuf<uint32_t> packed;  // omr_audit_compact's piece of compact ciphertexts, expanded into `stage`
  omr::DevBuf<omr_ct_audit> records;
  omr::DevBuf<uint16_t> decoded;
  omr::DevBuf<omr_audit_summary> summary;
  // Key audit: the pack's secrets (host copies taken at creation) and, built by ensure_key_material on the
  // first key-audit call, the level-1 tables, NTT(s1), the coefficient forms and the sigma_g(s2) table.
  struct KeyMaterial {
    std::vector<uint8_t> h_s0, h_sint;
    std::vector<int8_t> h_s1, h_s2;
    std::vector<uint64_t> h_s1_ntt;
    bool ready = false;
    double ninv1 = 0.0;
    omr::DevBuf<double> tw1, itw1, s1_ntt;
    omr::DevBuf<int8_t> s1, s2, sigma;
    omr::DevBuf<uint8_t> s0, sint;
    omr::DevBuf<omr_key_audit_summary> summary;
  } key;
  // Solve mod 257 (retrieve_device.hip): the augmented matrix and the pivot rows of a solve. One call's
  // kernels own them at a time: `free` is recorded behind every call on `stream`, a call on another stream
  // waits for it, and growing waits for it on the host.
  struct Solve {
    omr::DevBuf<uint16_t> aug;
    omr::DevBuf<uint32_t> pivots;
    hipEvent_t free = nullptr;
    hipStream_t stream = nullptr;
    bool used = false;        // `free` has been recorded
    bool profile = false;     // omr_solve_profile: events around every step of later solves
    std::vector<hipEvent_t> events;  // profile: n_events recorded by the last solve, one per step boundary
    std::vector<int> steps;          // profile: the step (0..3) between events i and i + 1
  } solve;
  // Retrieval on the auditor (retrieve_device.hip): decoded ciphertexts, the system and its solution, all
  // on `st` (idle between calls)
  struct Retrieve {
    omr::DevBuf<uint16_t> decoded, matrix, rhs, solution;
    omr::DevBuf<uint64_t> indices;
    omr::DevBuf<uint32_t> status;
  } ret;
  std::mutex mu;

  ~omr_auditor() {
    for (hipEvent_t e : solve.events) (void)hipEventDestroy(e);
    if (solve.free) (void)hipEventDestroy(solve.free);
    if (st) (void)hipStreamDestroy(st);
  }
};

namespace omr {

// audit.hip: n ciphertexts from host memory (full for bits = 0, compact otherwise) staged in pieces on
// aud->st, decoded by audit_kernel into the device buffer d_decoded u16 [n][2048]; `summary` (host, may be
// NULL) is added into. Returns after the stream has finished. The caller holds aud->mu, has selected the
// device and has validated bits.
omr_status audit_decode_to_device(omr_auditor *aud, const void *src, size_t n, int bits, uint16_t *d_decoded,
                                  omr_audit_summary *summary, const char *who);

}  // namespace omr
