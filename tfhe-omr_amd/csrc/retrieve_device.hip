// Retrieval on the auditor (include/omr_gpu.h, "Solve mod 257"): the device solver of solve_kernels.hpp and
// the device twins of omr_retrieve_indices / omr_retrieve_payloads[_indexed] (retriever.hip). The decode is
// audit_kernel through audit.hip's audit_decode_to_device; the index buckets are read on the host from the
// decoded values copied back; the indexed or seek matrix and the right-hand side are built on the device, the
// solver runs there, and the solution and its status word are copied back.
#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "audit_decode.hpp"
#include "auditor.hpp"
#include "compact_math.hpp"
#include "retrieve_system.hpp"
#include "solve_kernels.hpp"

using namespace omr;

namespace {

constexpr unsigned col_grid(size_t n) { return (unsigned)((n + SOLVE_COL_T - 1) / SOLVE_COL_T); }

// Event bookkeeping of omr_solve_profile: one event per step boundary of the solve being enqueued.
struct StepMarks {
  omr_auditor::Solve &sv;
  hipStream_t st;
  size_t n = 0;
  omr_status mark(int step) {  // an event in front of a kernel of `step` (4: the end)
    if (!sv.profile) return OMR_OK;
    if (n == sv.events.size()) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      sv.events.push_back(e);
    }
    HIP_TRY(hipEventRecord(sv.events[n++], st));
    sv.steps.push_back(step);
    return OMR_OK;
  }
};

// The solver's kernels on st, the scratch already sized and leased to this call (launch_solve).
omr_status enqueue_solve(omr_auditor *aud, const uint16_t *d_matrix, const uint16_t *d_rhs, size_t rows, size_t cols,
                         size_t width, size_t ld, uint16_t *d_solution, uint32_t *d_status, hipStream_t st) {
  omr_auditor::Solve &sv = aud->solve;
  sv.steps.clear();
  StepMarks marks{sv, st};
  uint16_t *W = sv.aug;
  const uint32_t R = (uint32_t)rows, C = (uint32_t)cols, LD = (uint32_t)ld;
  HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), st));
  solve_load_kernel<<<col_grid(rows * ld), SOLVE_COL_T, 0, st>>>(d_matrix, d_rhs, R, C, (uint32_t)width, LD, W);
  for (uint32_t i0 = 0; i0 < C; i0 += SOLVE_PANEL) {
    const uint32_t pc = std::min<uint32_t>(SOLVE_PANEL, C - i0), k0 = i0 + pc;
    OMR_TRY(marks.mark(0));
    solve_panel_kernel<<<1, SOLVE_PANEL_T, 0, st>>>(W, R, LD, i0, pc, sv.pivots, d_status);
    OMR_TRY(marks.mark(1));
    solve_swap_kernel<<<col_grid(LD - k0), SOLVE_COL_T, 0, st>>>(W, LD, i0, pc, k0, sv.pivots, d_status);
    if (k0 < C) {  // after the last panel the rows below carry nothing that is read again
      OMR_TRY(marks.mark(2));
      const dim3 grid((LD - k0 + SOLVE_TILE_WIDTH - 1) / SOLVE_TILE_WIDTH, (R - k0 + SOLVE_TILE_ROWS - 1) / SOLVE_TILE_ROWS);
      solve_update_kernel<false><<<grid, SOLVE_UPDATE_T, 0, st>>>(W, LD, k0, R, k0, LD, i0, i0, pc, d_status);
    }
  }
  for (uint32_t b0 = (C - 1) / SOLVE_PANEL * SOLVE_PANEL;; b0 -= SOLVE_PANEL) {
    const uint32_t pb = std::min<uint32_t>(SOLVE_PANEL, C - b0);
    OMR_TRY(marks.mark(3));
    solve_back_kernel<<<col_grid(LD - C), SOLVE_COL_T, 0, st>>>(W, LD, b0, pb, C, d_status);
    if (b0 == 0) break;
    const dim3 grid((LD - C + SOLVE_TILE_WIDTH - 1) / SOLVE_TILE_WIDTH, (b0 + SOLVE_TILE_ROWS - 1) / SOLVE_TILE_ROWS);
    solve_update_kernel<true><<<grid, SOLVE_UPDATE_T, 0, st>>>(W, LD, 0, b0, C, LD, b0, b0, pb, d_status);
  }
  solve_store_kernel<<<col_grid(cols * width), SOLVE_COL_T, 0, st>>>(W, LD, C, (uint32_t)width, d_solution, d_status);
  OMR_TRY(marks.mark(4));
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// A solve on st. The caller holds aud->mu and has selected the device.
omr_status launch_solve(omr_auditor *aud, const uint16_t *d_matrix, const uint16_t *d_rhs, size_t rows, size_t cols,
                        size_t width, uint16_t *d_solution, uint32_t *d_status, hipStream_t st) {
  omr_auditor::Solve &sv = aud->solve;
  const size_t ld = (cols + width + 7) / 8 * 8;
  if (ld > UINT32_MAX / 2) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_device: width too large");
  if (!sv.free) HIP_TRY(hipEventCreateWithFlags(&sv.free, hipEventDisableTiming));
  // the scratch belongs to the previous call's kernels until `free`: grow on an idle scratch only, and
  // order a call on another stream behind them
  if (sv.used && (!sv.aug.fits(rows * ld) || !sv.pivots.fits(cols))) HIP_TRY(hipEventSynchronize(sv.free));
  HIP_TRY(sv.aug.reserve(rows * ld));
  HIP_TRY(sv.pivots.reserve(cols));
  if (sv.used && sv.stream != st) HIP_TRY(hipStreamWaitEvent(st, sv.free, 0));
  const omr_status s = enqueue_solve(aud, d_matrix, d_rhs, rows, cols, width, ld, d_solution, d_status, st);
  // whatever was enqueued, on success or not, owns the scratch until `free`; if the event cannot be recorded
  // the stream is drained instead, so that the next call never meets running kernels
  const hipError_t e = hipEventRecord(sv.free, st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    sv.used = false;
    return s != OMR_OK ? s : hip_error("omr_solve_mod257_device: hipEventRecord", e);
  }
  sv.stream = st;
  sv.used = true;
  return s;
}

}  // namespace

extern "C" omr_status omr_solve_geometry(unsigned *panel_cols, unsigned *tile_rows, unsigned *tile_width) {
  if (panel_cols) *panel_cols = SOLVE_PANEL;
  if (tile_rows) *tile_rows = SOLVE_TILE_ROWS;
  if (tile_width) *tile_width = SOLVE_TILE_WIDTH;
  return OMR_OK;
}

extern "C" omr_status omr_solve_mod257_device(omr_auditor *aud, const uint16_t *d_matrix, const uint16_t *d_rhs,
                                              size_t rows, size_t cols, size_t width, uint16_t *d_solution,
                                              uint32_t *d_status, void *hip_stream) {
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_device: NULL auditor");
  if (!d_matrix || !d_rhs || !d_solution || !d_status)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_device: NULL argument");
  if (cols < 1 || rows < cols || width < 1)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_device: needs cols >= 1, rows >= cols, width >= 1");
  if (rows > OMR_SOLVE_MAX_ROWS)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_device: more than OMR_SOLVE_MAX_ROWS (8192) rows");
  if ((uintptr_t)d_matrix % 16 || (uintptr_t)d_rhs % 16 || (uintptr_t)d_solution % 16 || (uintptr_t)d_status % 4)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_mod257_device: buffers not 16-byte aligned");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  return launch_solve(aud, d_matrix, d_rhs, rows, cols, width, d_solution, d_status, (hipStream_t)hip_stream);
}

extern "C" omr_status omr_solve_profile(omr_auditor *aud, int enable, float step_ms[4]) {
  if (!aud) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_solve_profile: NULL auditor");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  omr_auditor::Solve &sv = aud->solve;
  if (sv.used) HIP_TRY(hipEventSynchronize(sv.free));
  if (step_ms) {
    for (int s = 0; s < 4; ++s) step_ms[s] = 0.0f;
    // steps[i] is the step that runs between events i and i + 1; the last mark (4) only ends the previous one
    for (size_t i = 0; i + 1 < sv.steps.size(); ++i) {
      float ms = 0.0f;
      HIP_TRY(hipEventElapsedTime(&ms, sv.events[i], sv.events[i + 1]));
      step_ms[sv.steps[i]] += ms;
    }
  }
  sv.steps.clear();
  sv.profile = enable != 0;
  return OMR_OK;
}

// ==========================================================================================
// Retrieval
// ==========================================================================================

namespace {

// The shared front of the entry points: bits, then the decode of n_ct ciphertexts into aud->ret.decoded.
omr_status decode_cts(omr_auditor *aud, const void *cts, uint32_t n_ct, int bits, omr_audit_summary *summary,
                      const char *who) {
  HIP_TRY(aud->ret.decoded.reserve(std::max<size_t>(1, (size_t)n_ct * N2)));
  return audit_decode_to_device(aud, cts, n_ct, bits, aud->ret.decoded, summary, who);
}

// omr_retrieve_indices after its argument checks, the decoded values taken from the device. Caller holds mu.
omr_status indices_locked(omr_auditor *aud, const void *idx_cts, uint32_t n_ct, int bits, const omr_retrieval_params &rp,
                          size_t pertinent_count, size_t *indices, size_t cap, size_t *found,
                          omr_audit_summary *summary, const char *who) {
  OMR_TRY(decode_cts(aud, idx_cts, n_ct, bits, summary, who));
  std::vector<uint16_t> dec((size_t)n_ct * N2);
  if (n_ct) HIP_TRY(hipMemcpy(dec.data(), aud->ret.decoded, dec.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
  std::set<size_t> set;
  // decode_digest stops at the first ciphertext after which every pertinent index is known
  for (uint32_t c = 0; c < n_ct; ++c) {
    read_index_buckets(&dec[(size_t)c * N2], rp, set);
    if (set.size() == pertinent_count) break;
  }
  write_indices(set, indices, cap, found);
  return OMR_OK;
}

// retrieve_payloads_body's device twin after the NULL test: the same system (retrieve_system.hpp), solved on
// the device, so with a row cap; a NULL seek is built on the auditor's device.
omr_status payloads_locked(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits, size_t all,
                           uint32_t combination_count, const MatrixSource &src, const size_t *indices,
                           size_t n_indices, uint16_t *payloads, omr_audit_summary *summary, const std::string &who,
                           const omr_payload_layout *ly = nullptr) {
  PayloadSystem sys;
  OMR_TRY(payload_system(all, combination_count, n_ct, indices, n_indices, who, &sys, ly));
  if (sys.cols == 0) return OMR_OK;
  const size_t rows = sys.rows, cols = sys.cols;
  if (rows > OMR_SOLVE_MAX_ROWS)
    return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": more than OMR_SOLVE_MAX_ROWS (8192) combinations");
  omr_auditor::Retrieve &r = aud->ret;
  hipStream_t st = aud->st;
  omr_weight_seek seek{};
  if (src.by_seek)
    OMR_TRY(resolve_seek(src.weight_seed, src.seek, rows, all, who,
                         [st](const uint8_t *seed, uint64_t draws, omr_weight_seek *out) {
                           return omr_weight_seek_build_device(seed, draws, out, st);
                         },
                         &seek));
  OMR_TRY(decode_cts(aud, pay_cts, n_ct, bits, summary, who.c_str()));
  // the stream is idle here (the decode ends with a synchronisation), so growing is safe
  HIP_TRY(r.matrix.reserve(rows * cols));
  const size_t len = sys.len;
  HIP_TRY(r.rhs.reserve(rows * len));
  HIP_TRY(r.solution.reserve(cols * len));
  HIP_TRY(r.status.reserve(1));
  std::vector<uint16_t> h_m;
  std::vector<uint64_t> h_idx;
  if (src.weights) {  // the table's entries, gathered on the host
    h_m.resize(rows * cols);
    OMR_TRY(fill_matrix_host(src, seek, sys, all, indices, h_m.data()));
    HIP_TRY(hipMemcpyAsync(r.matrix, h_m.data(), h_m.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  } else {
    const WeightKey key = weight_key(src.weight_seed);
    h_idx.assign(indices, indices + cols);
    HIP_TRY(r.indices.reserve(cols));
    HIP_TRY(hipMemcpyAsync(r.indices, h_idx.data(), cols * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (src.by_seek)
      retrieve_matrix_seek_kernel<<<col_grid(rows * cols), SOLVE_COL_T, 0, st>>>(key, seek, all, r.indices, (uint32_t)rows,
                                                                                 (uint32_t)cols, r.matrix);
    else
      retrieve_matrix_kernel<<<col_grid(rows * cols), SOLVE_COL_T, 0, st>>>(key, r.indices, (uint32_t)rows, (uint32_t)cols,
                                                                            r.matrix);
  }
  if (ly)
    retrieve_rhs_len_kernel<<<col_grid(rows * len), SOLVE_COL_T, 0, st>>>(r.decoded, (uint32_t)rows, (uint32_t)sys.per,
                                                                          (uint32_t)len, (uint32_t)sys.stripes, r.rhs);
  else
    retrieve_rhs_kernel<<<col_grid(rows * PAYLOAD_LEN), SOLVE_COL_T, 0, st>>>(r.decoded, (uint32_t)rows, (uint32_t)sys.per,
                                                                              r.rhs);
  omr_status s = hipGetLastError() == hipSuccess ? OMR_OK : set_error(OMR_ERR_DEVICE, who + ": kernel launch failed");
  if (s == OMR_OK) s = launch_solve(aud, r.matrix, r.rhs, rows, cols, len, r.solution, r.status, st);
  uint32_t status = 0;
  std::vector<uint16_t> sol(cols * len);
  hipError_t e = hipSuccess;
  if (s == OMR_OK) e = hipMemcpyAsync(&status, r.status, sizeof status, hipMemcpyDeviceToHost, st);
  if (s == OMR_OK && e == hipSuccess)
    e = hipMemcpyAsync(sol.data(), r.solution, sol.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, st);
  // always drain the stream: the host vectors above must outlive the copies
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (s == OMR_OK && e != hipSuccess) s = hip_error((who + ": solve").c_str(), e);
  if (s != OMR_OK) return s;
  if (status) return set_error(OMR_ERR_NOT_INVERTIBLE, "Matrix is not invertible");
  std::copy(sol.begin(), sol.end(), payloads);
  return OMR_OK;
}

// The shared front of the entry points after their NULL test: bits, the auditor's lock, its device, then body().
template <typename Body>
omr_status with_auditor(omr_auditor *aud, int bits, const std::string &who, Body body) {
  if (bits && !compact_bits_ok(bits)) return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": bits must be 0 or in [16, 32]");
  std::lock_guard<std::mutex> lk(aud->mu);
  HIP_TRY(hipSetDevice(aud->device));
  return body();
}

// The three omr_auditor_retrieve_payloads* entries: they differ in where the matrix comes from.
omr_status auditor_payloads(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits, size_t all,
                            uint32_t combination_count, const MatrixSource &src, const size_t *indices, size_t n_indices,
                            uint16_t *payloads, const std::string &who, const omr_payload_layout *ly = nullptr) {
  if (!retrieve_args_ok(aud, pay_cts, src, indices, n_indices, payloads))
    return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": NULL argument");
  return with_auditor(aud, bits, who, [&] {
    return payloads_locked(aud, pay_cts, n_ct, bits, all, combination_count, src, indices, n_indices, payloads, nullptr, who,
                           ly);
  });
}

}  // namespace

extern "C" omr_status omr_auditor_retrieve_indices(omr_auditor *aud, const void *idx_cts, uint32_t n_ct, int bits,
                                                   size_t all_payloads_count, size_t pertinent_count, size_t *indices,
                                                   size_t cap, size_t *found) {
  const char *who = "omr_auditor_retrieve_indices";
  if (!aud || !found || (n_ct && !idx_cts) || (cap && !indices))
    return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  return with_auditor(aud, bits, who, [&] {
    omr_retrieval_params rp;
    OMR_TRY(omr_get_retrieval_params(all_payloads_count, pertinent_count, &rp));
    return indices_locked(aud, idx_cts, n_ct, bits, rp, pertinent_count, indices, cap, found, nullptr, who);
  });
}

extern "C" omr_status omr_auditor_retrieve_payloads(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits,
                                                    size_t all_payloads_count, uint32_t combination_count,
                                                    const uint16_t *weights, const size_t *indices, size_t n_indices,
                                                    uint16_t *payloads) {
  return auditor_payloads(aud, pay_cts, n_ct, bits, all_payloads_count, combination_count, MatrixSource{weights}, indices,
                          n_indices, payloads, "omr_auditor_retrieve_payloads");
}

extern "C" omr_status omr_auditor_retrieve_payloads_indexed(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits,
                                                            size_t all_payloads_count, uint32_t combination_count,
                                                            const uint8_t weight_seed[32], const size_t *indices,
                                                            size_t n_indices, uint16_t *payloads) {
  return auditor_payloads(aud, pay_cts, n_ct, bits, all_payloads_count, combination_count,
                          MatrixSource{nullptr, weight_seed}, indices, n_indices, payloads,
                          "omr_auditor_retrieve_payloads_indexed");
}

extern "C" omr_status omr_auditor_retrieve_payloads_indexed_len(omr_auditor *aud, const void *pay_cts, uint32_t n_ct,
                                                                int bits, size_t all_payloads_count,
                                                                const omr_payload_layout *layout,
                                                                const uint8_t weight_seed[32], const size_t *indices,
                                                                size_t n_indices, uint16_t *payloads) {
  const char *who = "omr_auditor_retrieve_payloads_indexed_len";
  if (!layout) return set_error(OMR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  return auditor_payloads(aud, pay_cts, n_ct, bits, all_payloads_count, layout->combination_count,
                          MatrixSource{nullptr, weight_seed}, indices, n_indices, payloads, who, layout);
}

extern "C" omr_status omr_auditor_retrieve_payloads_seek(omr_auditor *aud, const void *pay_cts, uint32_t n_ct, int bits,
                                                         size_t all_payloads_count, uint32_t combination_count,
                                                         const uint8_t weight_seed[32], const omr_weight_seek *seek,
                                                         const size_t *indices, size_t n_indices, uint16_t *payloads) {
  return auditor_payloads(aud, pay_cts, n_ct, bits, all_payloads_count, combination_count,
                          MatrixSource{nullptr, weight_seed, true, seek}, indices, n_indices, payloads,
                          "omr_auditor_retrieve_payloads_seek");
}

extern "C" omr_status omr_auditor_decode_digest_indexed(omr_auditor *aud, const void *idx_cts, uint32_t n_idx_ct,
                                                        const void *pay_cts, uint32_t n_pay_ct, int bits,
                                                        size_t all_payloads_count, size_t pertinent_count,
                                                        const uint8_t weight_seed[32], size_t *indices, size_t cap,
                                                        size_t *found, uint16_t *payloads, omr_audit_summary *summary) {
  const std::string who = "omr_auditor_decode_digest_indexed";
  if (!aud || !found || !pay_cts || !weight_seed || (n_idx_ct && !idx_cts) || (cap && (!indices || !payloads)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": NULL argument");
  return with_auditor(aud, bits, who, [&] {
    omr_retrieval_params rp;
    OMR_TRY(omr_get_retrieval_params(all_payloads_count, pertinent_count, &rp));
    omr_audit_summary sum{};  // merged into the caller's only when the whole call succeeds
    OMR_TRY(indices_locked(aud, idx_cts, n_idx_ct, bits, rp, pertinent_count, indices, cap, found,
                           summary ? &sum : nullptr, who.c_str()));
    if (cap < *found) return set_error(OMR_ERR_INVALID_ARGUMENT, who + ": more indices found than cap");
    OMR_TRY(payloads_locked(aud, pay_cts, n_pay_ct, bits, all_payloads_count, rp.combination_count,
                            MatrixSource{nullptr, weight_seed}, indices, *found, payloads, summary ? &sum : nullptr, who));
    if (summary) merge_summary(*summary, sum);
    return OMR_OK;
  });
}
