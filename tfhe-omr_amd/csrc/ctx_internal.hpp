// What context.hip lends to the other host translation units of libomr_gpu (digest.hip): the
// context's lock and the bodies of the detect / encode entry points that run under it. The kernels
// and omr_ctx itself stay in context.hip; nothing here is part of the C ABI.
#pragma once

#include <mutex>

#include "hip_util.hpp"

namespace omr {

// The context mutex (omr_ctx::mu): every *_locked function below is called with it held and the
// context's device current (ctx_device).
std::mutex &ctx_mutex(omr_ctx *c);
int ctx_device(const omr_ctx *c);
size_t ctx_batch(const omr_ctx *c);  // omr_ctx_set_batch

// omr_detect_batch_device's body: D messages of device buffers on st in chunks of the batch, with the
// context's scratch acquired and released in stream order. Reports a pending hand-off error first.
omr_status detect_device_locked(omr_ctx *c, const uint16_t *d_clue_a, const uint16_t *d_clue_b, size_t D,
                                uint64_t *d_out, hipStream_t st);
// Reports (and clears) a hand-off error whose copy has landed: take_handoff_error of context.hip.
omr_status take_handoff_error_locked(omr_ctx *c);

// The bodies of omr_encode_indices_device / omr_encode_payloads_device after their argument checks.
// accumulate = false: out = the sum of the chunk partials (the public entry points);
// accumulate = true: out = (out + that sum) mod q2, out canonical before and after (the digest
// session); D = 0 then leaves out alone.
omr_status encode_indices_locked(omr_ctx *c, const uint64_t *d_pv, size_t D, size_t offset, size_t all,
                                 uint64_t seed, uint32_t first_ct, uint32_t n_ct, uint64_t *d_out,
                                 hipStream_t st, bool accumulate);
omr_status encode_payloads_locked(omr_ctx *c, const uint64_t *d_pv, const uint16_t *d_payloads, size_t D,
                                  size_t offset, size_t all, const uint16_t *d_weights, uint32_t n_ct,
                                  uint32_t per_ct, uint64_t *d_out, hipStream_t st, bool accumulate);

// digest = (digest + sum over `chunks` of partial [n_ct][chunks][2][N2]) mod q2 on st
// (accumulate_partials_kernel, encode_kernels.hpp). Needs no context.
omr_status accumulate_partials(const uint64_t *d_partial, int chunks, uint32_t n_ct, uint64_t *d_digest,
                               hipStream_t st);

}  // namespace omr
