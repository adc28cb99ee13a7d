// The detector context, struct omr_ctx, shared by the host translation units of libomr_gpu (nothing
// outside csrc/ includes this), and the few functions those units lend each other. By owner:
//   context.hip   creation and destruction, key conversion and bounds, setters and getters, scratch sizes
//   detect.hip    every rotation, key-switch and trace launch, detect on device and host buffers, timing
//   two_cu_from.hip  br2y_from_kernel / br2x_from_kernel alone (no host code but their launch pointers)
//   coalesce.hip  omr_detect's queue
//   encode.hip    the encode kernels' launches and entry points
//   digest.hip    the digest session over detect and encode
//   compact.hip   compact ciphertexts: both kernels' launches (lent through compact.hpp), the context's entry points
// Beside them, without the context: weights.hip (the host weight functions over weights.hpp's statement, which
// the kernels share) and the recipient's retriever.hip and retrieve_device.hip over retrieve_system.hpp.
// One rule for kernels: a non-template __global__ function lives in a header that exactly one of these
// includes (or in the .hip itself); a second includer would define its host stub twice and the link
// fails. Headers that several units share (kernels.hpp, device_*.hpp, fft1024.hpp, exactness.hpp,
// key_spectra.hpp, host_tables.hpp) hold template kernels and __device__ functions only.
#pragma once

#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "hip_util.hpp"
#include "kernels.hpp"
#include "weights.hpp"

#ifndef OMR_DEFAULT_LATENCY_MAX
#define OMR_DEFAULT_LATENCY_MAX 64  // chunks up to this many messages run the latency kernels
#endif

// Every device allocation is a DevBuf member (freed with the context); the destructor releases the
// stream, the events and the pinned error word. omr_ctx_destroy synchronises before it deletes.
// Every member but `q` is read and written with `mu` held.
struct omr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;  // the context's own stream: host entry points and key conversion
  std::mutex mu;
  size_t batch = omr::OMR_DEFAULT_BATCH;            // messages per detect chunk (omr_ctx_set_batch)
  size_t enc_max_chunks = omr::OMR_ENC_MAX_CHUNKS;  // chunk partials per encode ciphertext (omr_ctx_set_encode_chunks)
  size_t latency_max = OMR_DEFAULT_LATENCY_MAX;     // chunks up to this many messages run the latency kernels

  // The keys in the kernels' forms: written by omr_ctx_create and never again, but for bsk1n.
  struct Keys {
    omr::DevBuf<double2> bsk1f;  // level-1 FFT-domain keys [512][8][2][512] complex, x 1/512
    omr::DevBuf<double2> bsk1l;  // the same in br1l_kernel's layout [512][8 slot][8 row][2][64 lane]
    // BSK1 in the NTT domain x 1/1024 [512][8][2][1024] (br1_ntt.hpp: level 1's exact path): 64 MB,
    // converted only when level 1 is first guarded or run exactly (ensure_bsk1n), from the
    // coefficient-domain copy kept on the host (32 MB) until then
    omr::DevBuf<double> bsk1n;
    std::vector<uint32_t> bsk1_host;
    omr::DevBuf<double> bsk2, tk;  // BSK2 NTT domain (latency kernels), trace key
    omr::DevBuf<double2> bsk2f;    // BSK2 as FFT-domain 25-bit limbs (br2f_kernel), x 1/1024
    omr::DevBuf<double2> tkf;      // the trace key the same way (trace_fft_kernel)
    omr::DevBuf<uint32_t> kskb;    // int8 limbs of the KSK, [1024][4][672][32] (matrix-core key switch)
  } keys;

  // Constant tables: uploaded by omr_ctx_create; tb holds pointers into them, passed to kernels by value.
  struct Tables {
    omr::DevBuf<double> tables;  // tw1 itw1 tw2 itw2 lut1 lut2 tw2c
    omr::DevBuf<uint16_t> trace_tabs;
    omr::DevBuf<double2> fft1, fft2;  // level-1 FFT twiddles, Fft1024 twiddles
    omr::DeviceTables tb{};
  } tab;

  // Scratch shared by every call on the context, while device-buffer calls only enqueue on the
  // caller's stream: the last stream that used it records `free` (ScratchLease), a call on another
  // stream waits for that event before its first kernel, and a buffer is reallocated only once that
  // event has passed (scratch_idle). The s_* staging is used on the context's own stream only.
  struct Scratch {
    omr::DevBuf<uint32_t> ext, lwe1t, lwe_int;  // per detect chunk, grown together (ensure_batch)
    omr::DevBuf<int> ks_part;                   // split key-switch partial sums, [KS_SPLIT][64][672][4]
    omr::DevBuf<uint64_t> partial;              // encode chunk partials (ensure_partial)
    omr::DevBuf<uint16_t> s_clue_a, s_clue_b;   // host-API staging, grown together (stage_buffers)
    omr::DevBuf<uint64_t> s_out;
    hipEvent_t free = nullptr;
    hipStream_t stream = nullptr;  // the stream that recorded `free`; NULL before the first lease
  } scr;

  // The cooperative multi-CU latency kernels (br2x_kernel / br2y_kernel, trace_x_kernel): hand-off
  // slots and flags per message (handoff.hpp; scratch like the above) and the timeout flag x_err,
  // which every cooperative launch copies to the pinned x_err_host on its stream
  // (take_handoff_error reads it). The switches are read once, at creation.
  struct Handoff {
    omr::DevBuf<double> x_slots, t_slots;  // BR2XY_SLOT_DOUBLES, TRACE_X_SLOT_DOUBLES per message
    omr::DevBuf<uint32_t> x_flags, t_flags;
    omr::DevBuf<int> x_err;
    int *x_err_host = nullptr;
    int num_cu = 0;
    bool coop = false;  // hipDeviceAttributeCooperativeLaunch and not OMR_COOPERATIVE=0
    // level 2 on the FFT (br2y_kernel with its key-prefetch helpers, 6.6 vs 7.6-7.9 ms for br2x at
    // one message) unless OMR_BR2Y=0; used when Exactness::apriori_y proves it exact and level 2 is
    // not guarded, br2x_kernel's NTT otherwise
    bool br2y = true;
    bool no_prefetch = false;      // OMR_PREFETCH=0: the latency kernels launch no key-prefetch helpers
    bool no_fast_handoff = false;  // OMR_FAST_HANDOFF=0: br2y keeps the sc1 hand-off on one XCD too
  } ho;

  // The exactness contract (exactness.hpp). kappa: largest stored key spectrum magnitude per level;
  // apriori: the bound it gives (apriori_bound); level l runs its guarded kernel variants when the
  // user set `guard` or apriori[l] >= 0.5 (guard_auto); thr = 1 - apriori, the certificate threshold
  // of one launch; margin: the GUARD_WORDS guard words. Set by create_bounds; guard and exact1 by
  // their setters, which build keys.bsk1n first.
  struct Exactness {
    bool guard = false, guard_auto[2] = {false, false};
    bool exact1 = false;  // omr_ctx_set_exact_level1: every level-1 launch on the exact NTT (br1n_kernel)
    omr::DevBuf<unsigned long long> margin;
    double kappa[2] = {0.0, 0.0}, apriori[2] = {0.0, 0.0}, thr[2] = {1.0, 1.0};
    // the throughput trace on the FFT (trace_fft_kernel) when its bound (apriori_bound level 4) is
    // below 0.5, else trace_kernel's NTT (never on a real key); apriori_y: br2y's bound (level 3)
    double apriori_t = 1.0, apriori_y = 1.0;
    bool trace_fft = false;
  } ex;

  // The launch record (omr_ctx_launch_record): cumulative launches per omr_launch_kind, counted on the
  // host where detect.hip chooses the kernel. No device state.
  uint64_t launches[OMR_LAUNCH_COUNT] = {};

  // Stage timing. mode 0: off; 1 or 2: detect_device records EV_PER_CHUNK events per chunk, and
  // messages / chunks describe the last timed call. omr_detect_batch stages the host input in pieces
  // of `batch` messages: their stage times are summed in `host` (valid while host_valid), so that
  // omr_last_timing covers the whole call; device-buffer calls clear host_valid and read the events.
  struct Timing {
    int mode = 0;
    std::vector<hipEvent_t> events;
    size_t messages = 0, chunks = 0;
    omr_detect_timing host{};
    bool host_valid = false;
  } tm;

  // Compact ciphertexts (compact.hip): omr_compact_cts's staging on the context's own stream, grown on
  // demand, and the two knobs. The kernel needs the inverse twiddles of `tab` and nothing else.
  struct Compact {
    omr::DevBuf<uint64_t> stage;   // one piece of ciphertexts
    omr::DevBuf<uint32_t> packed;  // its compact form
    unsigned grid = 0;             // workgroups; 0: six per compute unit (omr_ctx_set_compact_grid)
    size_t staging = 0;            // ciphertexts per piece; 0: 2,048 (omr_ctx_set_compact_staging)
  } cp;

  // omr_detect's coalescer (coalesce.hip): everything here is guarded by its own mutex `mu`, never
  // by the context's. A leader takes every queued request, runs them as one detect and wakes the callers.
  struct Coalescer {
    struct Req {
      const uint16_t *a, *b;
      uint64_t *out;
      omr_status st;
      std::string err;
      bool done;
    };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Req *> queue;
    bool leader = false;
    size_t max = 65536;  // messages per combined launch
    long window_us = 0;  // a leader waits this long for more requests before launching
    size_t calls = 0, launches = 0;
  } q;

  ~omr_ctx() {
    if (ho.x_err_host) (void)hipHostFree(ho.x_err_host);
    for (auto e : tm.events) (void)hipEventDestroy(e);
    if (scr.free) (void)hipEventDestroy(scr.free);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace omr {

inline bool guarded(const omr_ctx *c, int level) { return c->ex.guard || c->ex.guard_auto[level]; }

// All of the following are called with c->mu held and the context's device current.

// context.hip. The scratch groups grow together: a group is reallocated only when a member is too
// small, and only once every stream that used the scratch is done with it (scratch_idle).
omr_status scratch_idle(omr_ctx *c);
omr_status ensure_batch(omr_ctx *c, size_t B);        // ext, lwe1t, lwe_int for chunks of B messages
omr_status ensure_partial(omr_ctx *c, size_t elems);  // the encode workspace
omr_status stage_buffers(omr_ctx *c, size_t B);       // the host entry points' staging of B messages

// A lease of the shared scratch on stream st, taken before a call's first kernel on it: acquire makes
// st wait for the last stream that held one, release records Scratch::free behind the call's last
// kernel. Leaving the scope without release (a failed launch) records it too: what the call did
// enqueue still uses the scratch, and the next call on another stream has to wait for it.
struct ScratchLease {
  omr_ctx *c = nullptr;
  hipStream_t st = nullptr;
  ScratchLease() = default;
  ScratchLease(const ScratchLease &) = delete;
  ScratchLease &operator=(const ScratchLease &) = delete;
  ~ScratchLease() { (void)release(); }
  omr_status acquire(omr_ctx *ctx, hipStream_t s) {
    if (ctx->scr.stream && ctx->scr.stream != s) HIP_TRY(hipStreamWaitEvent(s, ctx->scr.free, 0));
    c = ctx;
    st = s;
    return OMR_OK;
  }
  omr_status release() {
    if (!c) return OMR_OK;
    omr_ctx *ctx = std::exchange(c, nullptr);
    HIP_TRY(hipEventRecord(ctx->scr.free, st));
    ctx->scr.stream = st;
    return OMR_OK;
  }
};

// detect.hip. detect_device: D messages of device buffers on st in chunks of the batch (the body of
// omr_detect_batch_device); it reports a pending hand-off error first. detect_host: omr_detect_batch's
// body. take_handoff_error reports (and clears) a hand-off timeout whose copy to the host has landed.
omr_status detect_device(omr_ctx *c, const uint16_t *d_clue_a, const uint16_t *d_clue_b, size_t D, uint64_t *d_out,
                         hipStream_t st);
omr_status detect_host(omr_ctx *c, const uint16_t *clue_a, const uint16_t *clue_b, size_t D, uint64_t *out);
omr_status take_handoff_error(omr_ctx *c);

// encode.hip. The bodies of omr_encode_indices_device / omr_encode_payloads*_device after their
// argument checks. accumulate = false: out = the sum of the chunk partials (the public entry points);
// accumulate = true: out = (out + that sum) mod q2, out canonical before and after (the digest
// session); D = 0 then leaves out alone.
omr_status encode_indices(omr_ctx *c, const uint64_t *d_pv, size_t D, size_t offset, size_t all, uint64_t seed,
                          uint32_t first_ct, uint32_t n_ct, uint64_t *d_out, hipStream_t st, bool accumulate);
// Where a payload encode takes its weights from, one kind per device entry point and digest session.
struct PayloadWeights {
  enum Kind { TABLE, INDEXED, SEEK, INDEXED_LEN } kind = TABLE;
  const uint16_t *d_table = nullptr;  // TABLE: [n_ct * per_ct][all] on the device, row 0 = first_ct's first
  WeightKey key{};                    // INDEXED[_LEN] (weights.hpp, indexed_weight_block), SEEK: the weight seed
  omr_weight_seek seek{};             // SEEK (weights.hpp, "Reference payload weights by seek"): of combos * all draws
  uint32_t combos = 0;                // INDEXED[_LEN], SEEK: combinations from this one on are padding, weight 0
  uint32_t len = PAYLOAD_LEN;         // words per payload: INDEXED_LEN's board parameter, 612 for every other kind
};
// The body of the omr_encode_payloads*_device entries: the ciphertexts [first_ct, first_ct + n_ct) of
// per_ct combinations each (INDEXED_LEN: per group of payload_stripes(len) ciphertexts); payloads
// [D][weights.len]; the kind picks the kernel (encode_kernels.hpp).
omr_status encode_payloads(omr_ctx *c, const uint64_t *d_pv, const uint16_t *d_payloads, size_t D, size_t offset,
                           size_t all, const PayloadWeights &weights, uint32_t first_ct, uint32_t n_ct,
                           uint32_t per_ct, uint64_t *d_out, hipStream_t st, bool accumulate);
// The body of omr_encode_bitmap_device after its argument checks (bitmap_kernel.hpp): d_out is the whole
// board's [omr_bitmap_ct_count(all)][2][N2]. accumulate = false: the touched ciphertexts are the sums of
// their partials and the others zero; accumulate = true: the touched ones are added into, the others
// and D = 0 leave d_out alone.
omr_status encode_bitmap(omr_ctx *c, const uint64_t *d_pv, size_t D, size_t offset, size_t all, uint64_t *d_out,
                         hipStream_t st, bool accumulate);
// digest = (digest + sum over `chunks` of partial [n_ct][chunks][2][N2]) mod q2 on st
// (accumulate_partials_kernel). Needs no context.
omr_status accumulate_partials(const uint64_t *d_partial, int chunks, uint32_t n_ct, uint64_t *d_digest,
                               hipStream_t st);

}  // namespace omr
