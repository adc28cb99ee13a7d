// Detector context: device-resident keys and tables, batch orchestration and the C ABI of
// include/omr_gpu.h for the detect / encode path.
//
// Detector::new (detector.rs:85-110) -> omr_ctx_create: uploads the coefficient-domain keys,
// converts them on the GPU (BSK1 to the FFT domain x 1/512, BSK2 and the trace key to centred
// FP64 NTT-domain rows with N^-1 folded into the external-product keys, the KSK to int8 limbs)
// and builds the LUTs (:457-503). Detector::detect (:135-166) for a batch of messages -> four
// launches per chunk: br1f_kernel (7 blind rotations per message), sum7_kernel, ks_mfma_kernel,
// br2f_kernel (level-2 rotation on the exact FFT + the trace).
//
// Top to bottom: the context (omr_ctx owns every device allocation through DevBuf, hip_util.hpp),
// the launch helpers, context creation (tables from host_tables.hpp, keys, bounds and guards) and
// the C ABI. The digest session (digest.hip) runs the detect and encode bodies through
// ctx_internal.hpp.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "br1_latency.hpp"
#include "br1_ntt.hpp"
#include "br2_fft.hpp"
#include "br2_ntt.hpp"
#include "ctx_internal.hpp"
#include "encode_kernels.hpp"
#include "hip_util.hpp"
#include "host_tables.hpp"
#include "key_spectra.hpp"
#include "ks_mfma.hpp"

using namespace omr;
#ifndef OMR_DEFAULT_LATENCY_MAX
#define OMR_DEFAULT_LATENCY_MAX 64  // chunks up to this many messages run the latency kernels
#endif

// Every device allocation is a DevBuf member (freed with the context); the destructor releases the
// stream, the events and the pinned error word. omr_ctx_destroy synchronises before it deletes.
struct omr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf<double2> bsk1f;  // level-1 FFT-domain keys [512][8][2][512] complex, x 1/512
  DevBuf<double2> bsk1l;  // the same in br1l_kernel's layout [512][8 slot][8 row][2][64 lane]
  DevBuf<double> bsk1n;   // BSK1 in the NTT domain x 1/1024 [512][8][2][1024] (br1_ntt.hpp: level 1's exact path)
  // the coefficient-domain BSK1 kept on the host (32 MB) until bsk1n is built: bsk1n (64 MB of HBM)
  // is converted lazily, only when level 1 is guarded or run exactly (ensure_bsk1n)
  std::vector<uint32_t> bsk1_host;
  DevBuf<double2> fft1;     // level-1 FFT twiddles
  DevBuf<double> bsk2, tk;  // BSK2 NTT domain (latency kernels), trace key
  DevBuf<double2> bsk2f;    // BSK2 as FFT-domain 25-bit limbs (br2f_kernel), x 1/1024
  DevBuf<double2> tkf;      // the trace key the same way (br2f_kernel's fused trace)
  DevBuf<double2> fft2;     // Fft1024 twiddles
  DevBuf<uint32_t> kskb;    // int8 limbs of the KSK, [1024][4][672][32] (matrix-core key switch)
  DevBuf<double> tables;    // tw1 itw1 tw2 itw2 lut1 lut2 tw2c
  DevBuf<uint16_t> trace_tabs;
  DeviceTables tb{};
  size_t batch = OMR_DEFAULT_BATCH;
  size_t enc_max_chunks = OMR_ENC_MAX_CHUNKS;  // chunk partials per encode ciphertext (omr_ctx_set_encode_chunks)
  DevBuf<uint32_t> ext, lwe1t, lwe_int;  // per-chunk scratch, grown together (ensure_batch)
  // chunks of at most latency_max messages run the latency kernels (br1_latency.hpp)
  size_t latency_max = OMR_DEFAULT_LATENCY_MAX;
  DevBuf<int> ks_part;  // split key-switch partial sums, [KS_SPLIT][64][672][4]
  // two-CU level-2 latency kernels (br2x_kernel, br2y_kernel; cooperative launch): hand-off slots
  // and flags (handoff.hpp: BR2XY_SLOT_DOUBLES, BR2XY_FLAGS per message), a timeout flag x_err that
  // every launch copies to the pinned host word x_err_host on its stream (read by omr_ctx_check
  // and at the start of the next call)
  DevBuf<double> x_slots;
  DevBuf<uint32_t> x_flags;
  DevBuf<int> x_err;
  int *x_err_host = nullptr;
  // multi-CU trace of the latency path (trace_x_kernel): TRACE_X_SLOT_DOUBLES, TRACE_X_FLAGS per message
  DevBuf<double> t_slots;
  DevBuf<uint32_t> t_flags;
  int num_cu = 0;
  bool coop = false;  // hipDeviceAttributeCooperativeLaunch
  // rounding-margin guard (exactness.hpp): guarded kernel variants for level l when the user set
  // the guard or the key's a priori bound E_l >= 0.5 (guard_auto, the exactness contract); margin:
  // the GUARD_WORDS guard words (bits of the largest |y - rint(y)|, per launch and cumulative, and
  // the breach counts); kappa: largest stored key spectrum magnitude per level; apriori: the bound it
  // gives (apriori_bound); thr = 1 - apriori, the certificate threshold of one launch
  bool guard = false, guard_auto[2] = {false, false};
  // omr_ctx_set_exact_level1: every level-1 launch on the exact modular NTT (br1n_kernel)
  bool exact1 = false;
  DevBuf<unsigned long long> margin;
  double kappa[2] = {0.0, 0.0}, apriori[2] = {0.0, 0.0}, thr[2] = {1.0, 1.0};
  // the fused trace on the FFT (br2f_trace) when its a priori bound (apriori_bound level 4) is below
  // 0.5; otherwise br2f_kernel stops at the rotation and trace_kernel's NTT runs (never on a real key)
  double apriori_t = 1.0;
  bool trace_fft = false;
  // the latency path's level 2 on the FFT (br2y_kernel with its key-prefetch helpers; the default
  // since round 5, 6.6 vs 7.6-7.9 ms for br2x at one message; OMR_BR2Y=0 at context creation: br2x)
  // when its accumulation order's bound (apriori_bound level 3) proves it exact and the level is
  // not guarded; br2x_kernel's NTT otherwise
  double apriori_y = 1.0;
  bool br2y = true;
  bool no_prefetch = false;  // OMR_PREFETCH=0: the latency kernels launch no key-prefetch helpers
  bool no_fast_handoff = false;  // OMR_FAST_HANDOFF=0: br2y keeps the sc1 hand-off on one XCD too
  // host-API staging, grown together (stage_buffers)
  DevBuf<uint16_t> s_clue_a, s_clue_b;
  DevBuf<uint64_t> s_out;
  // encode workspace
  DevBuf<uint64_t> partial;
  // The scratch above is shared by every call on the context, while device-buffer calls only
  // enqueue on the caller's stream: the last stream that used it records scratch_free, and a call
  // on another stream waits for that event before its first kernel.
  hipEvent_t scratch_free = nullptr;
  hipStream_t scratch_stream = nullptr;
  // omr_detect_batch stages the host input in pieces of `batch` messages: their stage times are
  // summed here so omr_last_timing covers the whole call (device-buffer calls read the events)
  omr_detect_timing host_timing{};
  bool host_timing_valid = false;
  // timing: mode 0 off, 1 stage events around the production kernels, 2 trace as its own launch
  int timing = 0;
  std::vector<hipEvent_t> events;  // EV_PER_CHUNK per chunk
  size_t timed_messages = 0, timed_chunks = 0;
  bool timed_split = false;  // the timed call ran the trace as its own launch in every chunk
  std::mutex mu;
  // omr_detect: concurrent single-message calls are combined into batched launches (a leader
  // takes every queued request, runs them as one detect, and wakes their callers)
  struct DetectReq {
    const uint16_t *a, *b;
    uint64_t *out;
    omr_status st;
    std::string err;
    bool done;
  };
  std::mutex qmu;
  std::condition_variable qcv;
  std::vector<DetectReq *> queue;
  bool leader = false;
  size_t coalesce_max = 65536;   // messages per combined launch
  long coalesce_window_us = 0;   // a leader waits this long for more requests before launching
  size_t coalesced_calls = 0, coalesced_launches = 0;

  ~omr_ctx() {
    if (x_err_host) (void)hipHostFree(x_err_host);
    for (auto e : events) (void)hipEventDestroy(e);
    if (scratch_free) (void)hipEventDestroy(scratch_free);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

#define OMR_BR1_NAME "br1f_kernel"
#define OMR_KS_NAME "ks_mfma_kernel"
#define OMR_BR2_NAME "br2f_kernel"

namespace {

bool guarded(const omr_ctx *c, int level) { return c->guard || c->guard_auto[level]; }

// Scratch reuse across streams (see omr_ctx::scratch_free). Callers hold c->mu.
omr_status scratch_acquire(omr_ctx *c, hipStream_t st) {
  if (c->scratch_stream && c->scratch_stream != st) HIP_TRY(hipStreamWaitEvent(st, c->scratch_free, 0));
  return OMR_OK;
}
omr_status scratch_release(omr_ctx *c, hipStream_t st) {
  HIP_TRY(hipEventRecord(c->scratch_free, st));
  c->scratch_stream = st;
  return OMR_OK;
}
// Reallocating scratch: every stream that used it must be done first.
omr_status scratch_idle(omr_ctx *c) {
  if (c->scratch_stream) HIP_TRY(hipEventSynchronize(c->scratch_free));
  return OMR_OK;
}

// The scratch groups grow together: a group is reallocated only when a member is too small, and
// scratch shared across streams only once every stream that used it is done (scratch_idle).
omr_status ensure_batch(omr_ctx *c, size_t B) {
  const size_t ne = B * CLUES * (N1 + 1), nt = B * (N1 + 1), ni = B * (NI + 1);
  if (c->ext.fits(ne) && c->lwe1t.fits(nt) && c->lwe_int.fits(ni)) return OMR_OK;
  omr_status s;
  if ((s = scratch_idle(c)) != OMR_OK) return s;
  HIP_TRY(c->ext.reserve(ne));
  HIP_TRY(c->lwe1t.reserve(nt));
  HIP_TRY(c->lwe_int.reserve(ni));
  return OMR_OK;
}

omr_status ensure_partial(omr_ctx *c, size_t elems) {
  if (c->partial.fits(elems)) return OMR_OK;
  omr_status s;
  if ((s = scratch_idle(c)) != OMR_OK) return s;
  HIP_TRY(c->partial.reserve(elems));
  return OMR_OK;
}

// The host entry points' staging of B messages (used on the context's own stream only).
omr_status stage_buffers(omr_ctx *c, size_t B) {
  HIP_TRY(c->s_clue_a.reserve(B * N0));
  HIP_TRY(c->s_clue_b.reserve(B * CLUES));
  HIP_TRY(c->s_out.reserve(B * 2 * N2));
  return OMR_OK;
}

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

// ---- BSK2 rows -> the CmuxNtt forward order, x scale (the blind rotation's key layout) ----
__global__ __launch_bounds__(256) static void key_to_cmux_kernel(const uint64_t *in, double *out, size_t npoly,
                                                        double scale, const double *tw2c) {
  using M = Mod<2>;
  using NTT = CmuxNtt;
  __shared__ double lds[NTT::LDS_DOUBLES];
  __shared__ double tws[NTT::N];
  const size_t poly = blockIdx.x;
  const int tid = threadIdx.x;
  if (poly >= npoly) return;
  const uint64_t *src = in + poly * NTT::N;
  double x[NTT::E];
#pragma unroll
  for (int e = 0; e < NTT::E; ++e) {
    x[e] = from_u64<M>(src[tid + e * NTT::T]);
    tws[tid + e * NTT::T] = tw2c[tid + e * NTT::T];
  }
  __syncthreads();
  NTT::fwd<0>(x, lds, tws, tid);
  double *dst = out + poly * NTT::N + tid * NTT::E;
#pragma unroll
  for (int e = 0; e < NTT::E; ++e) dst[e] = canon<M>(mm<M>(canon<M>(x[e]), scale));
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

bool latency_path(const omr_ctx *c, size_t n) { return n <= c->latency_max; }

// The two-CU kernel's bounded hand-off wait: a workgroup whose partner never published leaves its
// loop and sets x_err; each launch then copies x_err to the pinned x_err_host on its stream. This
// reports (and clears) an error whose copy has landed: callers sync the stream first for a
// definitive answer (omr_ctx_check, the host entry points), or call it before enqueueing new work
// (the device entry points) so a failed earlier call is never attributed to a later one.
omr_status take_handoff_error(omr_ctx *c) {
  if (!c->x_err_host || !__atomic_load_n(c->x_err_host, __ATOMIC_ACQUIRE)) return OMR_OK;
  HIP_TRY(hipDeviceSynchronize());  // no launch may still be copying the flag
  (void)__atomic_exchange_n(c->x_err_host, 0, __ATOMIC_ACQ_REL);
  HIP_TRY(hipMemset(c->x_err, 0, sizeof(int)));
  return set_error(OMR_ERR_DEVICE,
                   "level-2 two-CU hand-off timed out: the output of an earlier detect call on this "
                   "context is invalid");
}

// Zero the per-launch guard word of `level` before a guarded launch.
omr_status guard_begin(omr_ctx *c, int level, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(c->margin + 2 + level, 0, sizeof(unsigned long long), st));
  return OMR_OK;
}
// After a guarded launch and its conditional exact re-run: fold the launch's margin into the
// cumulative word and count a breach.
omr_status guard_end(omr_ctx *c, int level, hipStream_t st) {
  guard_fold_kernel<<<1, 64, 0, st>>>(c->margin, level, c->thr[level]);
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// Level 1's exact-NTT key (br1n_kernel / br1n_fallback_kernel), built on first need: when level 1
// is guarded (the exactness contract's re-run target) or run exactly. Callers hold c->mu (or own c).
omr_status ensure_bsk1n(omr_ctx *c) {
  if (c->bsk1n) return OMR_OK;
  if (c->bsk1_host.size() != BSK1_ELEMS)
    return set_error(OMR_ERR_DEVICE, "ensure_bsk1n: the coefficient-domain BSK1 is gone");
  DevBuf<double> key;
  HIP_TRY(key.alloc(BSK1_ELEMS));
  omr_status s;
  if ((s = convert_keys<1, uint32_t, double>(c->bsk1_host.data(), BSK1_ELEMS / N1, key, ninv_centred(N1, Q1),
                                             c->tb.tw1, c->stream)) != OMR_OK)
    return s;
  c->bsk1n = std::move(key);
  std::vector<uint32_t>().swap(c->bsk1_host);
  return OMR_OK;
}

// LWE key switch + modulus switch of B messages (lwe1t [1025][B] -> out [B][671]). Up to 64
// messages (the latency path) the input coefficients are split over KS_SPLIT workgroup slices.
omr_status launch_ks(omr_ctx *c, int B, uint32_t *out, hipStream_t st) {
  if (latency_path(c, (size_t)B) && B <= 64) {
    ks_mfma_split_kernel<<<dim3(1, KSM_COLS / 32, KS_SPLIT), 64, 0, st>>>(c->lwe1t, c->kskb, c->ks_part, B, 64);
    HIP_TRY(hipGetLastError());
    ks_combine_kernel<<<(B * (NI + 1) + 255) / 256, 256, 0, st>>>(c->ks_part, c->lwe1t, out, B, 64);
  } else {
    ks_mfma_kernel<<<dim3((B + 63) / 64, KSM_COLS / 32), 64, 0, st>>>(c->lwe1t, c->kskb, out, B);
  }
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// Level-1 blind rotations of n (message, clue) pairs (mode 0: clue g % 7 of message g / 7 ->
// extracted LWE; mode 1: explicit LWEs -> full RLWE), BR1F_WPG rotations per workgroup.
// `msgs`: the messages of the chunk (selects the latency kernels, one workgroup per rotation).
omr_status launch_br1(omr_ctx *c, size_t n, const uint16_t *ca, const uint16_t *cb,
                      const uint16_t *la, const uint16_t *lb, uint32_t *ext, uint64_t *rlwe, int mode,
                      hipStream_t st, size_t msgs) {
  if (c->exact1) {  // the reference's arithmetic for every rotation (omr_ctx_set_exact_level1)
    br1n_kernel<<<(unsigned)n, 64, 0, st>>>(ca, cb, la, lb, c->bsk1n, c->tb, ext, rlwe, mode, n);
    HIP_TRY(hipGetLastError());
    return OMR_OK;
  }
  const unsigned g1 = (unsigned)((n + BR1F_WPG - 1) / BR1F_WPG);
  const bool g = guarded(c, 0);
  omr_status s;
  if (g && (s = guard_begin(c, 0, st)) != OMR_OK) return s;
  if (latency_path(c, msgs)) {
    if (g)
      br1l_guard_kernel<<<(unsigned)n, 64 * BR1L_WAVES, 0, st>>>(ca, cb, la, lb, c->bsk1l, c->tb, ext, rlwe, mode,
                                                                  c->margin + 2);
    else
      br1l_kernel<<<(unsigned)n, 64 * BR1L_WAVES, 0, st>>>(ca, cb, la, lb, c->bsk1l, c->tb, ext, rlwe, mode);
  } else if (g) {
    br1f_guard_kernel<<<g1, 64 * BR1F_WPG, 0, st>>>(ca, cb, la, lb, c->bsk1f, c->tb, ext, rlwe, mode, n,
                                                    c->margin + 2);
  } else {
    br1f_kernel<<<g1, 64 * BR1F_WPG, 0, st>>>(ca, cb, la, lb, c->bsk1f, c->tb, ext, rlwe, mode, n);
  }
  HIP_TRY(hipGetLastError());
  if (!g) return OMR_OK;
  // the exactness contract: a guarded launch whose margin reached 1 - E1 is recomputed on the exact
  // NTT in the same stream order (every workgroup leaves at once otherwise)
  br1n_fallback_kernel<<<(unsigned)n, 64, 0, st>>>(ca, cb, la, lb, c->bsk1n, c->tb, ext, rlwe, mode, n,
                                                   c->margin + 2, c->thr[0]);
  HIP_TRY(hipGetLastError());
  return guard_end(c, 0, st);
}

// A cooperative launch (co-residency guaranteed, or the launch is refused): *launched stays false
// when the runtime refuses it (nothing was enqueued; the caller falls back to a plain kernel). A
// launch is followed by the copy of the context's error word to its pinned host copy.
omr_status coop_launch(omr_ctx *c, const char *name, const void *kernel, dim3 grid, dim3 block, void **args,
                       hipStream_t st, bool *launched) {
  const hipError_t e = hipLaunchCooperativeKernel(kernel, grid, block, args, 0, st);
  if (e == hipErrorCooperativeLaunchTooLarge || e == hipErrorNotSupported || e == hipErrorInvalidConfiguration) {
    (void)hipGetLastError();  // refused: nothing was enqueued
    return OMR_OK;
  }
  if (e != hipSuccess)
    return set_error(OMR_ERR_DEVICE, std::string(name) + " cooperative launch: " + hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(c->x_err_host, c->x_err, sizeof(int), hipMemcpyDeviceToHost, st));
  *launched = true;
  return OMR_OK;
}

// The hand-off slots and flags of a cooperative latency kernel for n messages (shared scratch),
// the flags zeroed on st.
omr_status handoff_scratch(omr_ctx *c, DevBuf<double> &slots, size_t nslots, DevBuf<uint32_t> &flags, size_t nflags,
                           hipStream_t st) {
  if (!slots.fits(nslots) || !flags.fits(nflags)) {
    omr_status s;
    if ((s = scratch_idle(c)) != OMR_OK) return s;
    HIP_TRY(slots.reserve(nslots));
    HIP_TRY(flags.reserve(nflags));
  }
  HIP_TRY(hipMemsetAsync(flags, 0, nflags * sizeof(uint32_t), st));
  return OMR_OK;
}

// br2x_kernel over 2 n workgroups as a cooperative launch; false when refused, so the caller falls
// back to br2l_kernel.
omr_status launch_br2x(omr_ctx *c, size_t n, const uint32_t *lwe_int, uint64_t *out, hipStream_t st,
                       bool *launched) {
  *launched = false;
  if (!c->coop || 2 * n > (size_t)c->num_cu) return OMR_OK;  // one 150 KB-LDS workgroup per CU
  omr_status s;
  // sized for whichever of br2x / br2y runs (handoff.hpp)
  if ((s = handoff_scratch(c, c->x_slots, n * BR2XY_SLOT_DOUBLES, c->x_flags, n * BR2XY_FLAGS, st)) != OMR_OK) return s;
  const double *bsk2 = c->bsk2;
  DeviceTables tb = c->tb;
  double *slots = c->x_slots;
  uint32_t *flags = c->x_flags;
  int *err = c->x_err;
  void *args[] = {(void *)&lwe_int, (void *)&bsk2, (void *)&tb, (void *)&slots, (void *)&flags, (void *)&err,
                  (void *)&out};
  // br2y_kernel (FFT) when the bound of its accumulation order proves it exact and level 2 is not
  // guarded; br2x_kernel's exact NTT otherwise (same arguments apart from the key form)
  const bool y = c->br2y && !guarded(c, 1) && c->apriori_y < 0.5;
  const double2 *bskf = c->bsk2f, *twg = c->fft2;
  // br2y: message m in column m of a grid w8 = n rounded up to 8 columns wide, its mask / body
  // workers in rows 0 / 1, plus 2 BR2Y_H rows of key prefetchers (br2_fft.hpp) when every workgroup
  // still gets a CU of its own
  const int nmsg = (int)n, w8 = (nmsg + 7) / 8 * 8, allow_fast = c->no_fast_handoff ? 0 : 1;
  const int rows = (size_t)w8 * (2 + 2 * BR2Y_H) <= (size_t)c->num_cu && !c->no_prefetch ? 2 + 2 * BR2Y_H : 2;
  if (y && (size_t)w8 * rows > (size_t)c->num_cu) return OMR_OK;  // one workgroup per CU: br2l instead
  void *args_y[] = {(void *)&lwe_int, (void *)&bskf, (void *)&twg, (void *)&tb, (void *)&slots, (void *)&flags,
                    (void *)&err, (void *)&out, (void *)&nmsg, (void *)&w8, (void *)&allow_fast};
  const void *kern = y ? reinterpret_cast<const void *>(&br2y_kernel) : reinterpret_cast<const void *>(&br2x_kernel);
  return coop_launch(c, "br2x", kern, dim3(y ? (unsigned)(w8 * rows) : (unsigned)(2 * n)), dim3(y ? BR2Y_T : BR2L_T),
                     y ? args_y : args, st, launched);
}

// The latency path's trace over TRACE_X CUs per message (trace_x_kernel) as a cooperative launch;
// false when refused (the caller then runs trace_kernel, one workgroup per message).
omr_status launch_trace_x(omr_ctx *c, size_t n, uint64_t *io, hipStream_t st, bool *launched) {
  *launched = false;
  if (!c->coop || TRACE_X * n > 2 * (size_t)c->num_cu) return OMR_OK;
  omr_status s;
  if ((s = handoff_scratch(c, c->t_slots, n * TRACE_X_SLOT_DOUBLES, c->t_flags, n * TRACE_X_FLAGS, st)) != OMR_OK) return s;
  const double *tk = c->tk;
  DeviceTables tb = c->tb;
  double *slots = c->t_slots;
  uint32_t *flags = c->t_flags;
  int *err = c->x_err;
  void *args[] = {(void *)&io, (void *)&tk, (void *)&tb, (void *)&slots, (void *)&flags, (void *)&err};
  return coop_launch(c, "trace_x", reinterpret_cast<const void *>(&trace_x_kernel), dim3((unsigned)(TRACE_X * n)),
                     dim3(BR2_T), args, st, launched);
}

// Level-2 blind rotation (+ trace, mode 0) of n LWE(670, 4096) ciphertexts. `mid` (optional) is
// recorded between the rotation and the trace; with split_trace (timing mode 2) the throughput
// path runs them as two launches so that the event separates them.
omr_status launch_br2(omr_ctx *c, size_t n, const uint32_t *lwe_int, uint64_t *out, int mode,
                      hipStream_t st, bool split_trace = false, hipEvent_t mid = nullptr) {
  if (latency_path(c, n)) {  // two CUs (or two 4-wave groups) per message, then the trace in place
    bool two_cu = false;
    omr_status s;
    if ((s = launch_br2x(c, n, lwe_int, out, st, &two_cu)) != OMR_OK) return s;
    if (!two_cu) br2l_kernel<<<(unsigned)n, BR2L_T, 0, st>>>(lwe_int, c->bsk2, c->tb, out);
    split_trace = true;
  } else {
    // br2f_kernel (the rotation, coefficient domain), then the trace as its own launch: on the FFT
    // (trace_fft_kernel) when its a priori bound allows, else the NTT (trace_kernel). The exactness
    // contract: a guarded pair notes both kernels' rounding margins in level 2's word, and a launch
    // pair whose margin reaches the threshold is re-run on the exact NTT (br2l_fallback_kernel and
    // trace_fallback_kernel: every workgroup leaves at once otherwise).
    const bool g = guarded(c, 1);
    omr_status s;
    if (g && (s = guard_begin(c, 1, st)) != OMR_OK) return s;
    if (g)
      br2f_guard_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(lwe_int, c->bsk2f, c->fft2, c->tb, out, c->margin + 3);
    else
      br2f_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(lwe_int, c->bsk2f, c->fft2, c->tb, out);
    HIP_TRY(hipGetLastError());
    if (mid) HIP_TRY(hipEventRecord(mid, st));
    if (mode == 0) {
      if (!c->trace_fft)
        trace_kernel<<<(unsigned)n, BR2_T, 0, st>>>(out, c->tk, c->tb);
      else if (g)
        trace_fft_guard_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(out, c->tkf, c->fft2, c->tb, c->margin + 3);
      else
        trace_fft_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(out, c->tkf, c->fft2, c->tb);
      HIP_TRY(hipGetLastError());
    }
    if (g) {
      br2l_fallback_kernel<<<(unsigned)n, BR2L_T, 0, st>>>(lwe_int, c->bsk2, c->tb, out, c->margin + 3, c->thr[1]);
      HIP_TRY(hipGetLastError());
      if (mode == 0)
        trace_fallback_kernel<<<(unsigned)n, BR2_T, 0, st>>>(out, c->tk, c->tb, c->margin + 3, c->thr[1]);
      HIP_TRY(hipGetLastError());
      if ((s = guard_end(c, 1, st)) != OMR_OK) return s;
    }
    return OMR_OK;
  }
  HIP_TRY(hipGetLastError());
  if (mid) HIP_TRY(hipEventRecord(mid, st));
  if (split_trace && mode == 0) {
    bool multi = false;
#ifndef OMR_NO_TRACE_X
    if (latency_path(c, n)) {
      omr_status s;
      if ((s = launch_trace_x(c, n, out, st, &multi)) != OMR_OK) return s;
    }
#endif
    if (!multi) trace_kernel<<<(unsigned)n, BR2_T, 0, st>>>(out, c->tk, c->tb);
    HIP_TRY(hipGetLastError());
  }
  return OMR_OK;
}

// The first level of B messages: br1 (7 rotations per message) -> sum7 -> key switch into
// c->lwe_int. With ev (detect_device's stage events) ev[1] is recorded after br1, ev[2] after the
// key switch.
omr_status launch_first_level(omr_ctx *c, int B, const uint16_t *ca, const uint16_t *cb, hipStream_t st,
                              hipEvent_t *ev = nullptr) {
  omr_status s;
  if ((s = launch_br1(c, (size_t)B * CLUES, ca, cb, nullptr, nullptr, c->ext, nullptr, 0, st, (size_t)B)) != OMR_OK)
    return s;
  if (ev) HIP_TRY(hipEventRecord(ev[1], st));
  const size_t n7 = (size_t)B * (N1 + 1);
  sum7_kernel<<<(unsigned)((n7 + 255) / 256), 256, 0, st>>>(c->ext, c->lwe1t, B);
  if ((s = launch_ks(c, B, c->lwe_int, st)) != OMR_OK) return s;
  if (ev) HIP_TRY(hipEventRecord(ev[2], st));
  return OMR_OK;
}

}  // namespace

// Scale the even (alpha) rows of the trace key by N^-1 in place.
__global__ void scale_even_rows_kernel(double *rows, size_t npoly, double s) {
  using M = Mod<2>;
  const size_t poly = (size_t)blockIdx.x * 2;
  if (poly >= npoly) return;
  double *p = rows + poly * N2;
  for (int j = threadIdx.x; j < N2; j += blockDim.x) p[j] = canon<M>(mm<M>(p[j], s));
}

// ------------------------------------------------------------------------------------------
// Context creation: tables, keys, bounds and guards (all on the context's stream)
// ------------------------------------------------------------------------------------------
namespace {

omr_status create_tables(omr_ctx *c) {
  std::vector<double> tw1, itw1, tw2, itw2;
  twiddles(Q1, N1, 7, tw1, itw1);
  twiddles(Q2, N2, 22, tw2, itw2);
  auto lut1 = first_level_lut(), lut2 = second_level_lut(), tw2c = cmux_twiddles(tw2);
  std::vector<double> tabs;
  for (auto *v : {&tw1, &itw1, &tw2, &itw2, &lut1, &lut2, &tw2c}) tabs.insert(tabs.end(), v->begin(), v->end());
  HIP_TRY(c->tables.upload_sync(tabs));
  HIP_TRY(c->trace_tabs.upload_sync(trace_tables()));
  HIP_TRY(c->fft1.upload_sync(fft_twiddles()));
  HIP_TRY(c->fft2.upload_sync(fft2_twiddles()));
  c->tb.tw1 = c->tables;
  c->tb.itw1 = c->tables + N1;
  c->tb.tw2 = c->tables + 2 * N1;
  c->tb.itw2 = c->tables + 2 * N1 + N2;
  c->tb.lut1 = c->tables + 2 * N1 + 2 * N2;
  c->tb.lut2 = c->tables + 3 * N1 + 2 * N2;
  c->tb.tw2c = c->tables + 3 * N1 + 3 * N2;
  c->tb.trace_src = c->trace_tabs;
  c->tb.trace_perm = c->trace_tabs + TRACE_STEPS * N2;
  c->tb.fft1 = c->fft1;
  return OMR_OK;
}

// The coefficient-domain keys of the view (host or device memory) -> the kernels' forms.
omr_status create_keys(omr_ctx *c, const omr_detection_key_view *key) {
  HIP_TRY(c->bsk1f.alloc(BSK1_ELEMS / 2));
  HIP_TRY(c->bsk1l.alloc(BSK1_ELEMS / 2));
  HIP_TRY(c->bsk2.alloc(BSK2_ELEMS));
  HIP_TRY(c->bsk2f.alloc(BSK2_ELEMS));
  HIP_TRY(c->tk.alloc(TK_ELEMS));
  HIP_TRY(c->tkf.alloc(TK_ELEMS));
  HIP_TRY(c->kskb.alloc(KSKB_WORDS));
  const double ninv2 = ninv_centred(N2, Q2);
  hipStream_t st = c->stream;
  omr_status s;
  if ((s = convert_keys_dd<1>(key->bsk1, BSK1_ELEMS / N1, c->bsk1f, st)) != OMR_OK) return s;
  bsk1_latency_layout_kernel<<<(unsigned)(BSK1_ELEMS / 2 / 256), 256, 0, st>>>(c->bsk1f, c->bsk1l, BSK1_ELEMS / 2);
  HIP_TRY(hipGetLastError());
  c->bsk1_host.resize(BSK1_ELEMS);  // for ensure_bsk1n (the view may point to host or device memory)
  HIP_TRY(hipMemcpy(c->bsk1_host.data(), key->bsk1, BSK1_ELEMS * sizeof(uint32_t), hipMemcpyDefault));
  if ((s = convert_keys_cmux(key->bsk2, BSK2_ELEMS / N2, c->bsk2, ninv2, c->tb.tw2c, st)) != OMR_OK) return s;
  if ((s = convert_keys_dd<2>(key->bsk2, BSK2_ELEMS / N2, c->bsk2f, st)) != OMR_OK) return s;
  if ((s = convert_keys_dd<2>(key->trace_key, TK_ELEMS / N2, c->tkf, st)) != OMR_OK) return s;
  if ((s = convert_keys<2, uint64_t, double>(key->trace_key, TK_ELEMS / N2, c->tk, 1.0, c->tb.tw2, st)) != OMR_OK)
    return s;
  scale_even_rows_kernel<<<(TK_ELEMS / N2 + 1) / 2, 256, 0, st>>>(c->tk, TK_ELEMS / N2, ninv2);
  // the KSK goes to the device once, as the int8 limbs of the matrix-core key switch (88 MB)
  DevBuf<uint32_t> ksk;
  HIP_TRY(ksk.alloc(KSK_ELEMS + 64));
  HIP_TRY(hipMemcpyAsync(ksk, key->ksk, KSK_ELEMS * sizeof(uint32_t), hipMemcpyDefault, st));
  HIP_TRY(hipMemsetAsync(ksk + KSK_ELEMS, 0, 64 * sizeof(uint32_t), st));
  ksk_to_i8_kernel<<<(unsigned)((KSKB_WORDS + 255) / 256), 256, 0, st>>>(ksk, c->kskb);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return OMR_OK;
}

// kappa_r per key row (the a priori bound's key constants), the bounds they give, the guard's
// margin words and which levels the exactness contract guards.
omr_status create_bounds(omr_ctx *c) {
  const size_t rows1 = BSK1_ELEMS / 2 / Fft512::N, rows2 = BSK2_ELEMS / Fft1024::n, rowst = TK_ELEMS / Fft1024::n;
  DevBuf<double> km;
  HIP_TRY(c->margin.alloc(GUARD_WORDS));
  HIP_TRY(km.alloc(rows1 + rows2 + rowst));
  HIP_TRY(hipMemsetAsync(c->margin, 0, GUARD_WORDS * sizeof(unsigned long long), c->stream));
  row_max_abs_kernel<<<(unsigned)rows1, 256, 0, c->stream>>>(c->bsk1f, Fft512::N, km);
  row_max_abs_kernel<<<(unsigned)rows2, 256, 0, c->stream>>>(c->bsk2f, Fft1024::n, km + rows1);
  row_max_abs_kernel<<<(unsigned)rowst, 256, 0, c->stream>>>(c->tkf, Fft1024::n, km + rows1 + rows2);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<double> k1(rows1), k2(rows2), kt(rowst);
  HIP_TRY(hipMemcpy(k1.data(), km, rows1 * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(k2.data(), km + rows1, rows2 * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(kt.data(), km + rows1 + rows2, rowst * sizeof(double), hipMemcpyDeviceToHost));
  c->kappa[0] = *std::max_element(k1.begin(), k1.end());
  c->kappa[1] = *std::max_element(k2.begin(), k2.end());
  c->apriori[0] = apriori_bound(1, k1);
  c->apriori[1] = apriori_bound(2, k2);
  c->apriori_y = apriori_bound(3, k2);
  c->apriori_t = apriori_bound(4, kt);
  c->trace_fft = c->apriori_t < 0.5;
  // the exactness contract: a level whose bound does not prove every rounding exact is guarded
  // on every launch and checked against 1 - E (omr_ctx_exactness)
  for (int l = 0; l < 2; ++l) {
    c->guard_auto[l] = !(c->apriori[l] < 0.5);
    c->thr[l] = 1.0 - c->apriori[l];
  }
  // the fused FFT trace shares level 2's guard word and threshold
  if (c->trace_fft) c->thr[1] = 1.0 - std::max(c->apriori[1], c->apriori_t);
  return c->guard_auto[0] ? ensure_bsk1n(c) : OMR_OK;  // the re-run target of a guarded level 1
}

}  // namespace

extern "C" omr_status omr_ctx_create(const omr_detection_key_view *key, int device, omr_ctx **out) {
  if (!key || !out || !key->bsk1 || !key->ksk || !key->bsk2 || !key->trace_key)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_create: NULL key component");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_create: no such device");
  HIP_TRY(hipSetDevice(device));
  // every early return destroys the half-built context (synchronised first, as omr_ctx_destroy does)
  std::unique_ptr<omr_ctx, decltype(&omr_ctx_destroy)> c(new omr_ctx(), &omr_ctx_destroy);
  c->device = device;
  HIP_TRY(hipDeviceGetAttribute(&c->num_cu, hipDeviceAttributeMultiprocessorCount, device));
  int coop = 0;
  HIP_TRY(hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device));
  // OMR_COOPERATIVE=0: never use the cooperative multi-CU latency kernels (br2l_kernel and
  // trace_kernel run instead, bit-identical); see DESIGN.md §5a on the exit-time fault of
  // processes that made cooperative launches under rocprofv3
  c->coop = coop != 0 && !env_off("OMR_COOPERATIVE");
  c->br2y = !env_off("OMR_BR2Y");
  c->no_prefetch = env_off("OMR_PREFETCH");
  c->no_fast_handoff = env_off("OMR_FAST_HANDOFF");
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->scratch_free, hipEventDisableTiming));
  // the context's error word (a two-CU hand-off timeout) and its pinned copy
  HIP_TRY(c->x_err.alloc(1));
  HIP_TRY(hipMemset(c->x_err, 0, sizeof(int)));
  HIP_TRY(hipHostMalloc((void **)&c->x_err_host, sizeof(int), hipHostMallocDefault));
  *c->x_err_host = 0;
  omr_status s;
  if ((s = create_tables(c.get())) != OMR_OK || (s = create_keys(c.get(), key)) != OMR_OK ||
      (s = create_bounds(c.get())) != OMR_OK)
    return s;
  HIP_TRY(c->ks_part.alloc((size_t)KS_SPLIT * 64 * KSM_COLS * KSM_LIMBS));
  if ((s = ensure_batch(c.get(), c->batch)) != OMR_OK) return s;
  *out = c.release();
  return OMR_OK;
}

extern "C" void omr_ctx_destroy(omr_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->scratch_stream) (void)hipEventSynchronize(c->scratch_free);
  delete c;
}

// Names of the detect-path kernels this build launches (bench.py / profile summaries).
extern "C" const char *omr_detect_kernels(void) {
  return "br1=" OMR_BR1_NAME " ks=" OMR_KS_NAME " br2=" OMR_BR2_NAME;
}

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
  c->timing = mode;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_set_rounding_guard(omr_ctx *c, int enable) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_rounding_guard: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  omr_status s;
  if (enable && (s = ensure_bsk1n(c)) != OMR_OK) return s;  // a guarded level-1 launch may re-run exactly
  c->guard = enable != 0;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_set_exact_level1(omr_ctx *c, int enable) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_exact_level1: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  omr_status s;
  if (enable && (s = ensure_bsk1n(c)) != OMR_OK) return s;
  c->exact1 = enable != 0;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_rounding_margin(omr_ctx *c, double observed[2], double apriori[2], double kappa[2],
                                              int reset) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_rounding_margin: NULL ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());  // every guarded launch on any stream has published
  unsigned long long w[2];
  HIP_TRY(hipMemcpy(w, c->margin, sizeof(w), hipMemcpyDeviceToHost));
  for (int l = 0; l < 2; ++l) {
    if (observed) observed[l] = __builtin_bit_cast(double, w[l]);
    if (apriori) apriori[l] = c->apriori[l];
    if (kappa) kappa[l] = c->kappa[l];
  }
  if (reset) HIP_TRY(hipMemset(c->margin, 0, 2 * sizeof(unsigned long long)));
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
    HIP_TRY(hipMemcpy(w, c->margin + 4, sizeof(w), hipMemcpyDeviceToHost));
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
  HIP_TRY(hipMemcpy(out, (level == 1 ? c->bsk1f : c->bsk2f) + first, count * sizeof(double2), hipMemcpyDeviceToHost));
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

namespace {

constexpr int EV_PER_CHUNK = 5;

// Detect D messages of device buffers on st, in chunks of c->batch: per chunk br1f (7 rotations
// per message) -> sum7 -> key switch -> br2 + trace. Stage events per chunk: [0] br1 start,
// [1] br1 end, [2] key switch end, [3] level-2 rotation end, [4] trace end (the trace is its own
// launch on both kernel families since round 5: trace_fft_kernel / trace_x_kernel).
omr_status detect_device(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D,
                         uint64_t *out, hipStream_t st) {
  omr_status s;
  if ((s = take_handoff_error(c)) != OMR_OK) return s;  // an earlier call's output is invalid
  if ((s = ensure_batch(c, std::min(D, c->batch))) != OMR_OK) return s;
  const size_t nchunks = (D + c->batch - 1) / c->batch;
  const bool split = c->timing == 2;
  if (c->timing) {
    while (c->events.size() < nchunks * EV_PER_CHUNK) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      c->events.push_back(e);
    }
    c->timed_messages = D;
    c->timed_chunks = nchunks;
    c->timed_split = true;
  }
  if ((s = scratch_acquire(c, st)) != OMR_OK) return s;
  for (size_t ch = 0; ch < nchunks; ++ch) {
    const size_t off = ch * c->batch;
    const int B = (int)std::min(c->batch, D - off);
    hipEvent_t *ev = c->timing ? &c->events[ch * EV_PER_CHUNK] : nullptr;
    if (ev) HIP_TRY(hipEventRecord(ev[0], st));
    if ((s = launch_first_level(c, B, ca + off * N0, cb + off * CLUES, st, ev)) != OMR_OK) return s;
    if ((s = launch_br2(c, (size_t)B, c->lwe_int, out + off * 2 * N2, 0, st, split, ev ? ev[3] : nullptr)) != OMR_OK)
      return s;
    if (ev) HIP_TRY(hipEventRecord(ev[4], st));
  }
  return scratch_release(c, st);
}

}  // namespace

extern "C" omr_status omr_detect_batch_device(omr_ctx *c, const uint16_t *ca, const uint16_t *cb,
                                              size_t D, uint64_t *out, void *stream) {
  if (!c || (D && (!ca || !cb || !out)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_detect_batch_device: NULL argument");
  if (D == 0) return OMR_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  c->host_timing_valid = false;
  return detect_device(c, ca, cb, D, out, (hipStream_t)stream);  // NULL: HIP's null stream
}

namespace {
omr_status collect_timing(omr_ctx *c, omr_detect_timing *t);
}

namespace {
// omr_detect_batch with c->mu held.
omr_status detect_host_locked(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D, uint64_t *out) {
  HIP_TRY(hipSetDevice(c->device));
  omr_status s;
  const size_t B = std::min(D, c->batch);
  if ((s = stage_buffers(c, B)) != OMR_OK) return s;
  omr_detect_timing acc{};
  acc.trace_separate = 1;
  c->host_timing_valid = false;
  for (size_t off = 0; off < D; off += B) {
    const size_t n = std::min(B, D - off);
    HIP_TRY(hipMemcpyAsync(c->s_clue_a, ca + off * N0, n * N0 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->s_clue_b, cb + off * CLUES, n * CLUES * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    if ((s = detect_device(c, c->s_clue_a, c->s_clue_b, n, c->s_out, c->stream)) != OMR_OK) return s;
    HIP_TRY(hipMemcpyAsync(out + off * 2 * N2, c->s_out, n * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((s = take_handoff_error(c)) != OMR_OK) return s;
    if (c->timing) {
      omr_detect_timing t;
      if ((s = collect_timing(c, &t)) != OMR_OK) return s;
      acc.first_level_ms += t.first_level_ms;
      acc.key_switch_ms += t.key_switch_ms;
      acc.second_level_ms += t.second_level_ms;
      acc.trace_ms += t.trace_ms;
      acc.total_ms += t.total_ms;
      acc.messages += t.messages;
      acc.trace_separate &= t.trace_separate;
    }
  }
  if (c->timing) {
    c->host_timing = acc;
    c->host_timing_valid = true;
  }
  return OMR_OK;
}
}  // namespace

extern "C" omr_status omr_detect_batch(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D,
                                       uint64_t *out) {
  if (!c || (D && (!ca || !cb || !out)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_detect_batch: NULL argument");
  if (D == 0) return OMR_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  return detect_host_locked(c, ca, cb, D, out);
}

// Detector::detect (detector.rs:135-138) for one message, callable from many host threads at once
// (the reference's `clues.par_iter().map(|c| detector.detect(c))`, examples/omr.rs:160-164, on a
// shared &Detector): the requests queue on the context; whichever caller finds no launch in
// progress becomes the leader, optionally waits coalesce_window_us for more, gathers up to
// coalesce_max queued clues into one omr_detect_batch (latency kernels up to the threshold,
// throughput kernels above), scatters the outputs and wakes their callers; the next leader takes
// what queued meanwhile. Every caller gets its batch's status and error message.
extern "C" omr_status omr_detect(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, uint64_t *out) {
  if (!c || !ca || !cb || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_detect: NULL argument");
  omr_ctx::DetectReq r{ca, cb, out, OMR_OK, std::string(), false};
  std::unique_lock<std::mutex> lk(c->qmu);
  c->queue.push_back(&r);
  c->qcv.notify_all();  // a leader inside its window may be waiting for a full batch
  while (!r.done) {
    if (c->leader) {
      c->qcv.wait(lk);
      continue;
    }
    c->leader = true;
    if (c->coalesce_window_us > 0 && c->queue.size() < c->coalesce_max)
      c->qcv.wait_for(lk, std::chrono::microseconds(c->coalesce_window_us),
                      [&] { return c->queue.size() >= c->coalesce_max; });
    const size_t n = std::min(c->queue.size(), c->coalesce_max);
    std::vector<omr_ctx::DetectReq *> batch(c->queue.begin(), c->queue.begin() + (long)n);
    c->queue.erase(c->queue.begin(), c->queue.begin() + (long)n);
    lk.unlock();
    // gather, launch, scatter: nothing may throw out of this extern "C" function, and the leader
    // flag must be cleared whatever happens (a staging allocation of up to coalesce_max messages
    // can fail): a failure becomes the batch's status
    omr_status st;
    std::string err;
    try {
      std::vector<uint16_t> ga(n * N0), gb(n * CLUES);
      std::vector<uint64_t> go(n * 2 * N2);
      for (size_t k = 0; k < n; ++k) {
        memcpy(&ga[k * N0], batch[k]->a, N0 * sizeof(uint16_t));
        memcpy(&gb[k * CLUES], batch[k]->b, CLUES * sizeof(uint16_t));
      }
      {
        std::lock_guard<std::mutex> dl(c->mu);
        st = detect_host_locked(c, ga.data(), gb.data(), n, go.data());
      }
      if (st == OMR_OK)
        for (size_t k = 0; k < n; ++k) memcpy(batch[k]->out, &go[k * 2 * N2], 2 * N2 * sizeof(uint64_t));
      else
        err = omr_last_error();
    } catch (const std::bad_alloc &) {
      st = OMR_ERR_OUT_OF_MEMORY;
      err = "omr_detect: host staging of the coalesced batch failed";
    } catch (...) {
      st = OMR_ERR_DEVICE;
      err = "omr_detect: unexpected failure while running the coalesced batch";
    }
    lk.lock();
    for (auto *q : batch) {
      q->st = st;
      q->err = err;
      q->done = true;
    }
    c->coalesced_calls += n;
    c->coalesced_launches += 1;
    c->leader = false;
    c->qcv.notify_all();
  }
  return r.st == OMR_OK ? OMR_OK : set_error(r.st, r.err);
}

extern "C" omr_status omr_ctx_set_coalescing(omr_ctx *c, size_t max_messages, long window_us) {
  if (!c || window_us < 0) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_coalescing: bad argument");
  std::lock_guard<std::mutex> lk(c->qmu);
  c->coalesce_max = max_messages ? max_messages : 65536;
  c->coalesce_window_us = window_us;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_coalescing_stats(omr_ctx *c, size_t *calls, size_t *launches) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_coalescing_stats: NULL ctx");
  std::lock_guard<std::mutex> lk(c->qmu);
  if (calls) *calls = c->coalesced_calls;
  if (launches) *launches = c->coalesced_launches;
  return OMR_OK;
}

namespace {
// Stage times of the last detect_device call from its per-chunk events (DetectTimeInfo's split:
// first level includes the key switch, detector.rs:183-191).
omr_status collect_timing(omr_ctx *c, omr_detect_timing *t) {
  memset(t, 0, sizeof(*t));
  if (!c->timing || c->timed_messages == 0) return OMR_OK;
  for (size_t ch = 0; ch < c->timed_chunks; ++ch) {  // the chunk count of the timed call
    hipEvent_t *ev = &c->events[ch * EV_PER_CHUNK];
    HIP_TRY(hipEventSynchronize(ev[4]));
    float a = 0, b = 0, d = 0, e = 0;
    HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
    HIP_TRY(hipEventElapsedTime(&d, ev[2], ev[3]));
    HIP_TRY(hipEventElapsedTime(&e, ev[3], ev[4]));
    t->first_level_ms += a + b;
    t->key_switch_ms += b;
    t->second_level_ms += d;
    t->trace_ms += e;
  }
  t->total_ms = t->first_level_ms + t->second_level_ms + t->trace_ms;
  t->messages = c->timed_messages;
  t->trace_separate = c->timed_split ? 1 : 0;
  return OMR_OK;
}
}  // namespace

extern "C" omr_status omr_last_timing(omr_ctx *c, omr_detect_timing *t) {
  if (!c || !t) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_last_timing: NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->host_timing_valid) {
    *t = c->host_timing;
    return OMR_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  return collect_timing(c, t);
}

extern "C" omr_status omr_detect_with_time_info(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D,
                                                uint64_t *out, omr_detect_timing *t) {
  if (!c || !t || (D && (!ca || !cb || !out)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_detect_with_time_info: NULL argument");
  memset(t, 0, sizeof(*t));
  t->trace_separate = 1;
  if (D == 0) return OMR_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  const int mode = c->timing;
  c->timing = 2;
  omr_status s = detect_host_locked(c, ca, cb, D, out);
  if (s == OMR_OK) *t = c->host_timing;
  c->timing = mode;
  c->host_timing_valid = mode != 0 && s == OMR_OK;
  return s;
}

// ------------------------------------------------------------------------------------------
// Encode (detector.rs:223-453)
// ------------------------------------------------------------------------------------------
namespace {
// Messages per encode workgroup: at least 32 (128 from D = 16,384), and at most max_chunks
// (default 4,096) chunk partials per ciphertext (scratch n_ct x chunks x 32 KiB: 3.7 GB for 28
// ciphertexts at D = 2^20); above ENC_T messages the index kernel stages its buckets in blocks.
int encode_per_wg(size_t D, size_t max_chunks) {
  const size_t base = D >= 16384 ? 128 : 32;
  return (int)std::max(base, (D + max_chunks - 1) / max_chunks);
}
// The shared tail of the encode entry points: after the encode kernel's launch, reduce the chunk
// partials into the n_ct output ciphertexts (or add them to a running digest), then release the
// scratch.
omr_status encode_finish(omr_ctx *c, int chunks, uint32_t n_ct, uint64_t *out, hipStream_t st, bool accumulate) {
  HIP_TRY(hipGetLastError());
  omr_status s;
  if (accumulate) {
    if ((s = accumulate_partials(c->partial, chunks, n_ct, out, st)) != OMR_OK) return s;
  } else {
    const size_t tot = (size_t)n_ct * 2 * N2;
    reduce_partials_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(c->partial, chunks, (int)n_ct, out);
    HIP_TRY(hipGetLastError());
  }
  return scratch_release(c, st);
}
}  // namespace

// What digest.hip borrows (ctx_internal.hpp).
namespace omr {

std::mutex &ctx_mutex(omr_ctx *c) { return c->mu; }
int ctx_device(const omr_ctx *c) { return c->device; }
size_t ctx_batch(const omr_ctx *c) { return c->batch; }

omr_status detect_device_locked(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D, uint64_t *out,
                                hipStream_t st) {
  c->host_timing_valid = false;
  return detect_device(c, ca, cb, D, out, st);
}

omr_status take_handoff_error_locked(omr_ctx *c) { return take_handoff_error(c); }

omr_status accumulate_partials(const uint64_t *partial, int chunks, uint32_t n_ct, uint64_t *digest,
                               hipStream_t st) {
  const size_t tot = (size_t)n_ct * 2 * N2;
  accumulate_partials_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(partial, chunks, (int)n_ct, digest);
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

omr_status encode_indices_locked(omr_ctx *c, const uint64_t *pv, size_t D, size_t offset, size_t all,
                                 uint64_t seed, uint32_t first_ct, uint32_t n_ct, uint64_t *out, hipStream_t st,
                                 bool accumulate) {
  omr_retrieval_params rp;
  omr_status s;
  if ((s = omr_get_retrieval_params(all, 0, &rp)) != OMR_OK) return s;
  if (D == 0) {
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_ct * 2 * N2 * sizeof(uint64_t), st));
    return OMR_OK;
  }
  const int per_wg = encode_per_wg(D, c->enc_max_chunks);
  const int chunks = (int)((D + per_wg - 1) / per_wg);
  if ((s = ensure_partial(c, (size_t)n_ct * chunks * 2 * N2)) != OMR_OK) return s;
  if ((s = scratch_acquire(c, st)) != OMR_OK) return s;
  EncodeLayout ly{(int)rp.index_slots_per_bucket, (int)rp.slots_per_bucket,
                  (int)rp.slots_per_segment, (int)rp.segment_per_cipher};
  encode_indices_kernel<<<dim3(chunks, n_ct), ENC_T, 0, st>>>(pv, (int)D, offset, ly, seed, first_ct,
                                                              per_wg, c->tb.tw2, c->partial);
  return encode_finish(c, chunks, n_ct, out, st, accumulate);
}

omr_status encode_payloads_locked(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads, size_t D,
                                  size_t offset, size_t all, const uint16_t *weights, uint32_t n_ct,
                                  uint32_t per_ct, uint64_t *out, hipStream_t st, bool accumulate) {
  if (D == 0) {
    if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_ct * 2 * N2 * sizeof(uint64_t), st));
    return OMR_OK;
  }
  const int per_wg = encode_per_wg(D, c->enc_max_chunks);
  const int chunks = (int)((D + per_wg - 1) / per_wg);
  omr_status s;
  if ((s = ensure_partial(c, (size_t)n_ct * chunks * 2 * N2)) != OMR_OK) return s;
  if ((s = scratch_acquire(c, st)) != OMR_OK) return s;
  encode_payloads_kernel<<<dim3(chunks, n_ct), ENC_T, 0, st>>>(pv, payloads, (int)D, offset, all,
                                                               weights, (int)per_ct, per_wg,
                                                               c->tb.tw2, c->partial);
  return encode_finish(c, chunks, n_ct, out, st, accumulate);
}

}  // namespace omr

extern "C" omr_status omr_encode_indices_device(omr_ctx *c, const uint64_t *pv, size_t D,
                                                size_t offset, size_t all, uint64_t seed,
                                                uint32_t first_ct, uint32_t n_ct, uint64_t *out,
                                                void *stream) {
  if (!c || !out || (D && !pv) || n_ct == 0 || offset + D > all || D > (size_t)INT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_indices_device: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // NULL: HIP's null stream
  return encode_indices_locked(c, pv, D, offset, all, seed, first_ct, n_ct, out, (hipStream_t)stream, false);
}

extern "C" omr_status omr_encode_payloads_device(omr_ctx *c, const uint64_t *pv,
                                                 const uint16_t *payloads, size_t D, size_t offset,
                                                 size_t all, const uint16_t *weights, uint32_t n_ct,
                                                 uint32_t per_ct, uint64_t *out, void *stream) {
  if (!c || !out || (D && (!pv || !payloads || !weights)) || n_ct == 0 || per_ct == 0 ||
      per_ct * PAYLOAD_LEN > (uint32_t)N2 || offset + D > all || D > (size_t)INT32_MAX)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_payloads_device: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // NULL: HIP's null stream
  return encode_payloads_locked(c, pv, payloads, D, offset, all, weights, n_ct, per_ct, out, (hipStream_t)stream,
                                false);
}

extern "C" omr_status omr_encode_indices(omr_ctx *c, const uint64_t *pv, size_t D, size_t offset,
                                         size_t all, uint64_t seed, uint32_t ct, uint64_t *out) {
  if (!c || !out || (D && !pv)) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_indices");
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint64_t> dpv, dout;
  HIP_TRY(dpv.alloc(std::max<size_t>(D, 1) * 2 * N2));
  HIP_TRY(dout.alloc(2 * N2));
  HIP_TRY(hipMemcpy(dpv, pv, D * 2 * N2 * sizeof(uint64_t), hipMemcpyHostToDevice));
  omr_status s = omr_encode_indices_device(c, dpv, D, offset, all, seed, ct, 1, dout, c->stream);
  if (s != OMR_OK) return s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, dout, 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_encode_payloads(omr_ctx *c, const uint64_t *pv, const uint16_t *payloads,
                                          size_t D, size_t offset, size_t all,
                                          const uint16_t *weights, uint32_t n_ct, uint32_t per_ct,
                                          uint64_t *out) {
  if (!c || !out || (D && (!pv || !payloads || !weights)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_encode_payloads");
  HIP_TRY(hipSetDevice(c->device));
  const size_t wn = (size_t)n_ct * per_ct * all;
  DevBuf<uint64_t> dpv, dout;
  DevBuf<uint16_t> dpay, dw;
  HIP_TRY(dpv.alloc(std::max<size_t>(D, 1) * 2 * N2));
  HIP_TRY(dpay.alloc(std::max<size_t>(D, 1) * PAYLOAD_LEN));
  HIP_TRY(dw.alloc(std::max<size_t>(wn, 1)));
  HIP_TRY(dout.alloc((size_t)n_ct * 2 * N2));
  HIP_TRY(hipMemcpy(dpv, pv, D * 2 * N2 * sizeof(uint64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dpay, payloads, D * PAYLOAD_LEN * sizeof(uint16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dw, weights, wn * sizeof(uint16_t), hipMemcpyHostToDevice));
  omr_status s = omr_encode_payloads_device(c, dpv, dpay, D, offset, all, dw, n_ct, per_ct,
                                            dout, c->stream);
  if (s != OMR_OK) return s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, dout, (size_t)n_ct * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

// ------------------------------------------------------------------------------------------
// Stage entry points (parity tests, per-stage benchmarks)
// ------------------------------------------------------------------------------------------
extern "C" omr_status omr_first_level(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D,
                                      uint32_t *lwe_int) {
  if (!c || !ca || !cb || !lwe_int || D == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_first_level: bad argument (D <= batch)");
  std::lock_guard<std::mutex> lk(c->mu);
  if (D > c->batch) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_first_level: bad argument (D <= batch)");
  HIP_TRY(hipSetDevice(c->device));
  omr_status s;
  if ((s = stage_buffers(c, D)) != OMR_OK || (s = ensure_batch(c, D)) != OMR_OK) return s;
  hipStream_t st = c->stream;
  if ((s = scratch_acquire(c, st)) != OMR_OK) return s;
  HIP_TRY(hipMemcpyAsync(c->s_clue_a, ca, D * N0 * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(c->s_clue_b, cb, D * CLUES * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  if ((s = launch_first_level(c, (int)D, c->s_clue_a, c->s_clue_b, st)) != OMR_OK) return s;
  HIP_TRY(hipMemcpyAsync(lwe_int, c->lwe_int, D * (NI + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if ((s = scratch_release(c, st)) != OMR_OK) return s;
  HIP_TRY(hipStreamSynchronize(st));
  return OMR_OK;
}

extern "C" omr_status omr_fft1_mul(omr_ctx *c, const uint32_t *a, const uint32_t *k, size_t n,
                                   uint64_t *out) {
  if (!c || !a || !k || !out || n == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_fft1_mul: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint32_t> da, dk;
  DevBuf<uint64_t> dout;
  HIP_TRY(da.alloc(n * N1));
  HIP_TRY(dk.alloc(n * N1));
  HIP_TRY(dout.alloc(n * N1));
  HIP_TRY(hipMemcpy(da, a, n * N1 * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dk, k, n * N1 * sizeof(uint32_t), hipMemcpyHostToDevice));
  fft1_mul_kernel<<<(unsigned)n, 64, 0, c->stream>>>(da, dk, dout, c->fft1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, dout, n * N1 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_blind_rotate_level1(omr_ctx *c, const uint16_t *la, const uint16_t *lb,
                                              size_t n, uint64_t *out) {
  if (!c || !la || !lb || !out || n == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_blind_rotate_level1: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint16_t> da, db;
  DevBuf<uint64_t> dout;
  HIP_TRY(da.alloc(n * N0));
  HIP_TRY(db.alloc(n));
  HIP_TRY(dout.alloc(n * 2 * N1));
  HIP_TRY(hipMemcpy(da, la, n * N0 * sizeof(uint16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(db, lb, n * sizeof(uint16_t), hipMemcpyHostToDevice));
  // a pending hand-off error belongs to an earlier detect call: report it before this launch (as
  // detect_device does) instead of discarding a valid level-1 output after it
  omr_status s;
  if ((s = take_handoff_error(c)) != OMR_OK) return s;
  // the guarded sequence (guard_begin, guard kernel, br1n_fallback, guard_fold) uses the context's
  // per-launch margin word, shared with every other call: serialise it with them like any scratch
  if ((s = scratch_acquire(c, c->stream)) != OMR_OK) return s;
  if ((s = launch_br1(c, n, nullptr, nullptr, da, db, nullptr, dout, 1, c->stream, n)) != OMR_OK) return s;
  if ((s = scratch_release(c, c->stream)) != OMR_OK) return s;
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, dout, n * 2 * N1 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

static omr_status second_level_impl(omr_ctx *c, const uint32_t *lwe, size_t n, uint64_t *out,
                                    int mode) {
  if (!c || !lwe || !out || n == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_second_level: bad argument");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint32_t> dl;
  DevBuf<uint64_t> dout;
  HIP_TRY(dl.alloc(n * (NI + 1)));
  HIP_TRY(dout.alloc(n * 2 * N2));
  HIP_TRY(hipMemcpy(dl, lwe, n * (NI + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  omr_status ls;
  if ((ls = take_handoff_error(c)) != OMR_OK) return ls;
  if ((ls = scratch_acquire(c, c->stream)) != OMR_OK) return ls;  // the hand-off slots are scratch
  if ((ls = launch_br2(c, n, dl, dout, mode, c->stream)) != OMR_OK) return ls;
  if ((ls = scratch_release(c, c->stream)) != OMR_OK) return ls;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((ls = take_handoff_error(c)) != OMR_OK) return ls;
  HIP_TRY(hipMemcpy(out, dout, n * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_second_level(omr_ctx *c, const uint32_t *lwe, size_t n, uint64_t *out) {
  return second_level_impl(c, lwe, n, out, 0);
}
extern "C" omr_status omr_blind_rotate_level2(omr_ctx *c, const uint32_t *lwe, size_t n,
                                              uint64_t *out) {
  return second_level_impl(c, lwe, n, out, 1);
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

#ifdef OMR_PHASE_TRACE
// Debug builds only (tools/phase_trace.py): copy the latency kernels' phase timestamps.
extern "C" int omr_debug_phase_read(unsigned long long *host, size_t n) {
  const size_t cap = sizeof(omr::omr_phase_buf) / sizeof(unsigned long long);
  if (n > cap) n = cap;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(omr::omr_phase_buf), n * sizeof(unsigned long long)) == hipSuccess
             ? (int)n
             : -1;
}
#endif
