// Detect: every rotation, key-switch and trace launch with the cooperative-launch and guard
// plumbing, detect on device and host buffers, the stage timing and the per-stage entry points.
//
// Detector::detect (detector.rs:135-166) for a batch of messages -> per chunk br1f_kernel (7 blind
// rotations per message), sum7_kernel, ks_mfma_kernel, br2f_kernel (level-2 rotation on the exact
// FFT) and trace_fft_kernel; chunks up to the latency threshold run the latency kernels instead.
// One translation unit for both levels: guard_fold_kernel and the phase-trace buffer (handoff.hpp,
// -DOMR_PHASE_TRACE) serve both.
#include <algorithm>
#include <cstring>
#include <string>

#include "br1_fft.hpp"
#include "br1_latency.hpp"
#include "br1_ntt.hpp"
#include "br2_fft.hpp"
#include "br2_ntt.hpp"
#include "ctx.hpp"
#include "ks_mfma.hpp"
#include "two_cu_from.hpp"

using namespace omr;

#define OMR_BR1_NAME "br1f_kernel"
#define OMR_KS_NAME "ks_mfma_kernel"
#define OMR_BR2_NAME "br2f_kernel"

// Names of the detect-path kernels this build launches (bench.py / profile summaries).
extern "C" const char *omr_detect_kernels(void) {
  return "br1=" OMR_BR1_NAME " ks=" OMR_KS_NAME " br2=" OMR_BR2_NAME;
}

// The two-CU kernel's bounded hand-off wait: a workgroup whose partner never published leaves its
// loop and sets x_err; each launch then copies x_err to the pinned x_err_host on its stream. This
// reports (and clears) an error whose copy has landed: callers sync the stream first for a
// definitive answer (omr_ctx_check, the host entry points), or call it before enqueueing new work
// (the device entry points) so a failed earlier call is never attributed to a later one.
omr_status omr::take_handoff_error(omr_ctx *c) {
  if (!c->ho.x_err_host || !__atomic_load_n(c->ho.x_err_host, __ATOMIC_ACQUIRE)) return OMR_OK;
  HIP_TRY(hipDeviceSynchronize());  // no launch may still be copying the flag
  (void)__atomic_exchange_n(c->ho.x_err_host, 0, __ATOMIC_ACQ_REL);
  HIP_TRY(hipMemset(c->ho.x_err, 0, sizeof(int)));
  return set_error(OMR_ERR_DEVICE,
                   "level-2 two-CU hand-off timed out: the output of an earlier detect call on this "
                   "context is invalid");
}

// After a guarded launch and its conditional exact re-run: fold the launch's margin (word 2 + level,
// exactness.hpp) into the cumulative word and count a breach.
namespace omr {
__global__ void guard_fold_kernel(unsigned long long *words, int level, double thr) {
  if (threadIdx.x != 0) return;
  const unsigned long long m = words[2 + level];
  atomicMax(&words[level], m);
  if (__longlong_as_double((long long)m) >= thr) atomicAdd(&words[4 + level], 1ull);
}
}  // namespace omr

namespace {

bool latency_path(const omr_ctx *c, size_t n) { return n <= c->latency_max; }

// The launch record (omr_ctx_launch_record): one more launch of `kind`, where the choice is made.
void note_launch(omr_ctx *c, omr_launch_kind kind) { ++c->launches[kind]; }

// Zero the per-launch guard word of `level` before a guarded launch.
omr_status guard_begin(omr_ctx *c, int level, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(c->ex.margin + 2 + level, 0, sizeof(unsigned long long), st));
  return OMR_OK;
}
omr_status guard_end(omr_ctx *c, int level, hipStream_t st) {
  guard_fold_kernel<<<1, 64, 0, st>>>(c->ex.margin, level, c->ex.thr[level]);
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// LWE key switch + modulus switch of B messages (lwe1t [1025][B] -> out [B][671]). Up to 64
// messages (the latency path) the input coefficients are split over KS_SPLIT workgroup slices.
omr_status launch_ks(omr_ctx *c, int B, uint32_t *out, hipStream_t st) {
  const omr_ctx::Scratch &s = c->scr;
  if (latency_path(c, (size_t)B) && B <= 64) {
    ks_mfma_split_kernel<<<dim3(1, KSM_COLS / 32, KS_SPLIT), 64, 0, st>>>(s.lwe1t, c->keys.kskb, s.ks_part, B, 64);
    HIP_TRY(hipGetLastError());
    ks_combine_kernel<<<(B * (NI + 1) + 255) / 256, 256, 0, st>>>(s.ks_part, s.lwe1t, out, B, 64);
  } else {
    ks_mfma_kernel<<<dim3((B + 63) / 64, KSM_COLS / 32), 64, 0, st>>>(s.lwe1t, c->keys.kskb, out, B);
  }
  HIP_TRY(hipGetLastError());
  return OMR_OK;
}

// Level-1 blind rotations of n (message, clue) pairs (mode 0: clue g % 7 of message g / 7 ->
// extracted LWE; mode 1: explicit LWEs -> full RLWE), BR1F_WPG rotations per workgroup.
// `msgs`: the messages of the chunk (selects the latency kernels, one workgroup per rotation).
// acc0 (the test entry omr_blind_rotate_level1_from): the rotations' initial accumulators (device,
// canonical u64 [n][2][N1]); the same selection, on each kernel's _from instantiation.
omr_status launch_br1(omr_ctx *c, size_t n, const uint16_t *ca, const uint16_t *cb,
                      const uint16_t *la, const uint16_t *lb, uint32_t *ext, uint64_t *rlwe, int mode,
                      hipStream_t st, size_t msgs, const uint64_t *acc0 = nullptr) {
  const omr_ctx::Keys &k = c->keys;
  const DeviceTables &tb = c->tab.tb;
  unsigned long long *word = c->ex.margin + 2;
  if (c->ex.exact1) {  // the reference's arithmetic for every rotation (omr_ctx_set_exact_level1)
    if (acc0)
      br1n_from_kernel<<<(unsigned)n, 64, 0, st>>>(ca, cb, la, lb, k.bsk1n, tb, ext, rlwe, mode, n, nullptr, 0.0, acc0);
    else
      br1n_kernel<<<(unsigned)n, 64, 0, st>>>(ca, cb, la, lb, k.bsk1n, tb, ext, rlwe, mode, n);
    HIP_TRY(hipGetLastError());
    return OMR_OK;
  }
  const unsigned g1 = (unsigned)((n + BR1F_WPG - 1) / BR1F_WPG);
  const bool g = guarded(c, 0);
  if (g) OMR_TRY(guard_begin(c, 0, st));
  if (acc0) {
    if (latency_path(c, msgs)) {
      if (g)
        br1l_guard_from_kernel<<<(unsigned)n, 64 * BR1L_WAVES, 0, st>>>(ca, cb, la, lb, k.bsk1l, tb, ext, rlwe, mode,
                                                                         word, acc0);
      else
        br1l_from_kernel<<<(unsigned)n, 64 * BR1L_WAVES, 0, st>>>(ca, cb, la, lb, k.bsk1l, tb, ext, rlwe, mode, acc0);
    } else if (g) {
      br1f_guard_from_kernel<<<g1, 64 * BR1F_WPG, 0, st>>>(ca, cb, la, lb, k.bsk1f, tb, ext, rlwe, mode, n, word,
                                                          acc0);
    } else {
      br1f_from_kernel<<<g1, 64 * BR1F_WPG, 0, st>>>(ca, cb, la, lb, k.bsk1f, tb, ext, rlwe, mode, n, acc0);
    }
  } else if (latency_path(c, msgs)) {
    if (g)
      br1l_guard_kernel<<<(unsigned)n, 64 * BR1L_WAVES, 0, st>>>(ca, cb, la, lb, k.bsk1l, tb, ext, rlwe, mode, word);
    else
      br1l_kernel<<<(unsigned)n, 64 * BR1L_WAVES, 0, st>>>(ca, cb, la, lb, k.bsk1l, tb, ext, rlwe, mode);
  } else if (g) {
    br1f_guard_kernel<<<g1, 64 * BR1F_WPG, 0, st>>>(ca, cb, la, lb, k.bsk1f, tb, ext, rlwe, mode, n, word);
  } else {
    br1f_kernel<<<g1, 64 * BR1F_WPG, 0, st>>>(ca, cb, la, lb, k.bsk1f, tb, ext, rlwe, mode, n);
  }
  HIP_TRY(hipGetLastError());
  if (!g) return OMR_OK;
  // the exactness contract: a guarded launch whose margin reached 1 - E1 is recomputed on the exact
  // NTT in the same stream order (every workgroup leaves at once otherwise)
  if (acc0)
    br1n_from_kernel<<<(unsigned)n, 64, 0, st>>>(ca, cb, la, lb, k.bsk1n, tb, ext, rlwe, mode, n, word, c->ex.thr[0],
                                                 acc0);
  else
    br1n_fallback_kernel<<<(unsigned)n, 64, 0, st>>>(ca, cb, la, lb, k.bsk1n, tb, ext, rlwe, mode, n, word,
                                                     c->ex.thr[0]);
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
  HIP_TRY(hipMemcpyAsync(c->ho.x_err_host, c->ho.x_err, sizeof(int), hipMemcpyDeviceToHost, st));
  *launched = true;
  return OMR_OK;
}

// The hand-off slots and flags of a cooperative latency kernel for n messages (shared scratch),
// the flags zeroed on st.
omr_status handoff_scratch(omr_ctx *c, DevBuf<double> &slots, size_t nslots, DevBuf<uint32_t> &flags, size_t nflags,
                           hipStream_t st) {
  if (!slots.fits(nslots) || !flags.fits(nflags)) {
    OMR_TRY(scratch_idle(c));
    HIP_TRY(slots.reserve(nslots));
    HIP_TRY(flags.reserve(nflags));
  }
  HIP_TRY(hipMemsetAsync(flags, 0, nflags * sizeof(uint32_t), st));
  return OMR_OK;
}

// The latency path's level-2 rotation over two CUs per message as a cooperative launch: br2y_kernel
// or br2x_kernel over 2 n workgroups; *launched stays false when it does not fit or is refused, so
// the caller falls back to br2l_kernel. acc0 (optional): the same choice, grid and arguments on
// br2y_from_kernel / br2x_from_kernel (two_cu_from.hip), which take acc0 as one more argument.
omr_status launch_br2xy(omr_ctx *c, size_t n, const uint32_t *lwe_int, uint64_t *out, hipStream_t st,
                        bool *launched, const uint64_t *acc0) {
  omr_ctx::Handoff &h = c->ho;
  *launched = false;
  if (!h.coop || 2 * n > (size_t)h.num_cu) return OMR_OK;  // one 150 KB-LDS workgroup per CU
  // sized for whichever of br2x / br2y runs (handoff.hpp)
  OMR_TRY(handoff_scratch(c, h.x_slots, n * BR2XY_SLOT_DOUBLES, h.x_flags, n * BR2XY_FLAGS, st));
  const double *bsk2 = c->keys.bsk2;
  DeviceTables tb = c->tab.tb;
  double *slots = h.x_slots;
  uint32_t *flags = h.x_flags;
  int *err = h.x_err;
  void *args[] = {(void *)&lwe_int, (void *)&bsk2, (void *)&tb, (void *)&slots, (void *)&flags, (void *)&err,
                  (void *)&out, (void *)&acc0};
  // br2y_kernel (FFT) when the bound of its accumulation order proves it exact and level 2 is not
  // guarded; br2x_kernel's exact NTT otherwise (same arguments apart from the key form)
  const bool y = h.br2y && !guarded(c, 1) && c->ex.apriori_y < 0.5;
  const double2 *bskf = c->keys.bsk2f, *twg = c->tab.fft2;
  // br2y: message m in column m of a grid w8 = n rounded up to 8 columns wide, its mask / body
  // workers in rows 0 / 1, plus 2 BR2Y_H rows of key prefetchers (br2_fft.hpp) when every workgroup
  // still gets a CU of its own
  const int nmsg = (int)n, w8 = (nmsg + 7) / 8 * 8, allow_fast = h.no_fast_handoff ? 0 : 1;
  const int rows = (size_t)w8 * (2 + 2 * BR2Y_H) <= (size_t)h.num_cu && !h.no_prefetch ? 2 + 2 * BR2Y_H : 2;
  if (y && (size_t)w8 * rows > (size_t)h.num_cu) return OMR_OK;  // one workgroup per CU: br2l instead
  void *args_y[] = {(void *)&lwe_int, (void *)&bskf, (void *)&twg, (void *)&tb, (void *)&slots, (void *)&flags,
                    (void *)&err, (void *)&out, (void *)&nmsg, (void *)&w8, (void *)&allow_fast, (void *)&acc0};
  // (the production kernels take the arguments before acc0)
  const void *kern = acc0 ? (y ? br2y_from_kernel_ptr() : br2x_from_kernel_ptr())
                          : (y ? reinterpret_cast<const void *>(&br2y_kernel)
                               : reinterpret_cast<const void *>(&br2x_kernel));
  OMR_TRY(coop_launch(c, "br2x", kern, dim3(y ? (unsigned)(w8 * rows) : (unsigned)(2 * n)), dim3(y ? BR2Y_T : BR2L_T),
                      y ? args_y : args, st, launched));
  if (*launched) {
    note_launch(c, y ? OMR_LAUNCH_BR2Y : OMR_LAUNCH_BR2X);
    if (y && rows > 2) note_launch(c, OMR_LAUNCH_BR2Y_HELPERS);
  }
  return OMR_OK;
}

// The latency path's trace over TRACE_X CUs per message (trace_x_kernel) as a cooperative launch;
// false when refused (the caller then runs trace_kernel, one workgroup per message).
omr_status launch_trace_x(omr_ctx *c, size_t n, uint64_t *io, hipStream_t st, bool *launched) {
  omr_ctx::Handoff &h = c->ho;
  *launched = false;
  if (!h.coop || TRACE_X * n > 2 * (size_t)h.num_cu) return OMR_OK;
  OMR_TRY(handoff_scratch(c, h.t_slots, n * TRACE_X_SLOT_DOUBLES, h.t_flags, n * TRACE_X_FLAGS, st));
  const double *tk = c->keys.tk;
  DeviceTables tb = c->tab.tb;
  double *slots = h.t_slots;
  uint32_t *flags = h.t_flags;
  int *err = h.x_err;
  void *args[] = {(void *)&io, (void *)&tk, (void *)&tb, (void *)&slots, (void *)&flags, (void *)&err};
  return coop_launch(c, "trace_x", reinterpret_cast<const void *>(&trace_x_kernel), dim3((unsigned)(TRACE_X * n)),
                     dim3(BR2_T), args, st, launched);
}

// The trace of n level-2 rotations in place (launch_br2's mode 0): on the FFT when its a priori bound
// allows (throughput; g: the guarded kernel), else the NTT; over TRACE_X CUs per message on the
// latency path when the cooperative launch fits.
omr_status launch_trace(omr_ctx *c, size_t n, uint64_t *out, hipStream_t st, bool lat, bool g) {
  const omr_ctx::Keys &k = c->keys;
  const DeviceTables &tb = c->tab.tb;
  const double2 *fft2 = c->tab.fft2;
  bool multi = false;
  if (lat) OMR_TRY(launch_trace_x(c, n, out, st, &multi));
  omr_launch_kind kind = OMR_LAUNCH_TRACE_X;
  if (lat || !c->ex.trace_fft) {
    if (!multi) {
      trace_kernel<<<(unsigned)n, BR2_T, 0, st>>>(out, k.tk, tb);
      kind = OMR_LAUNCH_TRACE_KERNEL;
    }
  } else if (g) {
    trace_fft_guard_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(out, k.tkf, fft2, tb, c->ex.margin + 3);
    kind = OMR_LAUNCH_TRACE_FFT_GUARD;
  } else {
    trace_fft_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(out, k.tkf, fft2, tb);
    kind = OMR_LAUNCH_TRACE_FFT;
  }
  HIP_TRY(hipGetLastError());
  note_launch(c, kind);
  return OMR_OK;
}

// Level-2 blind rotation of n LWE(670, 4096) ciphertexts and (mode 0) the trace, always a launch of
// its own; `mid` (optional) is recorded between the two. The latency path gives a message two CUs
// (or two 4-wave groups) and traces in place. The throughput path's exactness contract: a guarded
// pair notes both kernels' rounding margins in level 2's word, and a pair whose margin reaches the
// threshold is re-run on the exact NTT (every workgroup of the fallbacks leaves at once otherwise).
// acc0 (the test entry omr_blind_rotate_level2_from): the initial accumulators (device, canonical
// u64 [n][2][N2]); the same selection, on each kernel's _from instantiation -- on the latency path the
// two-CU br2y_from_kernel / br2x_from_kernel, and br2l_from_kernel only where br2l_kernel would run
// (the cooperative launch does not fit or is refused).
omr_status launch_br2(omr_ctx *c, size_t n, const uint32_t *lwe_int, uint64_t *out, int mode, hipStream_t st,
                      hipEvent_t mid = nullptr, const uint64_t *acc0 = nullptr) {
  const omr_ctx::Keys &k = c->keys;
  const DeviceTables &tb = c->tab.tb;
  const double2 *fft2 = c->tab.fft2;
  unsigned long long *word = c->ex.margin + 3;
  const bool lat = latency_path(c, n), g = !lat && guarded(c, 1);
  if (lat) {
    bool two_cu = false;
    OMR_TRY(launch_br2xy(c, n, lwe_int, out, st, &two_cu, acc0));  // notes br2y / br2x when it launched
    if (!two_cu) {
      if (acc0)
        br2l_from_kernel<<<(unsigned)n, BR2L_T, 0, st>>>(lwe_int, k.bsk2, tb, out, nullptr, 0.0, acc0);
      else
        br2l_kernel<<<(unsigned)n, BR2L_T, 0, st>>>(lwe_int, k.bsk2, tb, out);
      note_launch(c, OMR_LAUNCH_BR2L);
    }
  } else if (g) {
    note_launch(c, OMR_LAUNCH_BR2F_GUARD);
    OMR_TRY(guard_begin(c, 1, st));
    if (acc0)
      br2f_guard_from_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(lwe_int, k.bsk2f, fft2, tb, out, word, acc0);
    else
      br2f_guard_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(lwe_int, k.bsk2f, fft2, tb, out, word);
  } else {
    note_launch(c, OMR_LAUNCH_BR2F);
    if (acc0)
      br2f_from_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(lwe_int, k.bsk2f, fft2, tb, out, acc0);
    else
      br2f_kernel<<<(unsigned)n, Fft1024::T, 0, st>>>(lwe_int, k.bsk2f, fft2, tb, out);
  }
  if (acc0) note_launch(c, OMR_LAUNCH_BR2_FROM);
  HIP_TRY(hipGetLastError());
  if (mid) HIP_TRY(hipEventRecord(mid, st));
  if (mode == 0) OMR_TRY(launch_trace(c, n, out, st, lat, g));
  if (!g) return OMR_OK;
  note_launch(c, OMR_LAUNCH_GUARD_FALLBACK);
  if (acc0)
    br2l_from_kernel<<<(unsigned)n, BR2L_T, 0, st>>>(lwe_int, k.bsk2, tb, out, word, c->ex.thr[1], acc0);
  else
    br2l_fallback_kernel<<<(unsigned)n, BR2L_T, 0, st>>>(lwe_int, k.bsk2, tb, out, word, c->ex.thr[1]);
  HIP_TRY(hipGetLastError());
  if (mode == 0) trace_fallback_kernel<<<(unsigned)n, BR2_T, 0, st>>>(out, k.tk, tb, word, c->ex.thr[1]);
  HIP_TRY(hipGetLastError());
  return guard_end(c, 1, st);
}

// The trace alone, in place on n coefficient-domain RLWEs (the test entry omr_trace): launch_br2's
// mode-0 selection, guard and fallback without a rotation. A guarded run saves the input first: the
// FFT trace works in place, and the fallback recomputes from the input.
omr_status launch_trace_only(omr_ctx *c, size_t n, uint64_t *io, uint64_t *saved, hipStream_t st) {
  const bool lat = latency_path(c, n), g = !lat && guarded(c, 1);
  if (g) {
    OMR_TRY(guard_begin(c, 1, st));
    HIP_TRY(hipMemcpyAsync(saved, io, n * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  }
  OMR_TRY(launch_trace(c, n, io, st, lat, g));
  if (!g) return OMR_OK;
  note_launch(c, OMR_LAUNCH_GUARD_FALLBACK);
  trace_restore_kernel<<<(unsigned)n, BR2_T, 0, st>>>(io, saved, c->ex.margin + 3, c->ex.thr[1]);
  HIP_TRY(hipGetLastError());
  trace_fallback_kernel<<<(unsigned)n, BR2_T, 0, st>>>(io, c->keys.tk, c->tab.tb, c->ex.margin + 3, c->ex.thr[1]);
  HIP_TRY(hipGetLastError());
  return guard_end(c, 1, st);
}

// The first level after its rotations: the seven extracted LWEs of each of B messages in scr.ext ->
// sum7 -> key switch into scr.lwe_int (launch_first_level, and the stage entry omr_sum_key_switch).
omr_status launch_sum_ks(omr_ctx *c, int B, hipStream_t st) {
  const size_t n7 = (size_t)B * (N1 + 1);
  sum7_kernel<<<(unsigned)((n7 + 255) / 256), 256, 0, st>>>(c->scr.ext, c->scr.lwe1t, B);
  return launch_ks(c, B, c->scr.lwe_int, st);
}

// The first level of B messages: br1 (7 rotations per message) -> sum7 -> key switch into
// scr.lwe_int. With ev (detect_device's stage events) ev[1] is recorded after br1, ev[2] after the
// key switch.
omr_status launch_first_level(omr_ctx *c, int B, const uint16_t *ca, const uint16_t *cb, hipStream_t st,
                              hipEvent_t *ev = nullptr) {
  OMR_TRY(launch_br1(c, (size_t)B * CLUES, ca, cb, nullptr, nullptr, c->scr.ext, nullptr, 0, st, (size_t)B));
  if (ev) HIP_TRY(hipEventRecord(ev[1], st));
  OMR_TRY(launch_sum_ks(c, B, st));
  if (ev) HIP_TRY(hipEventRecord(ev[2], st));
  return OMR_OK;
}

constexpr int EV_PER_CHUNK = 5;

// Stage times of the last detect_device call from its per-chunk events (DetectTimeInfo's split:
// first level includes the key switch, detector.rs:183-191).
omr_status collect_timing(omr_ctx *c, omr_detect_timing *t) {
  memset(t, 0, sizeof(*t));
  t->trace_separate = 1;
  if (!c->tm.mode || c->tm.messages == 0) return OMR_OK;
  for (size_t ch = 0; ch < c->tm.chunks; ++ch) {  // the chunk count of the timed call
    hipEvent_t *ev = &c->tm.events[ch * EV_PER_CHUNK];
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
  t->messages = c->tm.messages;
  return OMR_OK;
}

}  // namespace

// Per chunk of c->batch messages: br1 (7 rotations per message) -> sum7 -> key switch -> br2 ->
// trace. Stage events per chunk when timed: [0] br1 start, [1] br1 end, [2] key switch end,
// [3] level-2 rotation end, [4] trace end.
omr_status omr::detect_device(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D, uint64_t *out,
                              hipStream_t st) {
  c->tm.host_valid = false;
  OMR_TRY(take_handoff_error(c));  // an earlier call's output is invalid
  OMR_TRY(ensure_batch(c, std::min(D, c->batch)));
  const size_t nchunks = (D + c->batch - 1) / c->batch;
  if (c->tm.mode) {
    while (c->tm.events.size() < nchunks * EV_PER_CHUNK) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      c->tm.events.push_back(e);
    }
    c->tm.messages = D;
    c->tm.chunks = nchunks;
  }
  ScratchLease lease;
  OMR_TRY(lease.acquire(c, st));
  for (size_t ch = 0; ch < nchunks; ++ch) {
    const size_t off = ch * c->batch;
    const int B = (int)std::min(c->batch, D - off);
    hipEvent_t *ev = c->tm.mode ? &c->tm.events[ch * EV_PER_CHUNK] : nullptr;
    if (ev) HIP_TRY(hipEventRecord(ev[0], st));
    OMR_TRY(launch_first_level(c, B, ca + off * N0, cb + off * CLUES, st, ev));
    OMR_TRY(launch_br2(c, (size_t)B, c->scr.lwe_int, out + off * 2 * N2, 0, st, ev ? ev[3] : nullptr));
    if (ev) HIP_TRY(hipEventRecord(ev[4], st));
  }
  return lease.release();
}

extern "C" omr_status omr_detect_batch_device(omr_ctx *c, const uint16_t *ca, const uint16_t *cb,
                                              size_t D, uint64_t *out, void *stream) {
  if (!c || (D && (!ca || !cb || !out)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_detect_batch_device: NULL argument");
  if (D == 0) return OMR_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  return detect_device(c, ca, cb, D, out, (hipStream_t)stream);  // NULL: HIP's null stream
}

omr_status omr::detect_host(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D, uint64_t *out) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t B = std::min(D, c->batch);
  OMR_TRY(stage_buffers(c, B));
  const omr_ctx::Scratch &s = c->scr;
  omr_detect_timing acc{};
  acc.trace_separate = 1;
  c->tm.host_valid = false;
  for (size_t off = 0; off < D; off += B) {
    const size_t n = std::min(B, D - off);
    HIP_TRY(hipMemcpyAsync(s.s_clue_a, ca + off * N0, n * N0 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s.s_clue_b, cb + off * CLUES, n * CLUES * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    OMR_TRY(detect_device(c, s.s_clue_a, s.s_clue_b, n, s.s_out, c->stream));
    HIP_TRY(hipMemcpyAsync(out + off * 2 * N2, s.s_out, n * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    OMR_TRY(take_handoff_error(c));
    if (c->tm.mode) {
      omr_detect_timing t;
      OMR_TRY(collect_timing(c, &t));
      acc.first_level_ms += t.first_level_ms;
      acc.key_switch_ms += t.key_switch_ms;
      acc.second_level_ms += t.second_level_ms;
      acc.trace_ms += t.trace_ms;
      acc.total_ms += t.total_ms;
      acc.messages += t.messages;
    }
  }
  if (c->tm.mode) {
    c->tm.host = acc;
    c->tm.host_valid = true;
  }
  return OMR_OK;
}

extern "C" omr_status omr_detect_batch(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, size_t D,
                                       uint64_t *out) {
  if (!c || (D && (!ca || !cb || !out)))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_detect_batch: NULL argument");
  if (D == 0) return OMR_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  return detect_host(c, ca, cb, D, out);
}

extern "C" omr_status omr_last_timing(omr_ctx *c, omr_detect_timing *t) {
  if (!c || !t) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_last_timing: NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->tm.host_valid) {
    *t = c->tm.host;
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
  const int mode = c->tm.mode;
  c->tm.mode = 1;  // timed for this call, whatever the caller's mode
  omr_status s = detect_host(c, ca, cb, D, out);
  if (s == OMR_OK) *t = c->tm.host;
  c->tm.mode = mode;
  c->tm.host_valid = mode != 0 && s == OMR_OK;
  return s;
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
  OMR_TRY(stage_buffers(c, D));
  OMR_TRY(ensure_batch(c, D));
  const omr_ctx::Scratch &s = c->scr;
  hipStream_t st = c->stream;
  ScratchLease lease;
  OMR_TRY(lease.acquire(c, st));
  HIP_TRY(hipMemcpyAsync(s.s_clue_a, ca, D * N0 * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(s.s_clue_b, cb, D * CLUES * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  OMR_TRY(launch_first_level(c, (int)D, s.s_clue_a, s.s_clue_b, st));
  HIP_TRY(hipMemcpyAsync(lwe_int, s.lwe_int, D * (NI + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  OMR_TRY(lease.release());
  HIP_TRY(hipStreamSynchronize(st));
  return OMR_OK;
}

// launch_first_level after its rotations, on caller-supplied extracted LWEs: ext goes where br1 writes
// it (scr.ext), then sum7 and launch_ks exactly as there.
extern "C" omr_status omr_sum_key_switch(omr_ctx *c, const uint32_t *ext, size_t n, uint32_t *lwe_int) {
  if (!c || !ext || !lwe_int || n == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sum_key_switch: bad argument (n <= batch)");
  std::lock_guard<std::mutex> lk(c->mu);
  if (n > c->batch) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sum_key_switch: bad argument (n <= batch)");
  const size_t words = n * CLUES * (N1 + 1);
  for (size_t i = 0; i < words; ++i)
    if (ext[i] >= (uint32_t)Q1)
      return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_sum_key_switch: ext holds a word >= q1");
  HIP_TRY(hipSetDevice(c->device));
  OMR_TRY(take_handoff_error(c));  // an earlier detect call's, never this call's (as detect_device does)
  OMR_TRY(ensure_batch(c, n));
  const omr_ctx::Scratch &s = c->scr;
  hipStream_t st = c->stream;
  ScratchLease lease;
  OMR_TRY(lease.acquire(c, st));
  HIP_TRY(hipMemcpyAsync(s.ext, ext, words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  OMR_TRY(launch_sum_ks(c, (int)n, st));
  HIP_TRY(hipMemcpyAsync(lwe_int, s.lwe_int, n * (NI + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  OMR_TRY(lease.release());
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
  fft1_mul_kernel<<<(unsigned)n, 64, 0, c->stream>>>(da, dk, dout, c->tab.fft1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, dout, n * N1 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

// Every word of a caller-supplied accumulator below q (host, before anything is enqueued).
static bool canonical_words(const uint64_t *v, size_t count, uint64_t q) {
  for (size_t i = 0; i < count; ++i)
    if (v[i] >= q) return false;
  return true;
}

static omr_status blind_rotate_level1_impl(omr_ctx *c, const uint16_t *la, const uint16_t *lb, size_t n,
                                           const uint64_t *acc0, uint64_t *out) {
  if (!c || !la || (!lb && !acc0) || !out || n == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_blind_rotate_level1: bad argument");
  if (acc0 && !canonical_words(acc0, n * 2 * N1, (uint64_t)Lvl1Int::Q))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_blind_rotate_level1_from: acc0 holds a word >= q1");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint16_t> da, db;
  DevBuf<uint64_t> dout, dacc;
  HIP_TRY(da.alloc(n * N0));
  HIP_TRY(db.alloc(n));
  HIP_TRY(dout.alloc(n * 2 * N1));
  HIP_TRY(hipMemcpy(da, la, n * N0 * sizeof(uint16_t), hipMemcpyHostToDevice));
  if (acc0) {  // the LWE bodies are unused: zeros
    HIP_TRY(hipMemset(db, 0, n * sizeof(uint16_t)));
    HIP_TRY(dacc.alloc(n * 2 * N1));
    HIP_TRY(hipMemcpy(dacc, acc0, n * 2 * N1 * sizeof(uint64_t), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(db, lb, n * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  // a pending hand-off error belongs to an earlier detect call: report it before this launch (as
  // detect_device does) instead of discarding a valid level-1 output after it
  OMR_TRY(take_handoff_error(c));
  // the guarded sequence (guard_begin, guard kernel, br1n_fallback, guard_fold) uses the context's
  // per-launch margin word, shared with every other call: serialise it with them like any scratch
  ScratchLease lease;
  OMR_TRY(lease.acquire(c, c->stream));
  OMR_TRY(launch_br1(c, n, nullptr, nullptr, da, db, nullptr, dout, 1, c->stream, n, acc0 ? dacc.get() : nullptr));
  OMR_TRY(lease.release());
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, dout, n * 2 * N1 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_blind_rotate_level1(omr_ctx *c, const uint16_t *la, const uint16_t *lb,
                                              size_t n, uint64_t *out) {
  if (!lb) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_blind_rotate_level1: bad argument");
  return blind_rotate_level1_impl(c, la, lb, n, nullptr, out);
}
extern "C" omr_status omr_blind_rotate_level1_from(omr_ctx *c, const uint16_t *la, const uint16_t *lb,
                                                   size_t n, const uint64_t *acc0, uint64_t *out) {
  return blind_rotate_level1_impl(c, la, lb, n, acc0, out);
}

static omr_status second_level_impl(omr_ctx *c, const uint32_t *lwe, size_t n, uint64_t *out,
                                    int mode, const uint64_t *acc0 = nullptr) {
  if (!c || !lwe || !out || n == 0)
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_second_level: bad argument");
  if (acc0 && !canonical_words(acc0, n * 2 * N2, (uint64_t)Mod<2>::Q))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_blind_rotate_level2_from: acc0 holds a word >= q2");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint32_t> dl;
  DevBuf<uint64_t> dout, dacc;
  HIP_TRY(dl.alloc(n * (NI + 1)));
  HIP_TRY(dout.alloc(n * 2 * N2));
  HIP_TRY(hipMemcpy(dl, lwe, n * (NI + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (acc0) {
    HIP_TRY(dacc.alloc(n * 2 * N2));
    HIP_TRY(hipMemcpy(dacc, acc0, n * 2 * N2 * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
  OMR_TRY(take_handoff_error(c));
  ScratchLease lease;  // the hand-off slots are scratch
  OMR_TRY(lease.acquire(c, c->stream));
  OMR_TRY(launch_br2(c, n, dl, dout, mode, c->stream, nullptr, acc0 ? dacc.get() : nullptr));
  OMR_TRY(lease.release());
  HIP_TRY(hipStreamSynchronize(c->stream));
  OMR_TRY(take_handoff_error(c));
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
extern "C" omr_status omr_blind_rotate_level2_from(omr_ctx *c, const uint32_t *lwe, size_t n,
                                                   const uint64_t *acc0, uint64_t *out) {
  return second_level_impl(c, lwe, n, out, 1, acc0);
}

extern "C" omr_status omr_trace(omr_ctx *c, const uint64_t *rlwe, size_t n, uint64_t *out) {
  if (!c || !rlwe || !out || n == 0) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_trace: bad argument");
  if (!canonical_words(rlwe, n * 2 * N2, (uint64_t)Mod<2>::Q))
    return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_trace: rlwe holds a word >= q2");
  std::lock_guard<std::mutex> lk(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<uint64_t> dio, dsaved;
  HIP_TRY(dio.alloc(n * 2 * N2));
  HIP_TRY(dsaved.alloc(n * 2 * N2));
  HIP_TRY(hipMemcpy(dio, rlwe, n * 2 * N2 * sizeof(uint64_t), hipMemcpyHostToDevice));
  OMR_TRY(take_handoff_error(c));
  ScratchLease lease;  // the hand-off slots are scratch
  OMR_TRY(lease.acquire(c, c->stream));
  OMR_TRY(launch_trace_only(c, n, dio, dsaved, c->stream));
  OMR_TRY(lease.release());
  HIP_TRY(hipStreamSynchronize(c->stream));
  OMR_TRY(take_handoff_error(c));
  HIP_TRY(hipMemcpy(out, dio, n * 2 * N2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return OMR_OK;
}

extern "C" omr_status omr_ctx_launch_record(omr_ctx *c, uint64_t counts[OMR_LAUNCH_COUNT]) {
  if (!c || !counts) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_launch_record: NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  std::copy(c->launches, c->launches + OMR_LAUNCH_COUNT, counts);
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
