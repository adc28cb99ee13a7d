// omr_detect's coalescer (host code only): concurrent single-message calls are combined into batched
// launches. It owns omr_ctx::Coalescer and takes the context mutex only around detect_host.
//
// Detector::detect (detector.rs:135-138) for one message, callable from many host threads at once
// (the reference's `clues.par_iter().map(|c| detector.detect(c))`, examples/omr.rs:160-164, on a
// shared &Detector): the requests queue on the context; whichever caller finds no launch in
// progress becomes the leader, optionally waits window_us for more, gathers up to max queued clues
// into one omr_detect_batch (latency kernels up to the threshold, throughput kernels above),
// scatters the outputs and wakes their callers; the next leader takes what queued meanwhile. Every
// caller gets its batch's status and error message.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>

#include "ctx.hpp"

using namespace omr;

extern "C" omr_status omr_detect(omr_ctx *c, const uint16_t *ca, const uint16_t *cb, uint64_t *out) {
  if (!c || !ca || !cb || !out) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_detect: NULL argument");
  omr_ctx::Coalescer &q = c->q;
  omr_ctx::Coalescer::Req r{ca, cb, out, OMR_OK, std::string(), false};
  std::unique_lock<std::mutex> lk(q.mu);
  q.queue.push_back(&r);
  q.cv.notify_all();  // a leader inside its window may be waiting for a full batch
  while (!r.done) {
    if (q.leader) {
      q.cv.wait(lk);
      continue;
    }
    q.leader = true;
    if (q.window_us > 0 && q.queue.size() < q.max)
      q.cv.wait_for(lk, std::chrono::microseconds(q.window_us), [&] { return q.queue.size() >= q.max; });
    const size_t n = std::min(q.queue.size(), q.max);
    std::vector<omr_ctx::Coalescer::Req *> batch(q.queue.begin(), q.queue.begin() + (long)n);
    q.queue.erase(q.queue.begin(), q.queue.begin() + (long)n);
    lk.unlock();
    // gather, launch, scatter: nothing may throw out of this extern "C" function, and the leader
    // flag must be cleared whatever happens (a staging allocation of up to max messages can fail):
    // a failure becomes the batch's status
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
        st = detect_host(c, ga.data(), gb.data(), n, go.data());
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
    for (auto *p : batch) {
      p->st = st;
      p->err = err;
      p->done = true;
    }
    q.calls += n;
    q.launches += 1;
    q.leader = false;
    q.cv.notify_all();
  }
  return r.st == OMR_OK ? OMR_OK : set_error(r.st, r.err);
}

extern "C" omr_status omr_ctx_set_coalescing(omr_ctx *c, size_t max_messages, long window_us) {
  if (!c || window_us < 0) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_set_coalescing: bad argument");
  std::lock_guard<std::mutex> lk(c->q.mu);
  c->q.max = max_messages ? max_messages : 65536;
  c->q.window_us = window_us;
  return OMR_OK;
}

extern "C" omr_status omr_ctx_coalescing_stats(omr_ctx *c, size_t *calls, size_t *launches) {
  if (!c) return set_error(OMR_ERR_INVALID_ARGUMENT, "omr_ctx_coalescing_stats: NULL ctx");
  std::lock_guard<std::mutex> lk(c->q.mu);
  if (calls) *calls = c->q.calls;
  if (launches) *launches = c->q.launches;
  return OMR_OK;
}
