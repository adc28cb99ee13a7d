// The sender handle (include/omr_gpu.h "Sender"): a table of public clue keys, and on a device its
// copy, the clue Gaussian's table and the error word, uploaded once by omr_sender_create (keygen.hip).
// omr_sender_gen_clues (keygen.hip) reads the host table; omr_sender_gen_clues_device (keygen_gpu.hip)
// the device one.
#pragma once

#include <mutex>
#include <vector>

#include "hip_util.hpp"

struct omr_sender {
  std::vector<uint16_t> keys;  // [n_keys][2][512]: a then b of each key, words < 2048
  size_t n_keys = 0;
  int device = -1;             // < 0: CPU only
  std::mutex mu;               // serialises the device calls (they share the error word)
  omr::DevBuf<uint16_t> d_keys;
  omr::DevBuf<uint64_t> d_cdt;
  int cdt_n = 0;
  omr::DevBuf<unsigned long long> d_err;  // smallest message index with an id out of range; ~0 = none
};

namespace omr {
constexpr unsigned long long SENDER_NO_ERROR = ~0ull;
}
