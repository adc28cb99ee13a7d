// Stand-alone host test of the reference payload weights by seek (csrc/weights.hip: omr_weight_seek_build_cpu,
// its zone stage entry and omr_payload_weights_at), meant for a build with csrc/weights.hip and csrc/keygen.hip
// under the address and undefined-behaviour sanitizers (make build/seek_weights_test; no GPU is touched). The overflow and
// boundary cases of tests/test_seek_weights_host.py (seed 23, zone 0xE0000000) and denser zones, in exactly
// sized heap buffers (an access one word past an omr_weight_seek, an index list or a matrix is an error
// under the sanitizer), checked against the sequential draw restated here over common.hpp's chacha_block.
// omr_indexed_weights_at, which shares omr_payload_weights_at's row loop, against omr_indexed_weights_table.
// Also the edges of common.hpp's range_on_board, the payload encode entries' range check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "omr_gpu.h"

namespace {

int fails = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

void seed_of(uint64_t lo, uint8_t seed[32]) {
  std::memset(seed, 0, 32);
  for (int i = 0; i < 8; ++i) seed[i] = (uint8_t)(lo >> (8 * i));
}

// The first `count` accepted values drawn one after the other, and the at[] entries met on the way.
void sequential(const uint8_t seed[32], uint32_t zone, size_t count, std::vector<uint16_t> &out, std::vector<uint64_t> &at) {
  uint32_t key[8], buf[16];
  for (int i = 0; i < 8; ++i) std::memcpy(&key[i], seed + 4 * i, 4);  // little-endian host
  out.clear();
  at.clear();
  for (uint64_t r = 0; out.size() < count; ++r) {
    if ((r & 15) == 0) omr::chacha_block(12, key, r >> 4, 0, buf);
    const uint64_t m = (uint64_t)buf[r & 15] * 257u;
    if ((uint32_t)m > zone) at.push_back(r - at.size());
    else out.push_back((uint16_t)(m >> 32));
  }
}

// One (seed, zone, draws) case: the builder with 1 and 5 threads into an exactly sized heap struct, then
// the whole stream through omr_payload_weights_at as a one-row board and as a board of `rows` rows.
void check(uint64_t lo, uint32_t zone, uint64_t draws, const char *name) {
  uint8_t seed[32];
  seed_of(lo, seed);
  std::vector<uint16_t> seq;
  std::vector<uint64_t> at;
  sequential(seed, zone, (size_t)draws, seq, at);
  // the draw stops at its last accepted word: every rejection it met matters (at[k] < draws), no other does
  const bool over = at.size() > OMR_WEIGHT_SEEK_MAX;
  for (int nthreads : {1, 5}) {
    omr_weight_seek *sk = (omr_weight_seek *)std::malloc(sizeof(omr_weight_seek));
    std::memset(sk, 0xAB, sizeof *sk);
    const omr_status st = omr_weight_seek_build_zone_cpu(seed, draws, zone, nthreads, sk);
    if (over) {
      EXPECT(st == OMR_ERR_INVALID_ARGUMENT);
      EXPECT(std::strstr(omr_last_error(), "more than 32 rejections: use the table") != nullptr);
      bool untouched = true;
      for (size_t i = 0; i < sizeof *sk; ++i) untouched = untouched && ((const uint8_t *)sk)[i] == 0xAB;
      EXPECT(untouched);
    } else {
      EXPECT(st == OMR_OK);
      EXPECT(sk->draws == draws && sk->zone == zone && sk->n == at.size());
      for (size_t k = 0; k < at.size() && k < sk->n; ++k) EXPECT(sk->at[k] == at[k]);
      for (uint32_t rows : {1u, 3u}) {
        if (draws == 0 || draws % rows) continue;
        const size_t all = (size_t)(draws / rows);
        size_t *idx = (size_t *)std::malloc(all * sizeof(size_t));
        uint16_t *m = (uint16_t *)std::malloc((size_t)(rows + 1) * all * sizeof(uint16_t));
        for (size_t i = 0; i < all; ++i) idx[i] = all - 1 - i;  // descending: every block change is taken
        EXPECT(omr_payload_weights_at(seed, all, rows, sk, 0, rows + 1, idx, all, m, nthreads) == OMR_OK);
        bool same = true;
        for (size_t j = 0; j < rows; ++j)
          for (size_t i = 0; i < all; ++i) same = same && m[j * all + i] == seq[j * all + (all - 1 - i)];
        for (size_t i = 0; i < all; ++i) same = same && m[(size_t)rows * all + i] == 0;  // the padding row
        EXPECT(same);
        // one draw more than the seek covers
        EXPECT(omr_payload_weights_at(seed, all + 1, rows, sk, 0, rows, idx, all, m, nthreads) == OMR_ERR_INVALID_ARGUMENT);
        std::free(idx);
        std::free(m);
      }
    }
    if (fails) std::fprintf(stderr, "  in case %s (draws %llu, nthreads %d)\n", name, (unsigned long long)draws, nthreads);
    std::free(sk);
  }
}

// omr_indexed_weights_at on unsorted indices that come back to a block they left, with one padding
// combination, into an exactly sized matrix: the gather from omr_indexed_weights_table's rows.
void check_indexed() {
  uint8_t seed[32];
  seed_of(77, seed);
  const size_t all = 40;
  const uint32_t combos = 3, rows = 4;  // two ciphertexts of two combinations: row 3 is padding
  const size_t list[] = {33, 2, 17, 35, 0, 39, 16, 2};  // blocks 2, 0, 1, 2, 0, 2, 1, 0
  const size_t n = sizeof list / sizeof list[0];
  uint16_t *table = (uint16_t *)std::malloc(rows * all * sizeof(uint16_t));
  size_t *idx = (size_t *)std::malloc(sizeof list);
  std::memcpy(idx, list, sizeof list);
  EXPECT(omr_indexed_weights_table(seed, all, combos, 2, 2, table, 1) == OMR_OK);
  for (int nthreads : {1, 3}) {
    uint16_t *m = (uint16_t *)std::malloc(rows * n * sizeof(uint16_t));
    std::memset(m, 0xAB, rows * n * sizeof(uint16_t));
    EXPECT(omr_indexed_weights_at(seed, combos, 0, rows, idx, n, m, nthreads) == OMR_OK);
    bool same = true, live = false;
    for (size_t j = 0; j < rows; ++j)
      for (size_t k = 0; k < n; ++k) {
        same = same && m[j * n + k] == table[j * all + idx[k]];
        live = live || m[j * n + k] != 0;
      }
    for (size_t k = 0; k < n; ++k) same = same && m[(size_t)combos * n + k] == 0;  // the padding row
    EXPECT(same && live);
    // a window that starts at the last real combination
    EXPECT(omr_indexed_weights_at(seed, combos, 2, 2, idx, n, m, nthreads) == OMR_OK);
    for (size_t j = 0; j < 2; ++j)
      for (size_t k = 0; k < n; ++k) same = same && m[j * n + k] == table[(2 + j) * all + idx[k]];
    EXPECT(same);
    std::free(m);
  }
  std::free(idx);
  std::free(table);
}

}  // namespace

int main() {
  const uint32_t Z = 0xE0000000u;
  check_indexed();
  for (uint64_t d : {0, 1, 2, 9, 10, 11, 84, 85, 86, 184, 185, 186, 213}) check(23, Z, d, "seed 23 edges");
  for (uint64_t d : {214, 215, 216}) check(23, Z, d, "exactly 32");
  for (uint64_t d : {217, 226, 227, 300, 4096, 70000}) check(23, Z, d, "overflow");
  // denser streams: half the words, and every word, rejected
  for (uint64_t d : {0, 1, 5, 30, 40, 100}) check(7, 0x80000000u, d, "half rejected");
  {
    uint8_t seed[32];
    seed_of(7, seed);
    omr_weight_seek sk;
    std::memset(&sk, 0xCD, sizeof sk);
    EXPECT(omr_weight_seek_build_zone_cpu(seed, 0, 0, 1, &sk) == OMR_OK && sk.n == 0 && sk.draws == 0);
    std::memset(&sk, 0xCD, sizeof sk);
    EXPECT(omr_weight_seek_build_zone_cpu(seed, 1, 0, 3, &sk) == OMR_ERR_INVALID_ARGUMENT);  // (almost) every word rejected
    EXPECT(*(const uint8_t *)&sk == 0xCD);
  }
  // the reference's zone: the seeds whose streams reject early, around the rejection and across a piece edge
  for (uint64_t d : {5713, 5714, 5715, 5716, 70000}) check(259680, OMR_WEIGHT_ZONE, d, "seed 259680");
  for (uint64_t d : {14655, 14656, 14657}) check(10448, OMR_WEIGHT_ZONE, d, "seed 10448");
  // argument errors
  uint8_t seed[32];
  seed_of(1, seed);
  omr_weight_seek sk{};
  size_t i0 = 0;
  uint16_t w = 0;
  EXPECT(omr_weight_seek_build_cpu(nullptr, 1, 1, &sk) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_weight_seek_build_cpu(seed, 1, 1, nullptr) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_weight_seek_build_cpu(seed, 1ull << 62, 1, &sk) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_weight_seek_build_cpu(seed, 8, 1, &sk) == OMR_OK && sk.n == 0 && sk.zone == OMR_WEIGHT_ZONE);
  EXPECT(omr_payload_weights_at(seed, 4, 2, &sk, 0, 1, &i0, 1, &w, 1) == OMR_OK);
  EXPECT(omr_payload_weights_at(seed, 4, 3, &sk, 0, 1, &i0, 1, &w, 1) == OMR_ERR_INVALID_ARGUMENT);  // 12 > 8 draws
  EXPECT(omr_payload_weights_at(seed, 4, 2, nullptr, 0, 1, &i0, 1, &w, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_payload_weights_at(nullptr, 4, 2, &sk, 0, 1, &i0, 1, &w, 1) == OMR_ERR_INVALID_ARGUMENT);
  i0 = 4;
  EXPECT(omr_payload_weights_at(seed, 4, 2, &sk, 0, 1, &i0, 1, &w, 1) == OMR_ERR_INVALID_ARGUMENT);  // index = all
  i0 = 0;
  sk.n = OMR_WEIGHT_SEEK_MAX + 1;
  EXPECT(omr_payload_weights_at(seed, 4, 2, &sk, 0, 1, &i0, 1, &w, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_payload_weights_at(seed, (size_t)1 << 63, 4, &sk, 0, 1, &i0, 1, &w, 1) == OMR_ERR_INVALID_ARGUMENT);
  // the payload encode entries' range check (common.hpp, range_on_board): offset + D wraps, an empty range at
  // the board's end, and the last message on the board and one beyond it
  EXPECT(!omr::range_on_board(SIZE_MAX, 2, 100));
  EXPECT(!omr::range_on_board(SIZE_MAX, 2, SIZE_MAX));
  EXPECT(omr::range_on_board(100, 0, 100) && !omr::range_on_board(101, 0, 100));
  EXPECT(omr::range_on_board(40, 60, 100) && !omr::range_on_board(40, 61, 100));
  EXPECT(omr::range_on_board(0, SIZE_MAX, SIZE_MAX) && omr::range_on_board(0, 0, 0) && !omr::range_on_board(0, 1, 0));
  if (fails) {
    std::printf("seek weights host test FAILED (%d)\n", fails);
    return 1;
  }
  std::printf("seek weights host test OK\n");
  return 0;
}
