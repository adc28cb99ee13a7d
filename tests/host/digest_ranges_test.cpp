// Stand-alone test of csrc/digest_ranges.hpp (the interval set of a digest session's folded-in
// message ranges). Exit 0 when every check holds; prints the first failing check otherwise.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "digest_ranges.hpp"

using omr::DigestRanges;

static int fails = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

static void insert_overlap_adjacency() {
  DigestRanges r(300);
  EXPECT(r.covered() == 0 && r.intervals() == 0);
  EXPECT(r.insert(10, 10));  // [10, 20)
  EXPECT(r.covered() == 10 && r.intervals() == 1);
  EXPECT(!r.insert(19, 6));   // overlaps the last message
  EXPECT(!r.insert(5, 6));    // overlaps the first
  EXPECT(!r.insert(12, 3));   // inside
  EXPECT(!r.insert(0, 300));  // around
  EXPECT(!r.insert(10, 10));  // the same range again
  EXPECT(r.covered() == 10 && r.intervals() == 1);  // rejected inserts change nothing
  EXPECT(r.insert(20, 5));                          // adjacent above: accepted and merged
  EXPECT(r.insert(5, 5));                           // adjacent below
  EXPECT(r.covered() == 20 && r.intervals() == 1);
  EXPECT(r.contains(5) && r.contains(24) && !r.contains(4) && !r.contains(25));
  EXPECT(!r.insert(295, 6));  // reaches beyond all
  EXPECT(r.insert(295, 5));
  EXPECT(!r.insert(300, 1));
  EXPECT(r.insert(300, 0) && r.insert(12, 0));  // D = 0 is a no-op anywhere up to all
  EXPECT(!r.insert(301, 0));
  EXPECT(r.covered() == 25 && r.intervals() == 2);
}

static void merging_and_order() {
  DigestRanges r(300);
  EXPECT(r.insert(260, 40));
  EXPECT(r.insert(0, 1));
  EXPECT(r.insert(38, 222));  // touches [260, 300)
  EXPECT(r.intervals() == 2 && r.covered() == 263);
  EXPECT(r.insert(1, 37));  // closes the gap: one interval
  EXPECT(r.intervals() == 1 && r.covered() == 300);
  EXPECT(!r.insert(0, 1) && !r.insert(299, 1) && r.insert(300, 0));
  // three intervals joined by the middle one
  DigestRanges s(100);
  EXPECT(s.insert(0, 10) && s.insert(20, 10) && s.intervals() == 2);
  EXPECT(s.insert(10, 10) && s.intervals() == 1 && s.covered() == 30);
}

static void overflow() {
  const size_t big = SIZE_MAX;
  DigestRanges r(300);
  EXPECT(!r.insert(10, big));      // offset + D wraps to 9
  EXPECT(!r.insert(big, 2));       // wraps to 1
  EXPECT(!r.insert(big - 1, 1));
  EXPECT(!r.insert(1, big));       // wraps to 0
  EXPECT(r.covered() == 0 && r.intervals() == 0);
  DigestRanges w(big);
  EXPECT(w.insert(big - 4, 4) && !w.insert(big - 4, 5) && !w.insert(big - 1, 2));
  EXPECT(w.insert(0, big - 4) && w.intervals() == 1 && w.covered() == big);
}

// Random inserts against a bitmap model, all <= 512.
static void randomised() {
  std::mt19937_64 rng(20250);
  for (int round = 0; round < 200; ++round) {
    const size_t all = 1 + rng() % 512;
    DigestRanges r(all);
    std::vector<char> bits(all, 0);
    size_t covered = 0;
    for (int k = 0; k < 300; ++k) {
      const size_t off = rng() % (all + 3), D = rng() % (k % 3 ? 9 : all + 3);
      bool ok = off <= all && D <= all - off;
      for (size_t i = off; ok && i < off + D; ++i) ok = !bits[i];
      EXPECT(r.can_insert(off, D) == ok);
      EXPECT(r.insert(off, D) == ok);
      if (ok) {
        for (size_t i = off; i < off + D; ++i) bits[i] = 1;
        covered += D;
      }
      EXPECT(r.covered() == covered);
    }
    size_t runs = 0;
    for (size_t i = 0; i < all; ++i) {
      EXPECT(r.contains(i) == (bits[i] != 0));
      if (bits[i] && (i == 0 || !bits[i - 1])) ++runs;
    }
    EXPECT(r.intervals() == runs);  // touching ranges are merged
    if (fails) return;
  }
}

int main() {
  insert_overlap_adjacency();
  merging_and_order();
  overflow();
  randomised();
  if (fails) {
    std::printf("digest_ranges_test: %d checks failed\n", fails);
    return 1;
  }
  std::printf("digest_ranges_test: ok\n");
  return 0;
}
