// Stand-alone host test of the mod-257 solve's CPU statement (csrc/retriever.hip: omr_solve_mod257_cpu), meant
// for a build with csrc/weights.hip and csrc/keygen.hip under the address and undefined-behaviour sanitizers
// (make build/solve_test; no GPU is touched): the crafted systems of tests/solve_cases.py restated here in exactly sized heap buffers
// (an access one word past a row or a buffer is an error under the sanitizer), checked against a plain
// restatement of the definition, the threaded row updates, the singular reports and the argument errors.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

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

constexpr uint32_t P = OMR_P;

struct System {
  size_t rows, cols, width;
  std::vector<uint16_t> m, r;
  System(size_t rows_, size_t cols_, size_t width_) : rows(rows_), cols(cols_), width(width_), m(rows_ * cols_), r(rows_ * width_) {}
  uint16_t &at(size_t j, size_t k) { return m[j * cols + k]; }
};

uint64_t lcg = 257;
uint32_t rnd(uint32_t n) {  // a small fixed stream
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((lcg >> 33) % n);
}
void fill_random(System &s, uint32_t lo, uint32_t hi) {
  for (auto &x : s.m) x = (uint16_t)(lo + rnd(hi - lo));
  for (auto &x : s.r) x = (uint16_t)(lo + rnd(hi - lo));
}

uint32_t inv(uint32_t v) {
  uint32_t r = 1;
  for (int e = 0; e < 255; ++e) r = r * v % P;
  return r;
}

// The definition, row lists and whole-row operations: -1 = solved, else the column without a pivot.
long reference(const System &s, std::vector<uint16_t> &out) {
  const size_t ld = s.cols + s.width;
  std::vector<std::vector<uint32_t>> w(s.rows, std::vector<uint32_t>(ld));
  for (size_t j = 0; j < s.rows; ++j) {
    for (size_t k = 0; k < s.cols; ++k) w[j][k] = s.m[j * s.cols + k] % P;
    for (size_t b = 0; b < s.width; ++b) w[j][s.cols + b] = s.r[j * s.width + b] % P;
  }
  for (size_t i = 0; i < s.cols; ++i) {
    size_t piv = i;
    while (piv < s.rows && w[piv][i] == 0) ++piv;
    if (piv == s.rows) return (long)i;
    std::swap(w[i], w[piv]);
    const uint32_t iv = inv(w[i][i]);
    for (auto &x : w[i]) x = x * iv % P;
    for (size_t j = 0; j < s.rows; ++j) {  // Gauss-Jordan: above and below
      const uint32_t c = w[j][i];
      if (j == i || !c) continue;
      for (size_t k = 0; k < ld; ++k) w[j][k] = (w[j][k] + P * P - c * w[i][k]) % P;
    }
  }
  out.assign(s.cols * s.width, 0);
  for (size_t k = 0; k < s.cols; ++k)
    for (size_t b = 0; b < s.width; ++b) out[k * s.width + b] = (uint16_t)w[k][s.cols + b];
  return -1;
}

void check(const System &s, long want_singular, const char *name) {
  std::vector<uint16_t> ref;
  const long rs = reference(s, ref);
  EXPECT(rs == want_singular);
  for (int nthreads : {1, 3}) {
    // exactly sized heap copies: the sanitizer sees any access past them
    uint16_t *m = (uint16_t *)std::malloc(s.m.size() * 2), *r = (uint16_t *)std::malloc(s.r.size() * 2);
    uint16_t *out = (uint16_t *)std::malloc(s.cols * s.width * 2);
    std::memcpy(m, s.m.data(), s.m.size() * 2);
    std::memcpy(r, s.r.data(), s.r.size() * 2);
    std::memset(out, 0xAB, s.cols * s.width * 2);
    size_t col = 99999;
    const omr_status st = omr_solve_mod257_cpu(m, r, s.rows, s.cols, s.width, out, &col, nthreads);
    if (want_singular < 0) {
      EXPECT(st == OMR_OK);
      EXPECT(std::memcmp(out, ref.data(), ref.size() * 2) == 0);
    } else {
      EXPECT(st == OMR_ERR_NOT_INVERTIBLE);
      EXPECT(col == (size_t)want_singular);
      EXPECT(std::strcmp(omr_last_error(), "Matrix is not invertible") == 0);
      bool untouched = true;
      for (size_t i = 0; i < s.cols * s.width; ++i) untouched = untouched && out[i] == 0xABAB;
      EXPECT(untouched);
    }
    EXPECT(std::memcmp(m, s.m.data(), s.m.size() * 2) == 0 && std::memcmp(r, s.r.data(), s.r.size() * 2) == 0);
    if (fails) std::fprintf(stderr, "  in case %s (nthreads %d)\n", name, nthreads);
    std::free(m);
    std::free(r);
    std::free(out);
  }
}

}  // namespace

// argv[1]: the device solver's panel width (omr_solve_geometry, which is not linked here), so that the
// panel-edge systems sit where tests/solve_cases.py puts them. The CPU statement has no tiling of its own.
int main(int argc, char **argv) {
  const unsigned pc = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 0;
  if (pc < 2 || pc > 1024) {
    std::fprintf(stderr, "usage: %s PANEL_COLS (2 .. 1024)\n", argv[0]);
    return 2;
  }
  {
    System s(5, 5, 3);
    fill_random(s, 0, P);
    for (size_t j = 0; j < 5; ++j)
      for (size_t k = 0; k < 5; ++k) s.at(j, k) = j == k;
    check(s, -1, "identity");
  }
  {
    const size_t n = pc + 5;
    System s(n, n, 4);
    fill_random(s, 0, P);
    std::fill(s.m.begin(), s.m.end(), 0);
    for (size_t j = 0; j < n; ++j) s.at(j, (j + 1) % n) = 1;
    check(s, -1, "permutation");
  }
  for (size_t cols : {(size_t)5, (size_t)pc + 2}) {
    System s(cols + 5, cols, 6);
    fill_random(s, 0, P);
    std::fill(s.m.begin(), s.m.end(), 0);
    for (size_t i = 0; i < cols; ++i) {
      s.at(i + 5, i) = (uint16_t)(1 + rnd(P - 1));
      for (size_t k = i + 1; k < cols; ++k) s.at(i + 5, k) = (uint16_t)rnd(P);
    }
    check(s, -1, "pivots in extra rows");
  }
  for (size_t rows : {(size_t)4, (size_t)9}) {
    System s(rows, 4, 2);
    fill_random(s, 0, P);
    std::fill(s.m.begin(), s.m.end(), 256);
    check(s, 1, "all 256");
  }
  {
    const size_t cols = pc + 6;
    for (size_t z : {(size_t)0, (size_t)pc - 1, (size_t)pc, cols - 1}) {
      System s(cols + 5, cols, 3);
      fill_random(s, 0, P);
      for (size_t j = 0; j < s.rows; ++j) s.at(j, z) = 0;
      check(s, (long)z, "zero column");
    }
    System s(cols + 5, cols, 3);
    fill_random(s, 0, P);
    for (size_t j = 0; j < s.rows; ++j) s.at(j, pc + 1) = s.at(j, pc - 2);
    check(s, (long)pc + 1, "duplicate column");
  }
  for (size_t cols : {(size_t)24, (size_t)70}) {
    System s(cols + 5, cols, 7);
    fill_random(s, 0, P);
    for (auto &x : s.m)
      if (rnd(10) >= 3) x = 0;
    std::vector<uint16_t> ref;
    check(s, reference(s, ref), "sparse inconsistent");
  }
  {
    System s(2 * pc + 6, 2 * pc + 1, 9);
    fill_random(s, 255, 257);
    std::vector<uint16_t> ref;
    check(s, reference(s, ref), "dense 255 / 256");
  }
  {
    System s(pc + 9, pc + 4, 5);
    fill_random(s, 0, 65536);
    s.at(0, 0) = 257, s.at(1, 1) = 514, s.at(2, 2) = 65535, s.r[0] = 65535;
    std::vector<uint16_t> ref;
    check(s, reference(s, ref), "words above 256");
  }
  for (size_t width : {(size_t)1, (size_t)612, (size_t)613}) {
    System s(15, 10, width);
    fill_random(s, 0, P);
    std::vector<uint16_t> ref;
    check(s, reference(s, ref), "widths");
  }
  {  // large enough for the threaded row updates to engage
    System s(700, 60, 612);
    fill_random(s, 0, P);
    std::vector<uint16_t> ref;
    check(s, reference(s, ref), "threaded");
  }
  // argument errors
  uint16_t one = 1, out = 0;
  EXPECT(omr_solve_mod257_cpu(nullptr, &one, 1, 1, 1, &out, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_solve_mod257_cpu(&one, nullptr, 1, 1, 1, &out, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_solve_mod257_cpu(&one, &one, 1, 1, 1, nullptr, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_solve_mod257_cpu(&one, &one, 1, 0, 1, &out, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_solve_mod257_cpu(&one, &one, 1, 2, 1, &out, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_solve_mod257_cpu(&one, &one, 1, 1, 0, &out, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_solve_mod257_cpu(&one, &one, OMR_SOLVE_MAX_ROWS + 1, 1, 1, &out, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_solve_mod257_cpu(&one, &one, 1, 1, 1, &out, nullptr, 1) == OMR_OK && out == 1);
  if (fails) {
    std::printf("solve host test FAILED (%d)\n", fails);
    return 1;
  }
  std::printf("solve host test OK\n");
  return 0;
}
