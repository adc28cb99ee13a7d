// Stand-alone host test of the sender's CPU entries (include/omr_gpu.h "Sender"; csrc/keygen.hip), built
// under the address and undefined-behaviour sanitizers: every entry on exactly sized heap buffers, so that a
// read or write one element past any of them is reported, with count 0 and 1, n_keys 1, and a small mixed
// board. Host code only; no GPU is touched (the senders are created with device < 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "omr_gpu.h"

namespace {

constexpr size_t N0 = 512, CLUES = 7;
int fails = 0;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++fails;                                                           \
    }                                                                    \
  } while (0)
#define OK(expr) EXPECT((expr) == OMR_OK)

// exactly sized heap arrays (operator new[]: the sanitizer's redzones sit right behind the last element)
template <typename T>
std::unique_ptr<T[]> exact(size_t n) {
  return std::unique_ptr<T[]>(new T[n]());
}

}  // namespace

int main() {
  omr_secret_key_pack *pa = nullptr, *pb = nullptr;
  OK(omr_keygen_secret(42, &pa));
  OK(omr_keygen_secret(4242, &pb));

  // the clue key as a value, its checks
  auto keys = exact<omr_clue_key>(2);
  OK(omr_secret_clue_key(pa, &keys[0]));
  OK(omr_secret_clue_key(pb, &keys[1]));
  uint64_t K = 0, noncanon = 1, mx = 0;
  uint32_t over = 1, nc = 1;
  OK(omr_clue_key_noise_support(&K));
  EXPECT(K >= 1 && K < 64);
  OK(omr_clue_key_validate(keys.get(), 2, &noncanon));
  EXPECT(noncanon == 0);
  OK(omr_clue_key_validate(nullptr, 0, &noncanon));
  OK(omr_clue_key_audit(pa, &keys[0], UINT64_MAX, &mx, &over, &nc));
  EXPECT(mx <= K && over == 0 && nc == 0);
  OK(omr_clue_key_audit(pa, &keys[1], UINT64_MAX, &mx, &over, nullptr));
  EXPECT(over > 0);
  OK(omr_clue_key_audit(pa, &keys[0], 0, nullptr, nullptr, nullptr));

  // n_keys 1: count 0 (no buffer at all) and count 1, equal to omr_gen_clues
  omr_sender *one = nullptr, *two = nullptr;
  OK(omr_sender_create(&keys[0], 1, -1, &one));
  OK(omr_sender_gen_clues(one, nullptr, 9, 0, 0, nullptr, nullptr, 1));
  {
    auto a = exact<uint16_t>(N0), b = exact<uint16_t>(CLUES), ea = exact<uint16_t>(N0), eb = exact<uint16_t>(CLUES);
    auto rec = exact<uint32_t>(1);
    OK(omr_sender_gen_clues(one, rec.get(), 9, (1ull << 40) + 3, 1, a.get(), b.get(), 1));
    OK(omr_gen_clues(pa, 9, (1ull << 40) + 3, 1, ea.get(), eb.get(), 1));
    EXPECT(!std::memcmp(a.get(), ea.get(), N0 * 2) && !std::memcmp(b.get(), eb.get(), CLUES * 2));
    rec[0] = 1;  // = n_keys: rejected, nothing written
    std::memset(a.get(), 0x5a, N0 * 2);
    EXPECT(omr_sender_gen_clues(one, rec.get(), 9, 0, 1, a.get(), b.get(), 1) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(a[0] == 0x5a5a && a[N0 - 1] == 0x5a5a);
    // opening one message, each output alone
    auto v = exact<uint8_t>(CLUES), p = exact<uint8_t>(1), n = exact<uint8_t>(1);
    OK(omr_clue_open(pa, ea.get(), eb.get(), 1, v.get(), nullptr, nullptr, 1));
    OK(omr_clue_open(pa, ea.get(), eb.get(), 1, nullptr, p.get(), nullptr, 1));
    OK(omr_clue_open(pa, ea.get(), eb.get(), 1, nullptr, nullptr, n.get(), 1));
    EXPECT(p[0] == 1 && n[0] <= 128);
    for (size_t i = 0; i < CLUES; ++i) EXPECT(v[i] == 0);
    OK(omr_clue_open(pa, nullptr, nullptr, 0, v.get(), p.get(), n.get(), 1));
    EXPECT(omr_clue_open(pa, ea.get(), eb.get(), 1, nullptr, nullptr, nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  }

  // a mixed board over two keys, several threads: each recipient opens its own
  OK(omr_sender_create(keys.get(), 2, -1, &two));
  {
    constexpr size_t D = 67;
    auto a = exact<uint16_t>(D * N0), b = exact<uint16_t>(D * CLUES);
    auto rec = exact<uint32_t>(D);
    auto pert = exact<uint8_t>(D);
    for (size_t m = 0; m < D; ++m) rec[m] = (uint32_t)((m * 7 + 3) % 5 < 2);
    OK(omr_sender_gen_clues(two, rec.get(), 11, 5, D, a.get(), b.get(), 5));
    OK(omr_clue_open(pb, a.get(), b.get(), D, nullptr, pert.get(), nullptr, 3));
    for (size_t m = 0; m < D; ++m) EXPECT(pert[m] == rec[m]);
    // words with high bits are reduced, not read as larger numbers
    for (size_t i = 0; i < D * N0; ++i) a[i] |= 0xF800;
    auto pert2 = exact<uint8_t>(D);
    OK(omr_clue_open(pb, a.get(), b.get(), D, nullptr, pert2.get(), nullptr, 0));
    EXPECT(!std::memcmp(pert.get(), pert2.get(), D));
  }

  // creation errors
  omr_sender *bad = nullptr;
  EXPECT(omr_sender_create(keys.get(), 0, -1, &bad) == OMR_ERR_INVALID_ARGUMENT && !bad);
  keys[1].b[511] = 2048;
  EXPECT(omr_sender_create(keys.get(), 2, -1, &bad) == OMR_ERR_INVALID_ARGUMENT && !bad);
  EXPECT(std::strstr(omr_last_error(), "key 1") != nullptr);
  OK(omr_clue_key_validate(keys.get(), 2, &noncanon));
  EXPECT(noncanon == 1);

  omr_sender_destroy(one);
  omr_sender_destroy(two);
  omr_sender_destroy(nullptr);
  omr_secret_destroy(pa);
  omr_secret_destroy(pb);
  if (fails) {
    std::printf("sender host test FAILED (%d)\n", fails);
    return 1;
  }
  std::printf("sender host test OK\n");
  return 0;
}
