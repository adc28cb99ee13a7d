// Stand-alone host test of the seeded detection key (include/omr_gpu.h), meant for a build of csrc/keygen.hip
// under the address and undefined-behaviour sanitizers (make build/seeded_key_test; no GPU is touched):
// host keygen, host expansion and omr_key_masks on small row ranges at the start and the end of every
// component, the argument errors, and expanded rows = (omr_key_masks, body).
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Comp {
  int id;
  size_t rows, masks, row_elems, width;
};
const Comp COMPS[4] = {{OMR_KEY_BSK1, 4096, 1024, 2048, 4},
                       {OMR_KEY_KSK, 27648, 670, 671, 4},
                       {OMR_KEY_BSK2, 8040, 2048, 4096, 8},
                       {OMR_KEY_TRACE, 275, 2048, 4096, 8}};

}  // namespace

int main() {
  const uint64_t mask_seed = 2026;
  omr_secret_key_pack *sk = nullptr;
  EXPECT(omr_keygen_secret(42, &sk) == OMR_OK);
  // exactly sized buffers: an overrun of any of them is the sanitizer's to find
  std::vector<uint32_t> bsk1_b(4096u * 1024), ksk_b(27648), bsk1(4096u * 2048), ksk(27648u * 671);
  std::vector<uint64_t> bsk2_b(8040u * 2048), tk_b(275u * 2048), bsk2(8040u * 4096), tk(275u * 4096);
  EXPECT(omr_keygen_seeded_key(sk, 7, mask_seed, bsk1_b.data(), ksk_b.data(), bsk2_b.data(), tk_b.data(), 4) == OMR_OK);
  const omr_seeded_key_view view{bsk1_b.data(), ksk_b.data(), bsk2_b.data(), tk_b.data(), mask_seed};
  EXPECT(omr_expand_detection_key(&view, bsk1.data(), ksk.data(), bsk2.data(), tk.data(), 3) == OMR_OK);

  const void *full[4] = {bsk1.data(), ksk.data(), bsk2.data(), tk.data()};
  const void *body[4] = {bsk1_b.data(), ksk_b.data(), bsk2_b.data(), tk_b.data()};
  for (const Comp &c : COMPS) {
    const size_t ranges[3][2] = {{0, 3}, {c.rows - 2, 2}, {c.rows, 0}};
    for (const auto &r : ranges) {
      std::vector<unsigned char> m(r[1] * c.masks * c.width);
      EXPECT(omr_key_masks(mask_seed, c.id, r[0], r[1], m.data()) == OMR_OK);
      for (size_t i = 0; i < r[1]; ++i) {
        const unsigned char *row = (const unsigned char *)full[c.id] + (r[0] + i) * c.row_elems * c.width;
        EXPECT(std::memcmp(row, m.data() + i * c.masks * c.width, c.masks * c.width) == 0);
        const size_t nb = (c.row_elems - c.masks) * c.width;
        EXPECT(std::memcmp(row + c.masks * c.width, (const unsigned char *)body[c.id] + (r[0] + i) * nb, nb) == 0);
      }
    }
    unsigned char one[2048 * 8];
    EXPECT(omr_key_masks(mask_seed, c.id, c.rows - 1, 2, one) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_key_masks(mask_seed, c.id, c.rows + 1, 0, one) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_key_masks(mask_seed, c.id, 1, (size_t)-1, one) == OMR_ERR_INVALID_ARGUMENT);
    EXPECT(omr_key_masks(mask_seed, c.id, 0, 1, nullptr) == OMR_ERR_INVALID_ARGUMENT);
  }
  EXPECT(omr_key_masks(mask_seed, 4, 0, 1, bsk1.data()) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_key_masks(mask_seed, -1, 0, 1, bsk1.data()) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_keygen_seeded_key(sk, 7, mask_seed, bsk1_b.data(), nullptr, bsk2_b.data(), tk_b.data(), 1) ==
         OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_expand_detection_key(nullptr, bsk1.data(), ksk.data(), bsk2.data(), tk.data(), 1) == OMR_ERR_INVALID_ARGUMENT);
  EXPECT(omr_expand_detection_key(&view, bsk1.data(), ksk.data(), bsk2.data(), nullptr, 1) == OMR_ERR_INVALID_ARGUMENT);
  omr_secret_destroy(sk);
  std::printf(fails ? "FAILED (%d)\n" : "seeded key host test OK\n", fails);
  return fails ? 1 : 0;
}
