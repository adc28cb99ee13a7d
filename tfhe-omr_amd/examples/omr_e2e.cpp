// omr_e2e — the reference's end-to-end example (omr_core/examples/omr.rs:30-235) driven through
// the C ABI of include/omr_gpu.h from native code: key generation, clue generation (pertinent
// messages from sender A, the rest from sender B), detect on the GPU, encode_pertinent_indices /
// encode_pertinent_payloads, client-side retrieval, and a check that exactly the pertinent
// indices and their payloads come back.
//
//   omr_e2e [-p payload_count] [-d device] [-s seed] [--session PIECE] [--audit] [--bitmap] [--seeded]
//           [--compact BITS] [--audit-key] [--indexed-weights] [--payload-len L] [--seek-weights] [--device-retrieve]
//           [--sender] [--host-only]
//
// --session PIECE runs the same board through a digest session (omr_digest_*) in host pieces of
// PIECE messages instead of omr_detect_batch plus the encoders: no pertinency vector on the host.
// --audit checks the detector's output on the GPU with the recipient's secret (omr_audit): every pertinent
// message's ciphertext must decrypt to [1, 0, .., 0], every other one to zeros (with --session there is
// no pertinency vector to audit), and the digests' decode residuals are reported.
// --bitmap takes the pertinent indices from the bitmap digest (omr_encode_bitmap, or the session's with
// omr_digest_enable_bitmap; omr_retrieve_bitmap), which needs no pertinent count, instead of the index
// digest; the payloads are then solved for those indices. With --host-only it checks the bitmap's layout
// on the host (omr_bitmap_ct_count, omr_bitmap_indices on the board's own pertinent set).
// --seeded generates the detection key in its seeded form (omr_keygen_seeded_key: the bodies and a public
// mask seed, 146 MiB instead of 363) and builds the detector through omr_ctx_create_seeded, which expands
// it on the device. With --host-only the key is expanded on the host (omr_expand_detection_key) and its
// masks are checked against omr_key_masks.
// --compact BITS sends the digest in compact form (include/omr_gpu.h, "Compact ciphertexts"): the detector
// compacts it on the GPU to BITS bits per coefficient (omr_compact_cts, or the session's
// omr_digest_read_compact), the recipient expands it (omr_compact_expand_cpu) and retrieves from that. Both
// sizes, R(BITS) for the recipient's key and the measured residual increase are printed; an increase above R
// or a decoded value that changed fails the run.
// --audit-key audits the detection key it generated against the recipient's secret on the GPU before the
// detector is created (omr_audit_key, or omr_audit_key_seeded with --seeded; include/omr_gpu.h, "Key audit"):
// a row whose noise lies outside the generators' support, in any component, fails the run.
// --device-retrieve makes the recipient retrieve on an auditor (include/omr_gpu.h, "Solve mod 257":
// omr_auditor_retrieve_indices, omr_auditor_retrieve_payloads[_indexed]): decode, right-hand side and the
// mod-257 solve run on the device. With --compact the auditor takes the packed digest as it arrived and
// expands it on the device; with --indexed-weights it builds the matrix there too.
// --indexed-weights uses indexed payload weights on both sides (include/omr_gpu.h, "Indexed payload weights"):
// the detector encodes with omr_encode_payloads_indexed (or a session from omr_digest_begin_indexed) and the
// recipient solves with omr_retrieve_payloads_indexed; nobody draws the board-wide weight table. With
// --host-only it checks omr_indexed_weights_at against omr_indexed_weights_table on the pertinent set.
// --payload-len L (with --indexed-weights) makes the payload length a parameter of the board (include/omr_gpu.h,
// "Payload length as a board parameter"): payloads of L words, 1 <= L <= 16384, in omr_get_payload_layout's
// ciphertexts; the detector encodes with omr_encode_payloads_indexed_len (or a session from
// omr_digest_begin_indexed_len) and the recipient solves with omr_retrieve_payloads_indexed_len (with
// --device-retrieve: omr_auditor_retrieve_payloads_indexed_len). Works with --session, --compact, --bitmap.
// --seek-weights keeps the reference's weights and drops the table (include/omr_gpu.h, "Reference payload weights
// by seek"): the detector builds the seek of the board on its device and encodes with omr_encode_payloads_seek
// (or a session from omr_digest_begin_seek), the recipient solves with omr_retrieve_payloads_seek, which builds its
// own seek (with --device-retrieve: omr_auditor_retrieve_payloads_seek, on the auditor's device). With --host-only
// it checks omr_payload_weights_at against omr_payload_weights' table on the pertinent set.
// --sender plays the sender as a party of its own (include/omr_gpu.h, "Sender"): the board comes from one
// omr_sender_gen_clues over the two packs' public clue keys (recipient 0, the detector's pack, where a message
// is pertinent, 1 elsewhere) instead of two full generations and a merge; the recipient audits the clue key it
// published (omr_clue_key_audit) and opens the board (omr_clue_open), whose pertinent set must be the board's,
// before anything is detected. The rest of the flow is unchanged; with --host-only these CPU parts run.
// --host-only runs the CPU parts of the ABI (keys, clues, weights, retrieval parameters) without
// a GPU (used by the CPU test suite).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "omr_gpu.h"

namespace {

constexpr size_t N0 = 512, CLUES = 7, N2 = 2048, PAYLOAD = 612;
constexpr size_t BSK1 = 512ull * 8 * 2 * 1024, KSK = 1024ull * 27 * 671, BSK2 = 670ull * 12 * 2 * 2048,
                 TK = 11ull * 25 * 2 * 2048;
constexpr size_t BSK1_B = BSK1 / 2, KSK_B = 1024ull * 27, BSK2_B = BSK2 / 2, TK_B = TK / 2;  // seeded bodies

using clk = std::chrono::steady_clock;
double secs(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

#define CHECK(expr)                                                                    \
  do {                                                                                 \
    omr_status st_ = (expr);                                                           \
    if (st_ != OMR_OK) {                                                               \
      std::fprintf(stderr, "%s failed (%d): %s\n", #expr, (int)st_, omr_last_error()); \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

}  // namespace

int main(int argc, char **argv) {
  size_t D = 4096;
  int device = 0;
  uint64_t seed = 2025;
  bool host_only = false;
  size_t session_piece = 0;  // --session: messages per omr_digest_update call
  bool audit = false, bitmap = false, seeded = false, audit_key = false, indexed = false, seek_weights = false, device_retrieve = false, sender = false;
  int compact_bits = 0;  // --compact: bits per coefficient of the digest on the wire
  bool by_len = false;     // --payload-len given: the payload length is a parameter of the (indexed) board
  size_t payload_len = 0;  // its words per payload, 1 .. OMR_PAYLOAD_LEN_MAX
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if ((a == "-p" || a == "--payload-count") && i + 1 < argc) D = std::max<size_t>(1, std::stoull(argv[++i]));
    else if ((a == "-d" || a == "--device") && i + 1 < argc) device = std::atoi(argv[++i]);
    else if ((a == "-s" || a == "--seed") && i + 1 < argc) seed = std::stoull(argv[++i]);
    else if (a == "--session" && i + 1 < argc) session_piece = std::max<size_t>(1, std::stoull(argv[++i]));
    else if (a == "--audit") audit = true;
    else if (a == "--bitmap") bitmap = true;
    else if (a == "--seeded") seeded = true;
    else if (a == "--compact" && i + 1 < argc) compact_bits = std::atoi(argv[++i]);
    else if (a == "--audit-key") audit_key = true;
    else if (a == "--indexed-weights") indexed = true;
    else if (a == "--payload-len" && i + 1 < argc) {
      // digits only (stoull would take a sign and wrap it), and in the library's range: 0 is no length
      const std::string v = argv[++i];
      const bool digits = !v.empty() && v.size() <= 5 && v.find_first_not_of("0123456789") == std::string::npos;
      payload_len = digits ? std::stoull(v) : 0;
      if (payload_len < 1 || payload_len > OMR_PAYLOAD_LEN_MAX) {
        std::fprintf(stderr, "--payload-len takes a length of 1 to %d words, not '%s'\n", OMR_PAYLOAD_LEN_MAX, v.c_str());
        return 2;
      }
      by_len = true;
    }
    else if (a == "--seek-weights") seek_weights = true;
    else if (a == "--device-retrieve") device_retrieve = true;
    else if (a == "--sender") sender = true;
    else if (a == "--host-only") host_only = true;
    else {
      std::fprintf(stderr, "usage: %s [-p payload_count] [-d device] [-s seed] [--session PIECE] [--audit] [--bitmap] "
                   "[--seeded] [--compact BITS] [--audit-key] [--indexed-weights] [--payload-len L] [--seek-weights] "
                   "[--device-retrieve] [--sender] [--host-only]\n",
                   argv[0]);
      return 2;
    }
  }
  if (by_len && !indexed) {
    std::fprintf(stderr, "--payload-len needs --indexed-weights: the table and seek conventions stay at 612 words\n");
    return 2;
  }
  std::printf("%s; all payloads count: %zu\n", omr_version(), D);

  // KeyGen::generate_secret_key x2, generate_detector (omr.rs:76-83)
  auto t = clk::now();
  omr_secret_key_pack *pa = nullptr, *pb = nullptr;
  CHECK(omr_keygen_secret(seed ^ 0xA, &pa));
  CHECK(omr_keygen_secret(seed ^ 0xB, &pb));
  // full key, or with --seeded the bodies alone (the full key only where the host expands it)
  const bool full = !seeded || host_only;
  std::vector<uint32_t> bsk1(full ? BSK1 : 0), ksk(full ? KSK : 0), bsk1_b(seeded ? BSK1_B : 0), ksk_b(seeded ? KSK_B : 0);
  std::vector<uint64_t> bsk2(full ? BSK2 : 0), tk(full ? TK : 0), bsk2_b(seeded ? BSK2_B : 0), tk_b(seeded ? TK_B : 0);
  const omr_seeded_key_view sview{bsk1_b.data(), ksk_b.data(), bsk2_b.data(), tk_b.data(), seed ^ 0x5EED};
  if (seeded) {
    CHECK(omr_keygen_seeded_key(pa, seed ^ 0xD, sview.mask_seed, bsk1_b.data(), ksk_b.data(), bsk2_b.data(), tk_b.data(), 0));
    std::printf("seeded keygen time: %.3f s (%zu bytes on the wire, %zu expanded)\n", secs(t),
                BSK1_B * 4 + KSK_B * 4 + BSK2_B * 8 + TK_B * 8 + 8, BSK1 * 4 + KSK * 4 + BSK2 * 8 + TK * 8);
  } else {
    CHECK(omr_keygen_detection_key(pa, seed ^ 0xD, bsk1.data(), ksk.data(), bsk2.data(), tk.data(), 0));
    std::printf("keygen time: %.3f s\n", secs(t));
  }
  if (seeded && host_only) {
    t = clk::now();
    CHECK(omr_expand_detection_key(&sview, bsk1.data(), ksk.data(), bsk2.data(), tk.data(), 0));
    std::printf("host expansion time: %.3f s\n", secs(t));
    // the last row of every component: a = omr_key_masks, b = the body
    std::vector<uint32_t> m1(1024), mk(670);
    std::vector<uint64_t> m2(2048), mt(2048);
    CHECK(omr_key_masks(sview.mask_seed, OMR_KEY_BSK1, 4095, 1, m1.data()));
    CHECK(omr_key_masks(sview.mask_seed, OMR_KEY_KSK, 27647, 1, mk.data()));
    CHECK(omr_key_masks(sview.mask_seed, OMR_KEY_BSK2, 8039, 1, m2.data()));
    CHECK(omr_key_masks(sview.mask_seed, OMR_KEY_TRACE, 274, 1, mt.data()));
    const bool ok = std::equal(m1.begin(), m1.end(), &bsk1[BSK1 - 2048]) && std::equal(mk.begin(), mk.end(), &ksk[KSK - 671]) &&
                    std::equal(m2.begin(), m2.end(), &bsk2[BSK2 - 4096]) && std::equal(mt.begin(), mt.end(), &tk[TK - 4096]) &&
                    std::equal(&bsk1[BSK1 - 1024], &bsk1[BSK1], &bsk1_b[BSK1_B - 1024]) && ksk[KSK - 1] == ksk_b[KSK_B - 1] &&
                    std::equal(&bsk2[BSK2 - 2048], &bsk2[BSK2], &bsk2_b[BSK2_B - 2048]) &&
                    std::equal(&tk[TK - 2048], &tk[TK], &tk_b[TK_B - 2048]);
    if (!ok) {
      std::printf("Fail: the expanded key is not (omr_key_masks, body)\nFAILED\n");
      return 1;
    }
    std::printf("host-only: seeded key expands to (omr_key_masks, body) rows\n");
  }

  // pertinent = first min(D, 50) of a shuffle (omr.rs:103-113)
  const size_t pert_count = std::min<size_t>(D, 50);
  std::vector<size_t> order(D);
  std::iota(order.begin(), order.end(), 0);
  std::mt19937_64 rng(seed);
  std::shuffle(order.begin(), order.end(), rng);
  std::vector<size_t> pert(order.begin(), order.begin() + pert_count);
  std::sort(pert.begin(), pert.end());
  std::vector<char> is_pert(D, 0);
  for (size_t i : pert) is_pert[i] = 1;

  // Sender::gen_clues for every message (omr.rs:126-135)
  t = clk::now();
  std::vector<uint16_t> ca(D * N0), cb(D * CLUES);
  if (sender) {
    // the sender holds the two public clue keys and nothing else: one generation, each message under its recipient
    omr_clue_key keys[2];
    CHECK(omr_secret_clue_key(pa, &keys[0]));
    CHECK(omr_secret_clue_key(pb, &keys[1]));
    std::vector<uint32_t> recipient(D);
    for (size_t m = 0; m < D; ++m) recipient[m] = is_pert[m] ? 0 : 1;
    omr_sender *snd = nullptr;
    CHECK(omr_sender_create(keys, 2, -1, &snd));
    CHECK(omr_sender_gen_clues(snd, recipient.data(), seed + 1, 0, D, ca.data(), cb.data(), 0));
    omr_sender_destroy(snd);
    std::printf("gen clues time: %.3f s (one sender over 2 clue keys)\n", secs(t));
    // the recipient's checks: the key it published, and which messages of the board are its own
    uint64_t K = 0, key_max = 0;
    uint32_t over = 0, noncanon = 0;
    CHECK(omr_clue_key_noise_support(&K));
    CHECK(omr_clue_key_audit(pa, &keys[0], UINT64_MAX, &key_max, &over, &noncanon));
    std::vector<uint8_t> opened(D), open_noise(D);
    CHECK(omr_clue_open(pa, ca.data(), cb.data(), D, nullptr, opened.data(), open_noise.data(), 0));
    size_t wrong = 0, n_open = 0;
    uint8_t worst = 0;
    for (size_t m = 0; m < D; ++m) {
      wrong += (opened[m] != 0) != (is_pert[m] != 0);
      n_open += opened[m] != 0;
      if (opened[m]) worst = std::max(worst, open_noise[m]);
    }
    std::printf("sender: clue key max |e| %llu (support %llu), %u over, %u non-canonical words; %zu of %zu clues open as "
                "pertinent, max |noise| %u of 128\n",
                (unsigned long long)key_max, (unsigned long long)K, over, noncanon, n_open, D, (unsigned)worst);
    if (over || noncanon || wrong) {
      std::printf("Fail: %s\nFAILED\n", wrong ? "omr_clue_open's pertinent set is not the board's" : "the clue key fails its audit");
      return 1;
    }
  } else {
    std::vector<uint16_t> xa(D * N0), xb(D * CLUES);
    CHECK(omr_gen_clues(pa, seed + 1, 0, D, ca.data(), cb.data(), 0));
    CHECK(omr_gen_clues(pb, seed + 2, 0, D, xa.data(), xb.data(), 0));
    for (size_t m = 0; m < D; ++m)
      if (!is_pert[m]) {
        std::copy_n(&xa[m * N0], N0, &ca[m * N0]);
        std::copy_n(&xb[m * CLUES], CLUES, &cb[m * CLUES]);
      }
    std::printf("gen clues time: %.3f s\n", secs(t));
  }

  omr_retrieval_params rp;
  CHECK(omr_get_retrieval_params(D, pert_count, &rp));
  // the payload digest's layout: the reference's (2 combinations of 612 words per ciphertext) or the length's own
  omr_payload_layout ly{(uint32_t)PAYLOAD, rp.combination_count, rp.cmb_count_per_cipher, 1, rp.cmb_cipher_count};
  if (by_len) CHECK(omr_get_payload_layout(pert_count, payload_len, &ly));
  const size_t plen = ly.payload_len;

  // Payload::random (omr.rs:140-146)
  std::vector<uint16_t> payloads(D * plen);
  for (auto &b : payloads) b = (uint16_t)(rng() & 0xff);

  uint8_t wseed[32];
  for (int i = 0; i < 32; ++i) wseed[i] = (uint8_t)(rng() & 0xff);
  if (indexed && seek_weights) {
    std::fprintf(stderr, "--indexed-weights and --seek-weights are two conventions: choose one\n");
    return 2;
  }
  // the board-wide table of the reference's weights; with --indexed-weights or --seek-weights nobody needs one
  const bool table = !indexed && !seek_weights;
  std::vector<uint16_t> weights(table ? (size_t)rp.cmb_cipher_count * rp.cmb_count_per_cipher * D : 0);
  if (table)
    CHECK(omr_payload_weights(wseed, D, rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher,
                              weights.data()));
  std::printf("retrieval params: %u index ct, %u payload ct (%u combinations)\n",
              rp.max_encode_indices_cipher_count, ly.payload_ct, rp.combination_count);
  if (by_len)
    std::printf("payload layout: %u words, %u combinations per ciphertext, %u stripes\n", ly.payload_len,
                ly.cmb_count_per_cipher, ly.stripes);
  uint32_t n_bmp = 0;
  if (bitmap) CHECK(omr_bitmap_ct_count(D, &n_bmp));
  if (host_only && bitmap) {
    // the layout on the host: the board's pertinent set as decoded bitmap values, and back
    std::vector<uint16_t> dec((size_t)n_bmp * N2, 0);
    for (size_t g : pert) {
      const size_t l = g % OMR_BITMAP_MESSAGES_PER_CT;
      dec[g / OMR_BITMAP_MESSAGES_PER_CT * N2 + l % N2] |= (uint16_t)(1u << (l / N2));
    }
    std::vector<size_t> back(pert_count);
    size_t nback = 0;
    CHECK(omr_bitmap_indices(dec.data(), n_bmp, D, back.data(), back.size(), &nback));
    if (nback != pert_count || back != pert) {
      std::printf("Fail: bitmap layout returns %zu indices, %zu pertinent\nFAILED\n", nback, pert.size());
      return 1;
    }
    std::printf("host-only: bitmap layout OK (%u bitmap ct, %zu indices)\n", n_bmp, nback);
  }
  if (host_only && indexed) {
    // the recipient's submatrix against the table layout: the same function of (seed, combination, index)
    const size_t rows = (size_t)rp.cmb_cipher_count * rp.cmb_count_per_cipher;
    std::vector<uint16_t> table(rows * D), at(rows * pert_count);
    CHECK(omr_indexed_weights_table(wseed, D, rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher,
                                    table.data(), 0));
    CHECK(omr_indexed_weights_at(wseed, rp.combination_count, 0, (uint32_t)rows, pert.data(), pert_count, at.data(), 0));
    bool ok = true;
    for (size_t j = 0; j < rows; ++j)
      for (size_t k = 0; k < pert_count; ++k) {
        const uint16_t w = at[j * pert_count + k];
        ok = ok && w == table[j * D + pert[k]] && w <= 256 && (j < rp.combination_count || w == 0);
      }
    if (!ok) {
      std::printf("Fail: omr_indexed_weights_at differs from omr_indexed_weights_table\nFAILED\n");
      return 1;
    }
    std::printf("host-only: indexed weights OK (%zu x %zu submatrix of a %zu x %zu table)\n", rows, pert_count, rows, D);
  }
  if (host_only && seek_weights) {
    // the recipient's submatrix through the seek against the table the reference would draw
    const size_t rows = (size_t)rp.cmb_cipher_count * rp.cmb_count_per_cipher;
    std::vector<uint16_t> tab(rows * D), at(rows * pert_count);
    omr_weight_seek sk;
    CHECK(omr_payload_weights(wseed, D, rp.combination_count, rp.cmb_cipher_count, rp.cmb_count_per_cipher, tab.data()));
    CHECK(omr_weight_seek_build_cpu(wseed, (uint64_t)rp.combination_count * D, 0, &sk));
    CHECK(omr_payload_weights_at(wseed, D, rp.combination_count, &sk, 0, (uint32_t)rows, pert.data(), pert_count,
                                 at.data(), 0));
    bool ok = true;
    for (size_t j = 0; j < rows; ++j)
      for (size_t k = 0; k < pert_count; ++k) ok = ok && at[j * pert_count + k] == tab[j * D + pert[k]];
    if (!ok) {
      std::printf("Fail: omr_payload_weights_at differs from omr_payload_weights\nFAILED\n");
      return 1;
    }
    std::printf("host-only: seek weights OK (%zu x %zu submatrix of a %zu x %zu table, %u rejections)\n", rows, pert_count,
                rows, D, sk.n);
  }
  if (host_only) {
    std::printf("host-only: keys, clues, weights and parameters OK\n");
    omr_secret_destroy(pa);
    omr_secret_destroy(pb);
    return 0;
  }

  // Detector::new + detect over the board (omr.rs:160-164)
  omr_ctx *ctx = nullptr;
  omr_detection_key_view view{bsk1.data(), ksk.data(), bsk2.data(), tk.data()};
  if (audit_key) {
    // the recipient's check before the key leaves: every row's noise inside the generators' support
    static const char *const comp_name[4] = {"bsk1", "ksk", "bsk2", "trace_key"};
    omr_auditor *ka = nullptr;
    CHECK(omr_auditor_create(pa, device, &ka));
    omr_key_audit_summary ks[4];
    for (auto &k : ks) {
      std::memset(&k, 0, sizeof k);
      k.first_row_over = UINT64_MAX;
    }
    t = clk::now();
    if (seeded) CHECK(omr_audit_key_seeded(ka, &sview, nullptr, ks));
    else CHECK(omr_audit_key(ka, &view, nullptr, ks));
    std::printf("key audit time: %.3f s (%s)\n", secs(t), seeded ? "seeded key, expanded on the device" : "full key, staged");
    omr_auditor_destroy(ka);
    bool bad = false;
    for (int c = 0; c < 4; ++c) {
      uint64_t K = 0;
      CHECK(omr_key_noise_support(c, &K));
      std::printf("key audit %-9s: %llu rows, max |e| %llu (support %llu), %llu over, %llu non-canonical words\n", comp_name[c],
                  (unsigned long long)ks[c].rows, (unsigned long long)ks[c].max_abs_noise, (unsigned long long)K,
                  (unsigned long long)ks[c].rows_over, (unsigned long long)ks[c].noncanonical);
      if (ks[c].rows_over) {
        std::printf("Fail: %s row %llu has noise outside the generators' support\n", comp_name[c],
                    (unsigned long long)ks[c].first_row_over);
        bad = true;
      }
    }
    if (bad) {
      std::printf("FAILED\n");
      return 1;
    }
    std::printf("key audit OK\n");
  }
  t = clk::now();
  if (seeded) CHECK(omr_ctx_create_seeded(&sview, device, &ctx));
  else CHECK(omr_ctx_create(&view, device, &ctx));
  std::printf("detector creation time: %.3f s (%s)\n", secs(t), seeded ? "seeded key, expanded on the device" : "full key");
  const uint32_t n_idx = rp.max_encode_indices_cipher_count, n_pay = ly.payload_ct;
  omr_auditor *aud = nullptr;
  if (audit) CHECK(omr_auditor_create(pa, device, &aud));
  int audit_fails = 0;
  omr_audit_summary pv_sum{}, dg_sum{};
  std::vector<uint64_t> idx_ct((size_t)n_idx * 2 * N2), pay_ct((size_t)n_pay * 2 * N2), bmp_ct((size_t)n_bmp * 2 * N2);
  size_t ctb = 0;  // bytes of one compact ciphertext
  if (compact_bits) CHECK(omr_compact_ct_bytes(compact_bits, &ctb));
  std::vector<uint8_t> idx_pk(n_idx * ctb), pay_pk(n_pay * ctb), bmp_pk(n_bmp * ctb);
  if (session_piece) {
    // the same flow inside the library, piece by piece (omr_digest_*): detect + both encoders
    t = clk::now();
    omr_digest *dg = nullptr;
    if (by_len) CHECK(omr_digest_begin_indexed_len(ctx, D, pert_count, seed + 3, wseed, payload_len, nullptr, &dg));
    else if (indexed) CHECK(omr_digest_begin_indexed(ctx, D, pert_count, seed + 3, wseed, nullptr, &dg));
    else if (seek_weights) CHECK(omr_digest_begin_seek(ctx, D, pert_count, seed + 3, wseed, nullptr, &dg));
    else CHECK(omr_digest_begin(ctx, D, pert_count, seed + 3, wseed, nullptr, &dg));
    if (bitmap) CHECK(omr_digest_enable_bitmap(dg));
    for (size_t off = 0; off < D; off += session_piece) {
      const size_t n = std::min(session_piece, D - off);
      CHECK(omr_digest_update(dg, &ca[off * N0], &cb[off * CLUES], &payloads[off * plen], n, off));
    }
    CHECK(omr_digest_read(dg, idx_ct.data(), pay_ct.data()));
    if (bitmap) CHECK(omr_digest_read_bitmap(dg, bmp_ct.data()));
    if (compact_bits) CHECK(omr_digest_read_compact(dg, compact_bits, idx_pk.data(), pay_pk.data(), bitmap ? bmp_pk.data() : nullptr));
    omr_digest_info info;
    CHECK(omr_digest_get_info(dg, &info));
    omr_digest_destroy(dg);
    const double ts = secs(t);
    std::printf("digest session time: %.3f s (%.3f ms per message, host pieces of %zu, %zu messages folded in, "
                "room for %zu pertinency ciphertexts)\n",
                ts, ts * 1e3 / D, session_piece, info.messages, info.pv_capacity_messages);
    if (info.messages != D) {
      std::printf("FAILED\n");
      return 1;
    }
  } else {
    std::vector<uint64_t> pv(D * 2 * N2);
    t = clk::now();
    CHECK(omr_detect_batch(ctx, ca.data(), cb.data(), D, pv.data()));
    const double td = secs(t);
    std::printf("detect time: %.3f s (%.3f ms per message, host buffers)\n", td, td * 1e3 / D);
    if (audit) {
      // the omd KAT over the whole board: one-hot exactly where pertinent, zeros elsewhere
      std::vector<omr_ct_audit> rec(D);
      CHECK(omr_audit(aud, pv.data(), D, rec.data(), nullptr, &pv_sum));
      for (size_t m = 0; m < D; ++m) {
        const bool one_hot = rec[m].nonzero == 1 && rec[m].first == 1, zero = rec[m].nonzero == 0;
        if (is_pert[m] ? !one_hot : !zero) {
          if (!audit_fails) std::printf("Fail: message %zu (%s) decrypts to %u non-zero coefficients, first %u\n", m,
                                        is_pert[m] ? "pertinent" : "not pertinent", rec[m].nonzero, rec[m].first);
          ++audit_fails;
        }
      }
      if (pv_sum.other || pv_sum.one_hot != pert_count || pv_sum.zero != D - pert_count) ++audit_fails;
    }

    // encode_pertinent_indices x max_encode_indices_cipher_count, encode_pertinent_payloads
    t = clk::now();
    for (uint32_t c = 0; c < n_idx; ++c)
      CHECK(omr_encode_indices(ctx, pv.data(), D, 0, D, seed + 3, c, &idx_ct[(size_t)c * 2 * N2]));
    std::printf("encode indices time: %.3f s\n", secs(t));
    t = clk::now();
    if (by_len) {
      CHECK(omr_encode_payloads_indexed_len(ctx, pv.data(), payloads.data(), D, 0, D, wseed, ly.combination_count,
                                            ly.payload_len, ly.cmb_count_per_cipher, 0, n_pay, pay_ct.data()));
    } else if (indexed) {
      CHECK(omr_encode_payloads_indexed(ctx, pv.data(), payloads.data(), D, 0, D, wseed, rp.combination_count, 0, n_pay,
                                        rp.cmb_count_per_cipher, pay_ct.data()));
    } else if (seek_weights) {
      // the scan runs on the calling thread's current HIP device: the detector's, selected when it was created
      omr_weight_seek sk;
      CHECK(omr_weight_seek_build_device(wseed, (uint64_t)rp.combination_count * D, &sk, nullptr));
      std::printf("weight seek: %u rejections in %llu draws\n", sk.n, (unsigned long long)sk.draws);
      CHECK(omr_encode_payloads_seek(ctx, pv.data(), payloads.data(), D, 0, D, wseed, &sk, rp.combination_count, 0, n_pay,
                                     rp.cmb_count_per_cipher, pay_ct.data()));
    } else
      CHECK(omr_encode_payloads(ctx, pv.data(), payloads.data(), D, 0, D, weights.data(), n_pay,
                                rp.cmb_count_per_cipher, pay_ct.data()));
    std::printf("encode pertinent payloads time: %.3f s%s\n", secs(t),
                indexed ? " (indexed weights)" : seek_weights ? " (reference weights by seek)" : "");
    if (bitmap) {
      t = clk::now();
      CHECK(omr_encode_bitmap(ctx, pv.data(), D, 0, D, bmp_ct.data()));
      std::printf("encode bitmap time: %.3f s\n", secs(t));
    }
    if (compact_bits) {
      CHECK(omr_compact_cts(ctx, idx_ct.data(), n_idx, compact_bits, idx_pk.data()));
      CHECK(omr_compact_cts(ctx, pay_ct.data(), n_pay, compact_bits, pay_pk.data()));
      CHECK(omr_compact_cts(ctx, bmp_ct.data(), n_bmp, compact_bits, bmp_pk.data()));
    }
  }

  int compact_fails = 0;
  if (compact_bits) {
    // the recipient's side: expand what arrived and retrieve from that; the full digest is kept only to
    // measure what compaction cost
    uint64_t R = 0, before = 0, after = 0, grow = 0;
    CHECK(omr_compact_residual_bound(pa, compact_bits, &R));
    struct Part {
      std::vector<uint64_t> *full;
      std::vector<uint8_t> *packed;
      uint32_t n;
    } parts[3] = {{&idx_ct, &idx_pk, n_idx}, {&pay_ct, &pay_pk, n_pay}, {&bmp_ct, &bmp_pk, n_bmp}};
    for (Part &pt : parts) {
      if (!pt.n) continue;
      std::vector<omr_ct_audit> r0(pt.n), r1(pt.n);
      std::vector<uint16_t> d0((size_t)pt.n * N2), d1((size_t)pt.n * N2);
      CHECK(omr_audit_cpu(pa, pt.full->data(), pt.n, r0.data(), d0.data(), nullptr, 0));
      CHECK(omr_compact_expand_cpu(pt.packed->data(), pt.n, compact_bits, pt.full->data(), 0));
      CHECK(omr_audit_cpu(pa, pt.full->data(), pt.n, r1.data(), d1.data(), nullptr, 0));
      if (d0 != d1) ++compact_fails;
      for (uint32_t c = 0; c < pt.n; ++c) {
        before = std::max(before, r0[c].max_abs_residual);
        after = std::max(after, r1[c].max_abs_residual);
        if (r1[c].max_abs_residual > r0[c].max_abs_residual) grow = std::max(grow, r1[c].max_abs_residual - r0[c].max_abs_residual);
      }
    }
    if (grow > R) ++compact_fails;
    const size_t n_all = (size_t)n_idx + n_pay + n_bmp;
    std::printf("compact digest: %zu ciphertexts at %d bits, %zu bytes instead of %zu; R/q2 %.4e, max |r|/q2 %.3e -> %.3e, "
                "largest increase %.3e%s\n",
                n_all, compact_bits, n_all * ctb, n_all * 2 * N2 * 8, (double)R / (double)OMR_Q2,
                (double)before / (double)OMR_Q2, (double)after / (double)OMR_Q2, (double)grow / (double)OMR_Q2,
                compact_fails ? " -- FAILED" : "");
  }

  if (audit) {
    CHECK(omr_audit(aud, idx_ct.data(), n_idx, nullptr, nullptr, &dg_sum));
    CHECK(omr_audit(aud, pay_ct.data(), n_pay, nullptr, nullptr, &dg_sum));
    std::printf("audit: pertinency vector %llu one-hot, %llu zero, %llu other, max |r|/q2 %.3e; digests %llu "
                "ciphertexts, max |r|/q2 %.3e%s\n",
                (unsigned long long)pv_sum.one_hot, (unsigned long long)pv_sum.zero, (unsigned long long)pv_sum.other,
                (double)pv_sum.max_abs_residual / (double)OMR_Q2, (unsigned long long)dg_sum.ciphertexts,
                (double)dg_sum.max_abs_residual / (double)OMR_Q2, audit_fails ? " -- FAILED" : "");
    if (bitmap) {
      omr_audit_summary bmp_sum{};
      CHECK(omr_audit(aud, bmp_ct.data(), n_bmp, nullptr, nullptr, &bmp_sum));
      std::printf("audit: bitmap digest %u ciphertexts, max |r|/q2 %.3e (decode limit 0.5)\n", n_bmp,
                  (double)bmp_sum.max_abs_residual / (double)OMR_Q2);
    }
    omr_auditor_destroy(aud);
  }

  // Retriever::decode_digest (omr.rs:216-218)
  t = clk::now();
  std::vector<size_t> found(pert_count + 64);
  size_t nfound = 0;
  // --device-retrieve: the recipient's auditor takes the digest in the form it arrived in
  omr_auditor *ra = nullptr;
  if (device_retrieve) CHECK(omr_auditor_create(pa, device, &ra));
  const void *dev_idx = compact_bits ? (const void *)idx_pk.data() : (const void *)idx_ct.data();
  const void *dev_pay = compact_bits ? (const void *)pay_pk.data() : (const void *)pay_ct.data();
  if (bitmap) {
    // no count needed: the bitmap says how many there are, and whether the board's layout covers them
    CHECK(omr_retrieve_bitmap(pa, bmp_ct.data(), n_bmp, D, found.data(), found.size(), &nfound));
    std::printf("bitmap digest: %u ciphertexts, %zu pertinent indices (the board's %u combinations %s)\n", n_bmp,
                nfound, rp.combination_count, nfound <= rp.combination_count ? "cover them" : "do NOT cover them");
  } else if (device_retrieve) {
    CHECK(omr_auditor_retrieve_indices(ra, dev_idx, n_idx, compact_bits, D, pert_count, found.data(), found.size(), &nfound));
  } else {
    CHECK(omr_retrieve_indices(pa, idx_ct.data(), n_idx, D, pert_count, found.data(), found.size(), &nfound));
  }
  found.resize(std::min(nfound, found.size()));
  std::vector<uint16_t> solved(found.size() * plen);
  if (by_len && device_retrieve)
    CHECK(omr_auditor_retrieve_payloads_indexed_len(ra, dev_pay, n_pay, compact_bits, D, &ly, wseed, found.data(),
                                                    found.size(), solved.data()));
  else if (by_len)
    CHECK(omr_retrieve_payloads_indexed_len(pa, pay_ct.data(), n_pay, D, &ly, wseed, found.data(), found.size(),
                                            solved.data()));
  else if (device_retrieve && indexed)
    CHECK(omr_auditor_retrieve_payloads_indexed(ra, dev_pay, n_pay, compact_bits, D, rp.combination_count, wseed,
                                                found.data(), found.size(), solved.data()));
  else if (device_retrieve && seek_weights)
    CHECK(omr_auditor_retrieve_payloads_seek(ra, dev_pay, n_pay, compact_bits, D, rp.combination_count, wseed, nullptr,
                                             found.data(), found.size(), solved.data()));
  else if (device_retrieve)
    CHECK(omr_auditor_retrieve_payloads(ra, dev_pay, n_pay, compact_bits, D, rp.combination_count, weights.data(),
                                        found.data(), found.size(), solved.data()));
  else if (indexed)
    CHECK(omr_retrieve_payloads_indexed(pa, pay_ct.data(), n_pay, D, rp.combination_count, wseed, found.data(),
                                        found.size(), solved.data()));
  else if (seek_weights)
    CHECK(omr_retrieve_payloads_seek(pa, pay_ct.data(), n_pay, D, rp.combination_count, wseed, nullptr, found.data(),
                                     found.size(), solved.data()));
  else
    CHECK(omr_retrieve_payloads(pa, pay_ct.data(), n_pay, D, rp.combination_count, weights.data(), found.data(),
                                found.size(), solved.data()));
  std::printf("decode time: %.3f s%s\n", secs(t), device_retrieve ? " (on the auditor's device)" : "");
  omr_auditor_destroy(ra);

  int fails = (found == pert ? 0 : 1) + audit_fails + compact_fails;
  if (fails) std::printf("Fail: %zu indices recovered, %zu pertinent\n", found.size(), pert.size());
  for (size_t k = 0; k < found.size() && !fails; ++k)
    if (!std::equal(&solved[k * plen], &solved[(k + 1) * plen], &payloads[found[k] * plen])) {
      std::printf("Fail %zu\n", found[k]);
      ++fails;
    }
  std::printf(fails ? "FAILED\n" : "All done: %zu pertinent indices and payloads recovered\n", found.size());
  omr_ctx_destroy(ctx);
  omr_secret_destroy(pa);
  omr_secret_destroy(pb);
  return fails ? 1 : 0;
}
