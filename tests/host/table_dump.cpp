// Writes every table of csrc/host_tables.hpp as raw binary, one file per table, into the directory
// given as argv[1] (tests/test_host_tables.py compares them with tests/golden/host_tables.npz).
// Host code only, built with the library's flags (notably -ffp-contract=off):
//   hipcc <FLAGS of tfhe-omr_amd/Makefile> --cuda-host-only -x hip tests/host/table_dump.cpp -o table_dump
#include <cstdio>
#include <string>
#include <vector>

#include "../../tfhe-omr_amd/csrc/host_tables.hpp"

using namespace omr;

namespace {
std::string dir;
template <typename T>
bool put(const char *name, const std::vector<T> &v) {
  FILE *f = fopen((dir + "/" + name + ".bin").c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}
// apriori_bound's input for a level: a deterministic ramp of the level's shape [steps][rows][outputs]
std::vector<double> ramp(size_t n) {
  std::vector<double> k(n);
  for (size_t i = 0; i < n; ++i) k[i] = 1.0 + (double)((i * 37) % 1024) / 1024.0;
  return k;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  dir = argv[1];
  bool ok = true;
  std::vector<double> tw1, itw1, tw2, itw2;
  twiddles(Q1, N1, 7, tw1, itw1);
  twiddles(Q2, N2, 22, tw2, itw2);
  ok &= put("tw1", tw1) && put("itw1", itw1) && put("tw2", tw2) && put("itw2", itw2);
  ok &= put("ninv", std::vector<double>{ninv_centred(N1, Q1), ninv_centred(N2, Q2)});
  ok &= put("lut1", first_level_lut()) && put("lut2", second_level_lut());
  ok &= put("tw2c", cmux_twiddles(tw2));
  ok &= put("trace_tabs", trace_tables());
  ok &= put("fft1", fft_twiddles()) && put("fft2", fft2_twiddles());
  ok &= put("dd_tree9", dd_tree_twiddles(9)) && put("dd_tree10", dd_tree_twiddles(10));
  const size_t n1 = (size_t)N0 * 2 * D1 * 2, n2 = (size_t)NI * 2 * D2 * 4, nt = (size_t)TRACE_STEPS * DT * 4;
  ok &= put("apriori", std::vector<double>{apriori_bound(1, ramp(n1)), apriori_bound(2, ramp(n2)),
                                           apriori_bound(3, ramp(n2)), apriori_bound(4, ramp(nt))});
  return ok ? 0 : 1;
}
