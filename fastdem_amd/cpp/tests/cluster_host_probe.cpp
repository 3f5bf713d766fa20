// cluster_host_probe.cpp — the host algebra of Euclidean clustering (csrc/fdm_cluster_host.hpp) as a stand-alone CPU
// program: no device, no library.  Reads an operation and its numbers (hexadecimal floats) from standard input and prints
// the result the same way.  tests/test_cluster_restate.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer
// and holds it to the NumPy restatement.
//   1 tol                           -> ok, inv, r_sq, range of the relation
//   2 lo[3] hi[3] range             -> ok, ext[3], bits_x, bits_y, bits of the key over the box
//   3 m                             -> bits_root, bits of the ordering key
//   4 lo[3] hi[3] range v[3]        -> the packed key of biased voxel v and the voxel unpacked from it again [1 + 3]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fdm_cluster_host.hpp"

int main() {
  using namespace fdm;
  std::vector<double> in;
  char tok[128];
  while (std::scanf("%127s", tok) == 1) in.push_back(std::strtod(tok, nullptr));
  if (in.empty()) return 2;
  const int op = int(in[0]);
  const double* a = in.data() + 1;
  const size_t n = in.size() - 1;
  std::vector<double> out;
  if (op == 1 && n == 1) {
    cluster::Relation R{0.0f, 0.0f, 0};
    const bool ok = cluster::relation(float(a[0]), R);
    out = {ok ? 1.0 : 0.0, ok ? double(R.inv) : 0.0, ok ? double(R.r_sq) : 0.0, ok ? double(R.range) : 0.0};
  } else if ((op == 2 && n == 7) || (op == 4 && n == 10)) {
    uint32_t lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = uint32_t(a[k]); hi[k] = uint32_t(a[3 + k]); }
    ClusterBox B{};
    unsigned bits = 0;
    const bool ok = cluster::box(lo, hi, int(a[6]), B, bits);
    if (op == 2) {
      out = {ok ? 1.0 : 0.0};
      if (ok) out.insert(out.end(), {double(B.ext[0]), double(B.ext[1]), double(B.ext[2]), double(B.bits_x),
                                     double(B.bits_y), double(bits)});
    } else {
      if (!ok) return 2;
      const uint64_t v[3] = {uint64_t(a[7]), uint64_t(a[8]), uint64_t(a[9])};
      for (int k = 0; k < 3; ++k)
        if (v[k] < lo[k] || v[k] > hi[k]) return 2;
      const unsigned sh = B.bits_x + B.bits_y;
      const uint64_t key = ((v[2] - lo[2]) << sh) | ((v[1] - lo[1]) << B.bits_x) | (v[0] - lo[0]);
      if (bits < 64 && (key >> bits) != 0) return 3;
      out = {double(key), double((key & ((1ull << B.bits_x) - 1)) + lo[0]),
             double(((key >> B.bits_x) & ((1ull << B.bits_y) - 1)) + lo[1]), double((key >> sh) + lo[2])};
    }
  } else if (op == 3 && n == 1) {
    unsigned bits_root = 0, bits = 0;
    cluster::order_bits(uint32_t(a[0]), bits_root, bits);
    out = {double(bits_root), double(bits)};
  } else {
    return 2;
  }
  for (double v : out) std::printf("%a\n", v);
  return 0;
}
