// vgicp_host_probe.cpp — the host code of the voxel distribution map's mirror, stand-alone: voxel::pack and the binary
// search over ascending keys (include/nanopcl/registration/vgicp_lookup.hpp).  tests/test_vgicp_restate.py builds it with
// -fsanitize=address,undefined and holds its answers against the restatement's.
//
// stdin, numbers as hexadecimal floats: inv, m, then m keys in ascending order (each as two numbers: the high and the
// low 32 bits), then q, then q points x y z.  stdout per point: the key's high and low 32 bits and the position found
// (m for none).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nanopcl/registration/vgicp_lookup.hpp"

static bool next(double* v) {
  char tok[128];
  if (std::scanf("%127s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

int main() {
  using namespace nanopcl::registration::detail;
  double inv = 0.0, m = 0.0, q = 0.0;
  if (!next(&inv) || !next(&m)) return 2;
  std::vector<uint64_t> keys(static_cast<size_t>(m));
  for (uint64_t& k : keys) {
    double hi = 0.0, lo = 0.0;
    if (!next(&hi) || !next(&lo)) return 2;
    k = (uint64_t(hi) << 32) | uint64_t(lo);
  }
  if (!next(&q)) return 2;
  for (size_t i = 0; i < static_cast<size_t>(q); ++i) {
    double x = 0.0, y = 0.0, z = 0.0;
    if (!next(&x) || !next(&y) || !next(&z)) return 2;
    const uint64_t key = vgicp_pack(float(x), float(y), float(z), float(inv));
    const size_t at = vgicp_find(keys.data(), keys.size(), key);
    std::printf("%a %a %a\n", double(key >> 32), double(key & 0xFFFFFFFFull), double(at));
  }
  return 0;
}
