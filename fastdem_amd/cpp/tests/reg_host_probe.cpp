// reg_host_probe.cpp — the host algebra of cloud registration (csrc/fdm_register_host.hpp) as a stand-alone CPU program:
// no device, no library.  Reads an operation and its numbers (hexadecimal floats) from standard input and prints the
// result the same way.  tests/test_reg_restate.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and holds
// it to the NumPy restatement.
//   1 H[21] b[6] T[16]      -> delta[6], se3Exp(delta) * T [16]          (T column-major)
//   2 xi[6]                 -> se3Exp(xi) [16]
//   3 delta[6] prev curr translation_eps rotation_eps relative_error_eps -> converged
//   4 n H[21]               -> has_covariance, covariance[36]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fdm_register_host.hpp"

using namespace fdm::reg;

int main() {
  std::vector<double> in;
  char tok[128];
  while (std::scanf("%127s", tok) == 1) in.push_back(std::strtod(tok, nullptr));
  if (in.empty()) return 2;
  const int op = int(in[0]);
  const double* a = in.data() + 1;
  const size_t n = in.size() - 1;
  std::vector<double> out;
  if (op == 1 && n == 43) {
    double delta[6];
    compute_delta(full_hessian(a), a + 21, kLambda, delta);
    double m[16];
    rigid_to_colmajor(rigid_mul(se3_exp(delta), rigid_from_colmajor(a + 27)), m);
    out.assign(delta, delta + 6);
    out.insert(out.end(), m, m + 16);
  } else if (op == 2 && n == 6) {
    double m[16];
    rigid_to_colmajor(se3_exp(a), m);
    out.assign(m, m + 16);
  } else if (op == 3 && n == 11) {
    Criteria c;
    c.translation_eps = a[8];
    c.rotation_eps = a[9];
    c.relative_error_eps = a[10];
    out.push_back(c.converged(a, a[6], a[7]) ? 1.0 : 0.0);
  } else if (op == 4 && n == 22) {
    double cov[36] = {};
    const bool has = covariance_of(full_hessian(a + 1), uint64_t(a[0]), cov);
    out.push_back(has ? 1.0 : 0.0);
    out.insert(out.end(), cov, cov + 36);
  } else {
    return 2;
  }
  for (double v : out) std::printf("%a\n", v);
  return 0;
}
