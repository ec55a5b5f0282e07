// Host build of the exact quotients of scavislam_amd/csrc/devutil.h (rcp_rn, div_rn and the guarded forms the refinement tail and gate.h divide with).
// Built as a shared library by tests/test_quotient_cpu.py with -ffp-contract=off and driven from NumPy: every function below works on arrays and returns how
// many elements MISSED (the first miss in *first), so the comparison with the compiler's own a / b happens here, on the very doubles, bit for bit.
#include <stdint.h>
#include <string.h>

#include "../../scavislam_amd/csrc/devutil.h"

namespace {
inline uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
inline bool same(double x, double y) { return bits(x) == bits(y) || (x != x && y != y); }      // NaN payloads aside
inline double plain_div(double a, double b) { volatile double va = a, vb = b; return va / vb; }
}  // namespace

extern "C" {
// div_rn(a, b, r) with r = the correctly rounded reciprocal (the host's 1 / b) against a / b
long svs_host_div_rn_exact_rcp(const double *a, const double *b, long n, long *first) {
  long miss = 0;
  for (long i = 0; i < n; ++i)
    if (!same(div_rn(a[i], b[i], plain_div(1.0, b[i])), plain_div(a[i], b[i])) && miss++ == 0) *first = i;
  return miss;
}
// two Newton steps from the 24-bit seed against the correctly rounded reciprocal; out (optional): rcp_rn's values
long svs_host_rcp_rn(const double *b, long n, long *first, double *out) {
  long miss = 0;
  for (long i = 0; i < n; ++i) {
    const double r = rcp_rn(b[i]);
    if (out) out[i] = r;
    if (!same(r, plain_div(1.0, b[i])) && miss++ == 0) *first = i;
  }
  return miss;
}
// the seed the host build stands in for v_rcp_f64 with: relative error of the worst element (must be a 24-bit seed: <= 2^-23)
double svs_host_rcp_seed_error(const double *b, long n) {
  double worst = 0;
  for (long i = 0; i < n; ++i) {
    const double e = fabs(rcp_seed(b[i]) * b[i] - 1.0);
    if (e > worst) worst = e;
  }
  return worst;
}
// rcp_rn_checked: wherever it says ok the reciprocal must be the correctly rounded one; *n_ok = how many it accepted
long svs_host_rcp_checked(const double *b, long n, long *first, long *n_ok) {
  long miss = 0;
  *n_ok = 0;
  for (long i = 0; i < n; ++i) {
    bool ok;
    const double r = rcp_rn_checked(b[i], ok);
    *n_ok += ok;
    if (ok && !same(r, plain_div(1.0, b[i])) && miss++ == 0) *first = i;
  }
  return miss;
}
// the guarded forms (one quotient; three quotients by one denominator, as the clouds and the residual use it) against a / b; *n_fast = quotients from the short path
long svs_host_div_guarded(const double *a, const double *b, long n, long *first, long *n_fast) {
  long miss = 0;
  *n_fast = 0;
  for (long i = 0; i < n; ++i) {
    bool ok;
    const double r = rcp_rn_checked(b[i], ok);
    *n_fast += ok && quot_exp_ok(a[i]);
    const double num[3] = {a[i], a[(i + 1) % n], a[(i + 2) % n]};
    double q3[3];
    div_rn_guarded(num, b[i], q3);
    bool good = same(div_rn_guarded(a[i], b[i], r, ok), plain_div(a[i], b[i]));
    for (int k = 0; k < 3; ++k) good = good && same(q3[k], plain_div(num[k], b[i]));
    if (!good && miss++ == 0) *first = i;
  }
  return miss;
}
int svs_host_quot_exp_ok(double x) { return quot_exp_ok(x) ? 1 : 0; }
}
