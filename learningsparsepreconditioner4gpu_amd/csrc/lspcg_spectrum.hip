// Spectrum of the preconditioned system from the PCG loop's scalars -- host code only, no device
// call: the library's two functions behind spectrum.py (the reference's cond.py takes a dense
// eigvalsh of M A on the host, cond.py:24-33; this takes the extremes from the solve itself).
//
// CG is the Lanczos process on M⁻¹A in the M-inner product.  With α_k = ρ_k/π_k and
// β_k = ρ_k/ρ_{k-1} the Lanczos tridiagonal of the first m iterations is (Saad, Iterative Methods
// for Sparse Linear Systems, 2nd ed., §6.7.3; Golub & Van Loan, Matrix Computations, §11.3)
//   T[k][k]   = 1/α_k + β_k/α_{k-1}          (β_0/α_{-1} = 0)
//   T[k][k+1] = sqrt(β_{k+1}) / α_k
// and its extreme eigenvalues converge to those of M⁻¹A as the solve converges.  The recorded pairs
// (lspcg_solver_solve_coef) are exactly the ρ_k, π_k the loop divided, so T_m describes the run that
// happened, rounding included.
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "lspcg_internal.hpp"

namespace {

// number of eigenvalues of the tridiagonal below x: the negative pivots of the LDLᵀ of T - xI
// (a pivot smaller than pivmin in magnitude is taken as -pivmin, LAPACK dlaebz's rule)
int64_t sturm_count(int64_t m, const double* d, const double* e, double x, double pivmin) {
  int64_t cnt = 0;
  double q = d[0] - x;
  if (std::fabs(q) < pivmin) q = -pivmin;
  if (q < 0) ++cnt;
  for (int64_t i = 1; i < m; ++i) {
    q = d[i] - x - e[i - 1] * e[i - 1] / q;
    if (std::fabs(q) < pivmin) q = -pivmin;
    if (q < 0) ++cnt;
  }
  return cnt;
}

// the point where the count passes from < want to >= want, between lo (count < want) and hi
// (count >= want), bisected until the two are adjacent doubles
double bisect(int64_t m, const double* d, const double* e, double lo, double hi, int64_t want, double pivmin) {
  for (int it = 0; it < 4096; ++it) {
    const double mid = lo + (hi - lo) / 2;
    if (!(mid > lo && mid < hi)) break;
    if (sturm_count(m, d, e, mid, pivmin) >= want) hi = mid;
    else lo = mid;
  }
  return lo + (hi - lo) / 2;
}

}  // namespace

extern "C" {

int lspcg_cg_lanczos(int64_t m, const double* coef, double* diag, double* off) {
  LSPCG_CHECK(m >= 1 && coef && diag && (off || m == 1), LSPCG_ERR_ARG, "cg_lanczos: m < 1 or NULL argument");
  for (int64_t k = 0; k < m; ++k) {
    const double rho = coef[2 * k], pq = coef[2 * k + 1];
    LSPCG_CHECK(rho > 0 && pq > 0 && std::isfinite(rho) && std::isfinite(pq), LSPCG_ERR_ARG,
                "cg_lanczos: rho or pi of iteration " + std::to_string(k) +
                    " is not positive and finite (breakdown, or an operator that is not SPD)");
  }
  for (int64_t k = 0; k < m; ++k) {
    const double rho = coef[2 * k], pq = coef[2 * k + 1];
    double t = pq / rho;  // 1/α_k
    if (k > 0) t += (rho / coef[2 * k - 2]) * (coef[2 * k - 1] / coef[2 * k - 2]);  // β_k/α_{k-1}
    diag[k] = t;
    if (k + 1 < m) off[k] = std::sqrt(coef[2 * k + 2] / rho) * (pq / rho);
    LSPCG_CHECK(std::isfinite(diag[k]) && (k + 1 >= m || std::isfinite(off[k])), LSPCG_ERR_ARG,
                "cg_lanczos: the coefficients of iteration " + std::to_string(k) + " overflow");
  }
  return LSPCG_OK;
}

int lspcg_tridiag_extremes(int64_t m, const double* diag, const double* off, double* lmin, double* lmax) {
  LSPCG_CHECK(m >= 1 && diag && (off || m == 1) && lmin && lmax, LSPCG_ERR_ARG,
              "tridiag_extremes: m < 1 or NULL argument");
  double glo = INFINITY, ghi = -INFINITY, emax = 0.0;
  for (int64_t i = 0; i < m; ++i) {
    const double a = i > 0 ? std::fabs(off[i - 1]) : 0.0, b = i + 1 < m ? std::fabs(off[i]) : 0.0;
    LSPCG_CHECK(std::isfinite(diag[i]) && std::isfinite(a) && std::isfinite(b), LSPCG_ERR_ARG,
                "tridiag_extremes: non-finite entry in row " + std::to_string(i));
    glo = std::fmin(glo, diag[i] - a - b);
    ghi = std::fmax(ghi, diag[i] + a + b);
    emax = std::fmax(emax, b);
  }
  if (m == 1) {
    *lmin = *lmax = diag[0];
    return LSPCG_OK;
  }
  const double eps = std::numeric_limits<double>::epsilon();
  const double pivmin = std::numeric_limits<double>::min() * std::fmax(1.0, emax * emax);
  // the Gershgorin interval, widened by the count's own rounding so that both ends are certain
  const double tn = std::fmax(std::fabs(glo), std::fabs(ghi));
  const double lo = glo - 2.0 * tn * eps * double(m) - 2.0 * pivmin;
  const double hi = ghi + 2.0 * tn * eps * double(m) + 2.0 * pivmin;
  LSPCG_CHECK(std::isfinite(lo) && std::isfinite(hi), LSPCG_ERR_ARG, "tridiag_extremes: the Gershgorin interval overflows");
  *lmin = bisect(m, diag, off, lo, hi, 1, pivmin);
  *lmax = bisect(m, diag, off, lo, hi, m, pivmin);
  return LSPCG_OK;
}

}  // extern "C"
