// The scalar recurrence of scipy's cg (iterative.py:359-418), once: the loop's state and every
// transition of it, as functions on VALUES.  Every schedule of every solver -- the single-system
// loops and the one-workgroup solve (lspcg_pcg_kernels.hpp), the lockstep batches (lspcg_batch.hip),
// the K-wide epilogues of solve_multi (lspcg_multi.hip), the partitioned solve's device recurrence
// (lspcg_part.hip, test and square root) -- calls these, so they cannot drift apart bit by bit.
// The callers load the state fields they need into registers first (all of them before the first
// store: a store may alias a later load and would order it behind itself, one more round trip);
// the functions only compute and store.
#pragma once

#include "lspcg_internal.hpp"

namespace lspcg {

struct PcgState {
  double bb;        // ‖b‖²
  double rr;        // ‖r_k‖² (rounded to T)
  double rho;       // ρ_k = r_k·z_k (rounded to T)
  double rho_prev;  // ρ_{k-1}
  double pq;        // π_k = p_k·q_k (rounded to T)
  double alpha;     // α_k = ρ_k/π_k computed in T
  double atol;      // rtol·‖b‖
  double rtol;
  double eps;       // ε of ext_spai
  double* hist;     // ‖r_k‖ history (nullable)
  double* coef;     // (ρ_k, π_k) of every completed iteration, the CG-Lanczos coefficients (nullable, 16-B aligned)
  int64_t iter;     // completed iterations
  int64_t max_iter;
  int32_t done;     // 0 running, 1 converged, 2 max_iter reached, 3 non-finite residual
  int32_t pad;
  double rho_k;     // split schedule: ρ_k as UP summed it from KB's groups, read by UR (same bits)
};

template <typename T>
__device__ __forceinline__ T tsqrt(T v) { return sqrt(v); }

// ‖r‖ from ‖r‖² as scipy's np.linalg.norm gives it in T: the tested norm and the history entry
template <typename T>
__device__ __forceinline__ double res_norm(double rr) { return double(tsqrt<T>(T(rr))); }

// Top-of-iteration test of scipy's loop, `for iteration in range(maxiter): if norm(r) < atol`, at
// iteration k with ‖r_k‖² = rr: the `done` code (0: the iteration runs).
template <typename T>
__device__ __forceinline__ int loop_test(int64_t k, int64_t max_iter, double rr, double atol) {
  int code = 0;
  if (k >= max_iter) {
    code = 2;
  } else {
    const double rn = res_norm<T>(rr);
    if (rn < atol) code = 1;
    else if (!(rn == rn) || rn == INFINITY) code = 3;
  }
  return code;
}

// init: the state from the sums ‖r_0‖², ‖b‖² and ρ_0 = r_0·z_0 (without a preconditioning step in
// the init launch the caller passes ‖r_0‖² again); done = 1 where ‖b‖ = 0.  TEST: also iteration
// 0's top-of-loop test, for schedules whose first launch of an iteration does not run it.
template <typename T, bool TEST = false>
__device__ __forceinline__ void init_state(PcgState* St, double rtol, double* hist, double rr_sum, double bb_sum,
                                           double rho_sum, int64_t max_iter = 0) {
  const double rr = round_to<T>(rr_sum), bb = round_to<T>(bb_sum);
  const double bn = res_norm<T>(bb);
  const double atol = fmax(0.0, rtol * bn);
  St->rr = rr;
  St->bb = bb;
  St->atol = atol;
  St->rho = round_to<T>(rho_sum);
  St->alpha = 0.0;
  St->iter = 0;
  St->done = (bn == 0.0) ? 1 : (TEST ? loop_test<T>(0, max_iter, rr, atol) : 0);
  if (hist) hist[0] = res_norm<T>(rr);
}

// ‖r_k‖² (already rounded) and its history entry for k > 0; ‖r_0‖² and entry 0 are the init's
template <typename T>
__device__ __forceinline__ void keep_rr(PcgState* St, int64_t k, double* hist, double rr) {
  if (k > 0) {
    St->rr = rr;
    if (hist) hist[k] = res_norm<T>(rr);
  }
}

// KB's keep: ρ_{k-1} <- ρ (rho_old), ρ_k and ‖r_k‖² from the sums.  Returns the rounded ‖r_k‖² sum
// (for k = 0 the caller tests the init's instead).
template <typename T>
__device__ __forceinline__ double keep_z(PcgState* St, int64_t k, double rho_old, double* hist, double rho_sum,
                                         double rr_sum) {
  const double rr = round_to<T>(rr_sum);
  St->rho_prev = rho_old;
  St->rho = round_to<T>(rho_sum);
  keep_rr<T>(St, k, hist, rr);
  return rr;
}

// The pair (ρ_k, π_k) of iteration k as the recurrence uses it -- the rounded values that give α_k --
// in one 16-byte store; nothing without a buffer.
__device__ __forceinline__ void keep_coef(double* coef, int64_t k, double rho, double pq) {
  if (coef) *reinterpret_cast<double2*>(coef + 2 * k) = make_double2(rho, pq);
}

// KC's keep: π_k, α_k = ρ_k/π_k in T, the recorded pair and (INC: this launch completes iteration k)
// the count
template <typename T, bool INC>
__device__ __forceinline__ void keep_q(PcgState* St, int64_t k, double* coef, double rho, double pq_sum) {
  const double pq = round_to<T>(pq_sum);
  St->pq = pq;
  St->alpha = double(T(rho) / T(pq));
  keep_coef(coef, k, rho, pq);
  if constexpr (INC) St->iter = k + 1;
}

// UR's dot epilogue: ‖r_{k+1}‖² and history entry `it` = k + 1; RHO (no preconditioner, Jacobi):
// also ρ_k -> ρ_{k-1} and ρ_{k+1} from its sum (the caller passes ‖r‖²'s without a preconditioner).
// Returns the rounded ‖r_{k+1}‖².
template <typename T, bool RHO>
__device__ __forceinline__ double keep_r(PcgState* St, int64_t it, double rho_old, double* hist, double rr_sum,
                                         double rho_sum) {
  const double rr = round_to<T>(rr_sum);
  St->rr = rr;
  if constexpr (RHO) {
    St->rho_prev = rho_old;
    St->rho = round_to<T>(rho_sum);
  }
  if (hist) hist[it] = res_norm<T>(rr);
  return rr;
}

// the consumer-summing UR's commit of a finished iteration, iter - 1, with its recorded pair (the
// one-workgroup solve commits once, after its loop, and records inside it: coef = nullptr here)
template <typename T>
__device__ __forceinline__ void commit_step(PcgState* St, double* coef, double rho_prev, double rho, double pq,
                                            T alpha, int64_t iter) {
  keep_coef(coef, iter - 1, rho, pq);
  St->rho_prev = rho_prev;
  St->rho = rho;
  St->pq = pq;
  St->alpha = double(alpha);
  St->iter = iter;
}

}  // namespace lspcg
