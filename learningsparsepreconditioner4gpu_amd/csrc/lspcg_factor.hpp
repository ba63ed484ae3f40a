// Level-scheduled sparse factorizations / triangular solves shared by lspcg_factor.hip and the
// PCG solver (lspcg_pcg.hip).  See lspcg_factor.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "lspcg.h"

namespace lspcg {

// Rows grouped by dependency level: rows order[hptr[l] .. hptr[l+1]) form level l (ascending row
// index inside a level); hptr (host) sizes the per-level launches of the factorizations.
struct Levels {
  int nlev = 0;
  int32_t* order = nullptr;
  std::vector<int32_t> hptr;
  void release();
  Levels() = default;
  Levels(const Levels&) = delete;
  Levels& operator=(const Levels&) = delete;
  ~Levels() { release(); }
};

// lower: row i depends on the columns j < i of its row; upper: on the columns j > i.
int build_levels(lspcg_ctx* ctx, int64_t n, const int32_t* rp, const int32_t* ci, bool lower, Levels* out);

// What the sync-free solve with one triangular factor reads (lspcg_factor.hip k_trsv_syncfree).
struct TrsvPlan {
  // the level order with every level padded to whole wave64s (-1 = no row), so no wave holds two
  // rows of which one waits for the other; npad positions
  int32_t* pad = nullptr;
  int64_t npad = 0;
  unsigned* head = nullptr;  // head[0] = the launch's block dequeue counter, head[1] = timeout flag
  // the factor's column-scaled values sv_p = v_p / d_col and per row inv = 1 / d, c = d inv
  // (spsolve_triangular's scaling)
  void* sv = nullptr;
  void* inv = nullptr;
  void* c = nullptr;
  int cus = 0;  // the device's CU count (the resident grid's bound), queried when the plan is built
  void release();
};

// levels of T, their padded order, the counter words and T's scaled values (replaces *out)
int trsv_plan_build(const lspcg_mat* T, bool lower, TrsvPlan* out);
// New values in T, same pattern: sv / inv / c recomputed in place (enqueued, not waited for).  The
// levels, the padded order and the counter words depend on the pattern alone and are kept.
int trsv_plan_refill(const lspcg_mat* T, bool lower, const TrsvPlan& plan);
// x = T⁻¹ b in scipy spsolve_triangular's arithmetic (lower: diagonal stored last in each row,
// upper: first); `done` (nullable) is the solver's device done flag -- every launch returns at
// once when it is set.  Counter reset + fill + one sync-free launch (rows wait for their
// dependencies' values) + the diagonal scaling: three kernel launches, no memset or copy node.
int enqueue_trsv(const lspcg_mat* T, const TrsvPlan& plan, bool lower, const void* b, void* x, const int32_t* done,
                 hipStream_t st);
constexpr int kTrsvLaunches = 3;  // graph nodes one enqueue_trsv adds
// LSPCG_ERR_HIP (and clears the flag) when a sync-free solve with this plan timed out
int trsv_check_timeout(const TrsvPlan& plan, hipStream_t st);
// levels (nullable) <- the level sets of L's rows, for ic0_numeric
int ic0_factor(const lspcg_mat* A, lspcg_mat** L, Levels* levels = nullptr);
// Numeric-only IC(0): L (an ic0_factor result for a matrix of A's pattern) <- the factor of A's
// current values, with ic0_factor's kernels in its order (the same bits).  On LSPCG_ERR_BREAKDOWN
// L holds no usable factor.
int ic0_numeric(const lspcg_mat* A, lspcg_mat* L, const Levels& levels);
int ainv0_factor(const lspcg_mat* A, lspcg_mat** L);

}  // namespace lspcg
