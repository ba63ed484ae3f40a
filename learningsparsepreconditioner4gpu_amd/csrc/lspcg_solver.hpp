// The PCG solver handle and the host control code that the single-system solver (lspcg_pcg.hip)
// and the batched lockstep solver (lspcg_batch.hip, which runs on a solver of the block-diagonal
// system) share, solve_multi (lspcg_multi.hip) too: the cache of captured iteration graphs, the
// poll loop, the one-workgroup solve's launch, the initial state, the device history buffer and
// the tail of a solve.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "lspcg_factor.hpp"
#include "lspcg_internal.hpp"
#include "lspcg_pcg_kernels.hpp"
#include "lspcg_sell.hpp"
#include "lspcg_spmv.hpp"

#pragma GCC visibility push(hidden)  // internal to the library: nothing here is exported
namespace lspcg {

// Instantiated graphs of `chunk` consecutive iterations, by chunk size.  They hold the kernels'
// arguments by value, so the owner clears them whenever one of those changes (graph_key).
struct IterationGraphs {
  std::map<int, hipGraphExec_t> execs;
  std::map<int, hipGraph_t> defs;
  // The graph of `chunk` iterations; on a miss captured on `st` from `chunk` calls of
  // enqueue_one(), which returns a status code (the capture is ended before an error is returned).
  template <class F>
  int get(hipStream_t st, int chunk, F enqueue_one, hipGraphExec_t* out) {
    auto it = execs.find(chunk);
    if (it != execs.end()) {
      *out = it->second;
      return LSPCG_OK;
    }
    hipGraph_t g = nullptr;
    LSPCG_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = LSPCG_OK;
    for (int i = 0; i < chunk && rc == LSPCG_OK; ++i) rc = enqueue_one();
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) return rc;
    LSPCG_HIP(e);
    hipGraphExec_t ex = nullptr;
    LSPCG_HIP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    execs[chunk] = ex;
    defs[chunk] = g;
    *out = ex;
    return LSPCG_OK;
  }
  template <class F>
  int launch(hipStream_t st, int chunk, F enqueue_one) {  // get + launch on `st`
    hipGraphExec_t ex = nullptr;
    if (int rc = get(st, chunk, enqueue_one, &ex)) return rc;
    LSPCG_HIP(hipGraphLaunch(ex, st));
    return LSPCG_OK;
  }
  void clear() {
    for (auto& kv : execs) (void)hipGraphExecDestroy(kv.second);
    for (auto& kv : defs) (void)hipGraphDestroy(kv.second);
    execs.clear();
    defs.clear();
  }
};

struct MultiWs;  // lspcg_solver_solve_multi's workspace (lspcg_multi.hip)

}  // namespace lspcg

struct lspcg_solver {
  lspcg_ctx* ctx = nullptr;
  const lspcg_mat* A = nullptr;       // the system the loop runs on: A_user, or Ap when reordered
  const lspcg_mat* A_user = nullptr;  // the caller's A
  const lspcg_mat* L = nullptr;       // the caller's L (ext_spai)
  lspcg_mat* LT = nullptr;  // owned (the permuted Lᵀ when reordered)
  // bandwidth-reducing row placement (lspcg_reorder.hip): A, L, Lᵀ permuted with each row's
  // entries in their original order, vectors gathered in / scattered out around the loop
  lspcg::Reorder ro;
  lspcg_mat* Ap = nullptr;   // owned P A Pᵀ
  lspcg_mat* Lp = nullptr;   // owned P L Pᵀ
  lspcg_mat* LTo = nullptr;  // owned Lᵀ in the original numbering (reordered ext_spai; kept for reuse)
  int reorder_mode = -1;     // LSPCG_REORDER: -1 auto, 0 off, 1 always
  bool reorder_ok = false;   // single solves in the compensated order only (not batches, IC, parity)
  int precond = LSPCG_PRECOND_NONE;
  int dtype = LSPCG_F64;
  int64_t n = 0;
  double eps = 0.0;
  hipStream_t stream = nullptr;  // solver-owned (capturable) stream
  void *x = nullptr, *b = nullptr, *r = nullptr, *z = nullptr, *t = nullptr, *p = nullptr, *q = nullptr,
       *d = nullptr;
  bool split = false;   // current ext_spai schedule uses the split reductions (set_spai decides)
  bool allow_split = true;  // LSPCG_SPLIT_REDUCE=0 keeps the last-arriver reductions
  int split_mode = -1;  // -1 auto (by grid size), 1 groups, 2 no groups (LSPCG_SPLIT_REDUCE)
  double* groups = nullptr;  // [GZ: <= 4096 x 2 dots x DD | GQ: <= 4096 x DD]
  int gsz_l = 1, ng_l = 1, gsz_a = 1, ng_a = 1;  // group size / count of the KB and KC launches
  bool split_cg = false;  // CG / Jacobi on the split reductions (UP, KC, UR with the dots of ρ, ‖r‖²)
  int gsz_r = 1, ng_r = 1;  // ... group size / count of that UR launch
  lspcg::KernelTimer* tk = nullptr;  // lspcg_solver_time_kernels: start / end stamps armed for each launch
  int tk_i = 0;
  lspcg::PcgState* S = nullptr;
  lspcg::PcgState* hS = nullptr;  // pinned host mirrors [2] (poll slots)
  double* partials = nullptr;
  unsigned* ticket = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_t0 = nullptr, ev_t1 = nullptr, ev_poll = nullptr, ev_poll2 = nullptr;
  lspcg::IterationGraphs graphs;  // of enqueue_iteration
  // iteration views of A, L, Lᵀ: compact fp32 values when lossless, one shared index
  // structure when the patterns coincide (non-owning copies of the handles + owned buffers)
  lspcg_mat Av, Lv, LTv;
  void* own_A = nullptr;
  void* own_L = nullptr;
  void* own_LT = nullptr;
  int64_t own_A_n = -1, own_L_n = -1, own_LT_n = -1;  // entries of the fp32 copies above (refilled in place)
  int* flag = nullptr;
  // IC(0): factor, its explicit transpose and their sync-free solve plans
  lspcg_mat* icL = nullptr;
  lspcg_mat* icU = nullptr;
  lspcg::TrsvPlan planL, planU;
  // lspcg_solver_update_matrix: the level sets of icL's rows (set_ic's own factor; a given factor
  // does not follow A), and whether a numeric refactorization broke down and left icL unusable
  lspcg::Levels ic_lev;
  bool ic_own = false;
  bool ic_broken = false;
  bool update_failed = false;  // the last lspcg_solver_update_matrix returned an error (its graphs were dropped)
  // SELL-64 copies of the scalar iteration views A (0), L (1), Lᵀ (2) (lspcg_sell.hpp); sp[w]
  // is null where the CSR kernel is used (block size 3, irregular rows, LSPCG_NO_SELL=1)
  bool use_sell = true;
  lspcg::SellPattern spat[3];
  const lspcg::SellPattern* sp[3] = {nullptr, nullptr, nullptr};
  void* sv[3] = {nullptr, nullptr, nullptr};
  int svd[3] = {0, 0, 0};  // storage of sv[w]: LSPCG_F32 / LSPCG_F64
  int64_t svn[3] = {0, 0, 0};  // entries sv[w] was allocated for (an in-place refill must fit them)
  double* dhist = nullptr;  // device residual history (lspcg_solver_solve with res_hist), grown on demand
  double* hhist = nullptr;  // its pinned host mirror (the history's copy is enqueued, not a blocking copy)
  int64_t dhist_cap = 0;
  double* dcoef = nullptr;  // device (ρ_k, π_k) pairs (lspcg_solver_solve_coef with coef), grown on demand
  double* hcoef = nullptr;  // their pinned host mirror
  int64_t dcoef_cap = 0;
  unsigned* hflags = nullptr;  // pinned: the IC triangular solves' timeout flags, copied behind the solve
  int64_t small_n = lspcg::kSmallNDefault;  // largest n solved by k_pcg_small (LSPCG_SMALL_N; 0 disables it; also bounded by
                           // 3 rows per thread at 1024 threads and the LDS of 3 vectors: 2560 in fp64)
  bool small_sell = true;  // k_pcg_small reads the SELL copies (LSPCG_SMALL_SELL=0: the CSR views)
  bool split_ok = false;   // set_spai found SELL views for the split schedule
  bool dia_ok = true;      // SELL-DIA views allowed (a batch of one-workgroup solves turns them off)
  bool same_L_pattern = false;  // set around lspcg_solver_set_spai by a caller whose L is the installed handle with
                                // new values only (lspcg_batch_update): L's and Lᵀ's own SELL patterns are kept
  int dot_order = LSPCG_DOT_COMPENSATED;  // lspcg_solver_set_dot_order
  int dot_threads = 1;
  double* ob_part = nullptr;  // [3 dots x kObMaxThreads chunks] parity-mode chunk totals (k_dot_openblas_item)
  lspcg::MultiWs* multi = nullptr;  // K-wide vectors, states and graphs of solve_multi: allocated on first use
};

namespace lspcg {

// lspcg_multi.hip: drop solve_multi's captured graphs (whenever the solver drops its own: they hold
// the same views, ε and d by value); free its workspace (lspcg_solver_destroy)
void multi_clear_graphs(lspcg_solver* s);
void multi_destroy(lspcg_solver* s);

// lspcg_solver_create with the batch's switches: no SELL-DIA views (a window of one-workgroup
// solves), no reordering (lspcg_pcg.hip)
int solver_create(lspcg_ctx* ctx, const lspcg_mat* A, int precond, bool dia_ok, bool reorder_ok, lspcg_solver** out);

// Everything a captured iteration graph holds by value besides the solver's own fixed buffers: the
// views' arrays (SELL copies or CSR views), their value types, the reduction geometry and ε.  A
// new L whose views land at the same addresses keeps the graphs (build_sell / make_view refill in
// place), so a sample-by-sample loop does not re-capture every chunk size per sample.  The batch's
// graphs (lspcg_batch.hip) are captured on the same views and follow the same key.
struct GraphKey {
  std::vector<int64_t> v;  // pointers, kinds and sizes, in a fixed order
  double eps = 0.0;
  bool operator==(const GraphKey& o) const { return v == o.v && eps == o.eps; }
};
GraphKey graph_key(const lspcg_solver* s);  // lspcg_pcg.hip

// SpMV of iteration view w with the fused prologue / gather / epilogue, SELL when available.
template <typename T, class Gx, class Pro, class Epi>
int launch_it_gx(lspcg_solver* s, int w, Gx gx, Pro pro, Epi epi, hipStream_t st) {
  if (const SellPattern* P = s->sp[w]) {
    if constexpr (sizeof(T) == 8) {
      if (s->svd[w] == LSPCG_F32) return launch_sell<T, float>(*P, s->sv[w], gx, pro, epi, st);
    }
    return launch_sell<T, T>(*P, s->sv[w], gx, pro, epi, st);
  }
  const lspcg_mat* V = w == 0 ? &s->Av : (w == 1 ? &s->Lv : &s->LTv);
  return launch_spmv_gx<T>(V, gx, pro, epi, st);
}

template <typename T, class Pro, class Epi>
int launch_it(lspcg_solver* s, int w, const T* x, Pro pro, Epi epi, hipStream_t st) {
  return launch_it_gx<T>(s, w, GatherVec<T>{x}, pro, epi, st);
}

inline CsrView csr_view(const lspcg_solver* s, int w, const lspcg_mat& M) {
  CsrView v{M.rowptr, M.colind, M.vals, M.storage_dtype() == LSPCG_F32 ? 1 : 0, nullptr, nullptr, nullptr, 0, 0};
  if (const SellPattern* P = s->sp[w]) {
    // (SELL-DIA views are never built for systems this kernel solves: build_sell / lspcg_batch_create)
    if (s->small_sell && s->sv[w] && P->bs == 1 && P->groups > 0 && (P->col_bits == kSellOff16 || P->col_bits == kSellInt32)) {
      v.gp = P->gp;
      v.scol = P->col;
      v.sv = s->sv[w];
      v.sf32 = s->svd[w] == LSPCG_F32 ? 1 : 0;
      v.cmode = P->col_bits == kSellOff16 ? 1 : 0;
    }
  }
  return v;
}

inline size_t esize(int dtype) { return dtype == LSPCG_F32 ? 4 : 8; }

// Rows per thread R and threads TH of k_pcg_small for n rows (a window: its largest system's),
// passed to f as std::integral_constant values.
// n <= 1024: 512 threads, <= 2 rows each (the measured best there); above: 1024 threads, 2-3 rows
// (512 threads x 5 rows measured 20.5-28.2 vs 16.3-21.7 us per iteration)
template <class F>
void dispatch_small(int64_t n, F f) {
  using T512 = std::integral_constant<int, kSmallThreads>;
  using T1024 = std::integral_constant<int, kSmallThreadsBig>;
  if (n <= kSmallThreads) f(std::integral_constant<int, 1>{}, T512{});
  else if (n <= 2 * kSmallThreads) f(std::integral_constant<int, 2>{}, T512{});
  else if (n <= 2 * kSmallThreadsBig) f(std::integral_constant<int, 2>{}, T1024{});
  else f(std::integral_constant<int, 3>{}, T1024{});
}

// k_pcg_small on `grid` systems of solver s's views: the one system of n rows (boff = bn = nullptr),
// or a window's systems at rows boff[k] .. boff[k] + bn[k], the largest of n rows (d: 1 on a
// window's padding rows, which no workgroup owns)
template <typename T>
int launch_pcg_small(int precond, int grid, lspcg_solver* s, int64_t n, PcgState* S, const int32_t* boff,
                     const int32_t* bn, hipStream_t st) {
  const bool spai = precond == LSPCG_PRECOND_EXT_SPAI || precond == LSPCG_PRECOND_EXT_SPAI_SCALED;
  const CsrView A = csr_view(s, 0, s->Av);
  const CsrView L = spai ? csr_view(s, 1, s->Lv) : CsrView{};
  const CsrView LT = spai ? csr_view(s, 2, s->LTv) : CsrView{};
  const size_t lds = 3 * sizeof(T) * size_t(n);
  dispatch_small(n, [&](auto rows, auto threads) {
    auto go = [&](auto pre) {
      constexpr int R = decltype(rows)::value, TH = decltype(threads)::value;
      hipLaunchKernelGGL((k_pcg_small<T, decltype(pre)::value, R, TH>), dim3(unsigned(grid)), dim3(TH), lds, st,
                         int32_t(n), S, A, L, LT, as<T>(s->d), as<T>(s->x), as<T>(s->r), as<T>(s->p), boff, bn);
    };
    switch (precond) {
      case LSPCG_PRECOND_NONE: go(std::integral_constant<int, LSPCG_PRECOND_NONE>{}); break;
      case LSPCG_PRECOND_DIAGONAL: go(std::integral_constant<int, LSPCG_PRECOND_DIAGONAL>{}); break;
      case LSPCG_PRECOND_EXT_SPAI: go(std::integral_constant<int, LSPCG_PRECOND_EXT_SPAI>{}); break;
      default: go(std::integral_constant<int, LSPCG_PRECOND_EXT_SPAI_SCALED>{});
    }
  });
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

// The state a solve starts from (the init launch adds the norms and atol).
inline PcgState initial_state(double rtol, double eps, double* hist, int64_t max_iter, double* coef = nullptr) {
  PcgState init{};
  init.rtol = rtol, init.eps = eps, init.hist = hist, init.coef = coef, init.max_iter = max_iter;
  return init;
}

// What a solve reports from a system's final state.
struct SolveTail {
  int64_t iters;    // a non-finite residual (done == 3) stops early but reports max_iter (pymathprim's count)
  int64_t written;  // history entries 0..fin.iter were written ...
  SolveTail(const PcgState& fin, int64_t max_iter)
      : iters(fin.done == 3 ? max_iter : fin.iter), written(std::min<int64_t>(fin.iter, max_iter) + 1) {}
  void nan_fill(double* hist) const {  // ... so the rest of 0..iters is NaN-filled
    for (int64_t k = written; k <= iters; ++k) hist[k] = NAN;
  }
  int64_t pairs() const { return written - 1; }  // (ρ_k, π_k) of the completed iterations were recorded ...
  void nan_fill_coef(double* coef) const {       // ... so the rest of the `iters` pairs is NaN-filled
    for (int64_t k = 2 * pairs(); k < 2 * iters; ++k) coef[k] = NAN;
  }
};

// Device history buffer of at least `need` entries (grown after the stream has drained: a solve in
// flight may write the old one)
inline int grow_hist(double** buf, int64_t* cap, int64_t need, hipStream_t st) {
  if (need <= *cap) return LSPCG_OK;
  LSPCG_HIP(hipStreamSynchronize(st));
  (void)hipFree(*buf);
  *buf = nullptr;
  *cap = 0;
  LSPCG_HIP(hipMalloc(buf, sizeof(double) * need));
  *cap = need;
  return LSPCG_OK;
}

// iters / status / res_hist / coef (nullable, entries nullable) of ns systems from their final
// states, system k's history at dhist + hoff[k], its recorded pairs at dhist + coff[k]; LSPCG_OK when
// every system converged
inline int report_states(int ns, const PcgState* fin, const int64_t* max_iter, const double* dhist,
                         const int64_t* hoff, int64_t* iters, int32_t* status, double* const* res_hist,
                         const int64_t* coff = nullptr, double* const* coef = nullptr) {
  bool all = true;
  for (int k = 0; k < ns; ++k) {
    const SolveTail tail(fin[k], max_iter[k]);
    iters[k] = tail.iters;
    status[k] = fin[k].done == 1 ? LSPCG_OK : LSPCG_NOT_CONVERGED;
    all = all && fin[k].done == 1;
    if (res_hist && res_hist[k]) {
      LSPCG_HIP(hipMemcpy(res_hist[k], dhist + hoff[k], sizeof(double) * tail.written, hipMemcpyDeviceToHost));
      tail.nan_fill(res_hist[k]);
    }
    if (coef && coef[k]) {
      if (tail.pairs() > 0)
        LSPCG_HIP(hipMemcpy(coef[k], dhist + coff[k], sizeof(double) * 2 * tail.pairs(), hipMemcpyDeviceToHost));
      tail.nan_fill_coef(coef[k]);
    }
  }
  return all ? LSPCG_OK : LSPCG_NOT_CONVERGED;
}

// The host's view of ns >= 1 device states while their loop runs: two pinned poll slots, each a
// copy of all states plus an event, enqueued behind everything launched so far.
struct StatePoll {
  int ns;
  PcgState* dS;       // device states [ns]
  PcgState* hS;       // pinned mirrors [2 * ns]: the two poll slots
  hipEvent_t ev[2];
  hipStream_t st;
  std::unique_lock<std::mutex>& sub;  // the submission lock, held by the solve
  int64_t queued[2] = {0, 0};         // iterations launched after each outstanding poll
  int head = 0, npend = 0;            // oldest outstanding poll slot, number outstanding (<= 2)
  int64_t launched = 0, nlaunch = 0;  // iterations / graphs enqueued (LSPCG_SOLVE_PROFILE)

  // every host wait of the loop: the submission lock is released around it, and only here
  hipError_t wait(hipEvent_t e) {
    sub.unlock();
    const hipError_t r = hipEventSynchronize(e);
    sub.lock();
    return r;
  }
  int post() {  // a state copy + event after everything enqueued so far
    const int k = (head + npend) & 1;
    LSPCG_HIP(hipMemcpyAsync(hS + k * ns, dS, sizeof(PcgState) * ns, hipMemcpyDeviceToHost, st));
    LSPCG_HIP(hipEventRecord(ev[k], st));
    queued[k] = 0;
    ++npend;
    return LSPCG_OK;
  }
  // waits for the oldest outstanding poll: its states into cur[ns], the iterations launched after it
  int take(PcgState* cur, int64_t* inflight = nullptr) {
    LSPCG_HIP(wait(ev[head]));
    std::copy(hS + head * ns, hS + (head + 1) * ns, cur);
    if (inflight) *inflight = queued[head];
    head ^= 1;
    --npend;
    return LSPCG_OK;
  }

  // Poll loop, one chunk ahead: the states copied after chunk k are read while chunk k+1 runs, so
  // the GPU does not idle through the host round trip.  Runs while any system runs; chunk sizes
  // follow the slowest system's observed residual decay minus the iterations already in flight, so
  // that at most a few early-exit launches trail the converged iteration (every launch is
  // predicated on the device `done` flag).  launch_chunk(c) launches the graph of c <= max_chunk
  // iterations and returns a status code; cur[ns] receives the final states (later, early-exit
  // launches leave them unchanged).
  template <class L>
  int run(const int64_t* max_iter, int max_chunk, L launch_chunk, PcgState* cur) {
    auto launch = [&](int c) -> int {
      if (int r = launch_chunk(c)) return r;
      launched += c;
      ++nlaunch;
      for (int j = 0; j < npend; ++j) queued[(head + j) & 1] += c;
      return post();
    };
    int chunk = std::min(4, max_chunk);
    int rc = post();
    if (!rc) rc = launch(chunk);
    if (rc) return rc;
    std::vector<int64_t> last_it(ns, 0);
    std::vector<double> last_rr(ns, -1.0);
    for (;;) {
      int64_t inflight = 0;
      if ((rc = take(cur, &inflight))) return rc;
      int64_t rem = 0;  // largest predicted remaining count over the running systems
      bool unknown = false, running = false;
      for (int k = 0; k < ns; ++k) {
        const PcgState& c = cur[k];
        if (c.done) continue;  // the top-of-loop test sets done (convergence, max_iter or a non-finite residual)
        running = true;
        int64_t rk = -1;  // predicted iterations still needed after this state
        if (last_rr[k] > 0 && c.iter > last_it[k] && c.rr > 0 && c.rr < last_rr[k]) {
          const double rate = std::log(c.rr / last_rr[k]) / double(c.iter - last_it[k]);  // < 0
          const double need = std::log((c.atol * c.atol) / c.rr) / rate;
          rk = need > 0 ? int64_t(std::ceil(need)) : 1;
          rk = std::max<int64_t>(1, std::min<int64_t>(rk, max_iter[k] - c.iter));
        }
        if (c.iter > last_it[k] || last_rr[k] < 0) {
          last_it[k] = c.iter;
          last_rr[k] = c.rr;
        }
        if (rk < 0) unknown = true;
        else rem = std::max(rem, rk);
      }
      if (!running) break;
      if (unknown) rem = -1;
      if (rem >= 0) {
        const int64_t more = rem - inflight;
        if (more <= 0) {
          if (npend == 0) rc = launch(1);  // predicted to converge in flight; nothing in flight
          if (rc) return rc;
          continue;
        }
        int c = 1;
        while (c * 2 <= more && c < max_chunk) c *= 2;
        chunk = c;
      } else {
        chunk = std::min(max_chunk, chunk * 2);
      }
      rc = launch(std::min(chunk, max_chunk));
      if (rc) return rc;
    }
    return LSPCG_OK;
  }
};

}  // namespace lspcg
#pragma GCC visibility pop
