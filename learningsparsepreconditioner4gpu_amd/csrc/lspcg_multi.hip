// ==== several right-hand sides of ONE system in one lockstep PCG (lspcg_solver_solve_multi;
// DESIGN.md §6 "Several right-hand sides") ====================================================
// nrhs <= 8 columns share every launch of the ext_spai iteration and every matrix load: the
// working vectors are interleaved [n][Kp] (Kp = 2, 4, 8 >= nrhs, the surplus columns zero), a
// lane of the K-vector SpMV kernels (lspcg_sell.hpp) loads each slot of its row once and applies
// it to the Kp entries of the gathered row, and each column keeps scipy cg's recurrence with its
// own PcgState: scalars, top-of-loop test, iteration count, history, done code.  Five launches per
// iteration, the last-arriver schedule of lspcg_pcg.hip with K-wide epilogues:
//   KA  T = Lᵀ R                                                        [SpMM Lᵀ]
//   KB  Z = L T + ε R ; per column ρ_k = r·z, ‖r_k‖²                      [SpMM L, 2 Kp dots]
//   UP  per column: top-of-loop test ; x += α_{k-1} p_{k-1} ; p_k = p_{k-1}β + z
//   KD  Q = A P ; per column π_k = p·q, α_k = ρ_k/π_k, iteration k+1     [SpMM A, Kp dots]
//   UR  per column: r_{k+1} = r_k - α_k q
// One last-arriver reduction per reducing launch (grid_reduce_wide, lspcg_internal.hpp) carries all columns' dots; its
// fin updates every running column's state.  A finished column is frozen: fin skips it, UP and UR keep its x, p and r (a
// select per entry), and what KA / KB / KD compute in its lanes is never read.  Its deferred
// x += α p is applied once, by the launch that unpacks X.  A workgroup leaves when every column is
// done, so the host replays captured chunks and polls as it does for one system (StatePoll).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "lspcg_pcg_kernels.hpp"
#include "lspcg_solver.hpp"

using namespace lspcg;

namespace lspcg {

constexpr int kMultiMax = 8;  // right-hand sides per solve

template <int K>
struct ProAllDone {
  const PcgState* S;
  __device__ __forceinline__ bool exit() const {
    bool all = true;
#pragma unroll
    for (int k = 0; k < K; ++k) all = all && S[k].done != 0;
    return all;
  }
};

// KA: T = Lᵀ R (scaled: / d), EpiT per column
template <typename T, int K, bool SCALED>
struct EpiTK {
  static constexpr int NDOT = 0;
  T* t;
  const T* d;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, const T (&s)[K], DD*) const {
    T o[K];
    T di = T(1);
    if constexpr (SCALED) di = gld(d + i);
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = SCALED ? s[k] / di : s[k];
    RowK<T, K>::store(t + i * K, o);
  }
  __device__ __forceinline__ void fin(const double*) const {}
};

// KB: Z = L T + ε R (scaled: + (ε R)/d); dots [2k] = ρ, [2k + 1] = ‖r‖² of column k; KB's keep per
// running column
template <typename T, int K, bool SCALED>
struct EpiZK {
  static constexpr int NDOT = 2 * K;
  static constexpr bool CUSTOM_FINISH = true;  // grid_reduce_wide
  T* z;
  const T* r;
  const T* d;
  T eps;
  PcgState* S;
  double* partials;
  unsigned* ticket;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, const T (&s)[K], DD* dots) const {
    T ri[K], zi[K];
    RowK<T, K>::load(r + i * K, ri);
    T di = T(1);
    if constexpr (SCALED) di = gld(d + i);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if constexpr (SCALED) zi[k] = s[k] + (eps * ri[k]) / di;
      else zi[k] = s[k] + eps * ri[k];
      dd_fma(dots[2 * k], double(ri[k]), double(zi[k]));
      dd_fma(dots[2 * k + 1], double(ri[k]), double(ri[k]));
    }
    RowK<T, K>::store(z + i * K, zi);
  }
  __device__ __forceinline__ void finish(DD (&dd)[NDOT]) const {
    grid_reduce_wide<NDOT>(dd, partials, ticket, [&](const double* v) { fin(v); });
  }
  // (every column's fields are loaded before the first store: the stores may alias the loads, and
  // one thread would otherwise pay a memory round trip per column)
  __device__ __forceinline__ void fin(const double* v) const {
    int32_t done[K];
    int64_t it[K];
    double rho[K];
    double* hist[K];
#pragma unroll
    for (int k = 0; k < K; ++k) done[k] = S[k].done, it[k] = S[k].iter, rho[k] = S[k].rho, hist[k] = S[k].hist;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (!done[k]) keep_z<T>(S + k, it[k], rho[k], hist[k], v[2 * k], v[2 * k + 1]);
  }
};

// KD: Q = A P; dot [k] = π of column k; KC's keep and the count per running column
template <typename T, int K>
struct EpiQK {
  static constexpr int NDOT = K;
  static constexpr bool CUSTOM_FINISH = true;  // grid_reduce_wide
  T* q;
  const T* p;
  PcgState* S;
  double* partials;
  unsigned* ticket;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, const T (&s)[K], DD* dots) const {
    T pi[K];
    RowK<T, K>::load(p + i * K, pi);
    RowK<T, K>::store(q + i * K, s);
#pragma unroll
    for (int k = 0; k < K; ++k) dd_fma(dots[k], double(pi[k]), double(s[k]));
  }
  __device__ __forceinline__ void finish(DD (&dd)[NDOT]) const {
    grid_reduce_wide<NDOT>(dd, partials, ticket, [&](const double* v) { fin(v); });
  }
  __device__ __forceinline__ void fin(const double* v) const {
    int32_t done[K];
    int64_t it[K];
    double rho[K];
#pragma unroll
    for (int k = 0; k < K; ++k) done[k] = S[k].done, it[k] = S[k].iter, rho[k] = S[k].rho;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (!done[k]) keep_q<T, true>(S + k, it[k], nullptr, rho[k], v[k]);
  }
};

// init: R_0 = B - A X0; dots [2k] = ‖r_0‖², [2k + 1] = ‖b‖² of column k; the initial state per column
// (a zero column -- the padding columns among them -- is done here)
template <typename T, int K>
struct EpiResidK {
  static constexpr int NDOT = 2 * K;
  static constexpr bool CUSTOM_FINISH = true;  // grid_reduce_wide
  T* r;
  const T* b;
  PcgState* S;
  double* partials;
  unsigned* ticket;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, const T (&s)[K], DD* dots) const {
    T bi[K], ri[K];
    RowK<T, K>::load(b + i * K, bi);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ri[k] = bi[k] - s[k];
      dd_fma(dots[2 * k], double(ri[k]), double(ri[k]));
      dd_fma(dots[2 * k + 1], double(bi[k]), double(bi[k]));
    }
    RowK<T, K>::store(r + i * K, ri);
  }
  __device__ __forceinline__ void finish(DD (&dd)[NDOT]) const {
    grid_reduce_wide<NDOT>(dd, partials, ticket, [&](const double* v) { fin(v); });
  }
  __device__ __forceinline__ void fin(const double* v) const {
    double rtol[K];
    double* hist[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rtol[k] = S[k].rtol, hist[k] = S[k].hist;
#pragma unroll
    for (int k = 0; k < K; ++k) init_state<T>(S + k, rtol[k], hist[k], v[2 * k], v[2 * k + 1], v[2 * k]);
  }
};

// UP over the interleaved vectors, 16-B vectors as k_update_p.  A lane's vectors j, j + stride, ...
// all hold the same columns (the stride is a multiple of 256 vectors), so its per-entry scalars are
// selected once, column by column (an indexed register array would go to scratch).  The top-of-loop
// test per column; workgroup 0's thread 0 writes the done codes.
template <typename T, int K>
__global__ void __launch_bounds__(kThreads) k_multi_update_p(int64_t nv, PcgState* S, const T* __restrict__ z,
                                                             T* __restrict__ p, T* __restrict__ x) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  const int64_t jt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  T aw[W], bw[W];
  bool lw[W], fw[W];
#pragma unroll
  for (int w = 0; w < W; ++w) aw[w] = bw[w] = T(0), lw[w] = fw[w] = false;
  // every column's state is loaded before the done codes are stored (the stores may alias the loads)
  int32_t done[K];
  int64_t it[K], mi[K];
  double rr[K], atol[K], rho[K], rho_prev[K], alpha_prev[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const PcgState* St = S + k;
    done[k] = St->done, it[k] = St->iter, mi[k] = St->max_iter;
    rr[k] = St->rr, atol[k] = St->atol, rho[k] = St->rho, rho_prev[k] = St->rho_prev, alpha_prev[k] = St->alpha;
  }
  bool any = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int code = 0;
    if (!done[k]) {
      code = loop_test<T>(it[k], mi[k], rr[k], atol[k]);
      if (code && blockIdx.x == 0 && threadIdx.x == 0) S[k].done = code;
    }
    const bool live = !done[k] && !code;
    any = any || live;
    const bool first = it[k] == 0;
    const T beta = first ? T(0) : T(rho[k]) / T(rho_prev[k]);
    const T alpha = T(alpha_prev[k]);
#pragma unroll
    for (int w = 0; w < W; ++w) {  // the entries of this lane's vectors that belong to column k
      const bool mine = int((jt * W + w) & (K - 1)) == k;
      aw[w] = mine ? alpha : aw[w];
      bw[w] = mine ? beta : bw[w];
      lw[w] = mine ? live : lw[w];
      fw[w] = mine ? first : fw[w];
    }
  }
  if (!any) return;
  for (int64_t j0 = jt; j0 < nv; j0 += ts * kElemUnroll) {
    V zz[kElemUnroll], pp[kElemUnroll], xx[kElemUnroll];
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        zz[u] = reinterpret_cast<const V*>(z)[j];
        pp[u] = reinterpret_cast<const V*>(p)[j];
        xx[u] = reinterpret_cast<const V*>(x)[j];
      }
    }
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        V xn, pn;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const T xu = xx[u][w] + aw[w] * pp[u][w];
          const T pu = (pp[u][w] * bw[w]) + zz[u][w];
          xn[w] = (lw[w] && !fw[w]) ? xu : xx[u][w];
          pn[w] = lw[w] ? (fw[w] ? zz[u][w] : pu) : pp[u][w];
        }
        reinterpret_cast<V*>(x)[j] = xn;
        reinterpret_cast<V*>(p)[j] = pn;
      }
    }
  }
}

// UR: r -= α q in the running columns
template <typename T, int K>
__global__ void __launch_bounds__(kThreads) k_multi_update_r(int64_t nv, const PcgState* S, const T* __restrict__ q,
                                                             T* __restrict__ r) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  const int64_t jt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  T aw[W];
  bool lw[W];
#pragma unroll
  for (int w = 0; w < W; ++w) aw[w] = T(0), lw[w] = false;
  bool any = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const bool live = S[k].done == 0;
    any = any || live;
    const T alpha = T(S[k].alpha);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const bool mine = int((jt * W + w) & (K - 1)) == k;
      aw[w] = mine ? alpha : aw[w];
      lw[w] = mine ? live : lw[w];
    }
  }
  if (!any) return;
  for (int64_t j0 = jt; j0 < nv; j0 += ts * kElemUnroll) {
    V rr[kElemUnroll], qq[kElemUnroll];
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        rr[u] = reinterpret_cast<const V*>(r)[j];
        qq[u] = reinterpret_cast<const V*>(q)[j];
      }
    }
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        V rn;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const T ru = rr[u][w] - aw[w] * qq[u][w];
          rn[w] = lw[w] ? ru : rr[u][w];
        }
        reinterpret_cast<V*>(r)[j] = rn;
      }
    }
  }
}

// in: B, X [n][nrhs] -> b, x [n][K], columns >= nrhs zero
template <typename T>
__global__ void __launch_bounds__(kThreads) k_multi_pack(int64_t n, int nrhs, int K, const T* __restrict__ B,
                                                         const T* __restrict__ X, T* __restrict__ b,
                                                         T* __restrict__ x) {
  const int64_t ne = n * K;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < ne; e += int64_t(gridDim.x) * blockDim.x) {
    const int64_t i = e / K;
    const int j = int(e - i * K);
    b[e] = j < nrhs ? B[i * nrhs + j] : T(0);
    x[e] = j < nrhs ? X[i * nrhs + j] : T(0);
  }
}

// out: X [n][nrhs] <- x, with each column's deferred x += α_{k-1} p_{k-1} (k_x_fixup's rule); a
// zero column returns b (scipy)
template <typename T>
__global__ void __launch_bounds__(kThreads) k_multi_unpack(int64_t n, int nrhs, int K, const PcgState* S,
                                                           const T* __restrict__ b, const T* __restrict__ x,
                                                           const T* __restrict__ p, T* __restrict__ X) {
  const int64_t ne = n * nrhs;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < ne; e += int64_t(gridDim.x) * blockDim.x) {
    const int64_t i = e / nrhs;
    const int j = int(e - i * nrhs);
    const PcgState* St = S + j;
    const int64_t w = i * K + j;
    T v;
    if (St->bb == 0.0) {
      v = b[w];
    } else {
      v = x[w];
      if (St->iter >= 1) v = v + T(St->alpha) * p[w];
    }
    X[e] = v;
  }
}

// The workspace: per Kp the six interleaved vectors (q shares t's buffer, as in the solver), and
// for all of them the states, their pinned poll mirrors, the reduction's partials and ticket, the
// device histories and the captured chunks.
struct MultiWs {
  void* vec[3][6] = {};  // [Kp index][x, b, r, z, t, p], each (n rounded up to 4 rows) x Kp entries
  PcgState* S = nullptr;
  PcgState* hS = nullptr;
  double* partials = nullptr;
  unsigned* ticket = nullptr;
  double* dhist = nullptr;
  int64_t dhist_cap = 0;
  IterationGraphs graphs[3];
};

static int kp_index(int Kp) { return Kp == 2 ? 0 : Kp == 4 ? 1 : 2; }

void multi_clear_graphs(lspcg_solver* s) {
  if (!s->multi) return;
  for (auto& g : s->multi->graphs) g.clear();
}

void multi_destroy(lspcg_solver* s) {
  MultiWs* ws = s->multi;
  if (!ws) return;
  multi_clear_graphs(s);
  for (auto& row : ws->vec)
    for (void* v : row) (void)hipFree(v);
  (void)hipFree(ws->S);
  (void)hipHostFree(ws->hS);
  (void)hipFree(ws->partials);
  (void)hipFree(ws->ticket);
  (void)hipFree(ws->dhist);
  delete ws;
  s->multi = nullptr;
}

static int64_t multi_rows(const lspcg_solver* s) { return (s->n + 3) / 4 * 4; }  // whole 16-B vectors for every T, Kp

static int multi_workspace(lspcg_solver* s, int Kp) {
  if (!s->multi) {
    s->multi = new MultiWs();
    MultiWs* ws = s->multi;
    LSPCG_HIP(hipMalloc(&ws->S, sizeof(PcgState) * kMultiMax));
    LSPCG_HIP(hipHostMalloc(&ws->hS, 2 * sizeof(PcgState) * kMultiMax, hipHostMallocDefault));
    // one reducing launch in flight: <= 2 dots x 8 columns, DD each, per workgroup of the resident grid
    LSPCG_HIP(hipMalloc(&ws->partials, sizeof(double) * 2 * 2 * kMultiMax * (4096 + 1)));
    LSPCG_HIP(hipMalloc(&ws->ticket, sizeof(unsigned) * kTicketWords));
    LSPCG_HIP(hipMemsetAsync(ws->ticket, 0, sizeof(unsigned) * kTicketWords, s->stream));
  }
  MultiWs* ws = s->multi;
  void** v = ws->vec[kp_index(Kp)];
  if (!v[0]) {
    const size_t vb = esize(s->dtype) * size_t(multi_rows(s)) * Kp;
    for (int a = 0; a < 6; ++a) {
      LSPCG_HIP(hipMalloc(&v[a], vb));
      LSPCG_HIP(hipMemsetAsync(v[a], 0, vb, s->stream));
    }
  }
  return LSPCG_OK;
}

template <typename T, int K, class Pro, class Epi>
static int launch_spmm(lspcg_solver* s, int w, const T* x, Pro pro, Epi epi, hipStream_t st) {
  const SellPattern* P = s->sp[w];
  LSPCG_CHECK(P && spmm_supported(*P), LSPCG_ERR_UNSUPPORTED, "solve_multi: view without a K-vector kernel");
  if (sizeof(T) == 8 && s->svd[w] == LSPCG_F32) return launch_sell<T, float, K>(*P, s->sv[w], GatherVec<T>{x}, pro, epi, st);
  return launch_sell<T, T, K>(*P, s->sv[w], GatherVec<T>{x}, pro, epi, st);
}

template <typename T, int K>
static int enqueue_multi_init(lspcg_solver* s, hipStream_t st) {
  MultiWs* ws = s->multi;
  void** v = ws->vec[kp_index(K)];
  if (int rc = launch_spmm<T, K>(s, 0, as<T>(v[0]), ProNone{},
                                 EpiResidK<T, K>{as<T>(v[2]), as<T>(v[1]), ws->S, ws->partials, ws->ticket}, st))
    return rc;
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

template <typename T, int K, bool SC>
static int enqueue_multi_iteration(lspcg_solver* s, hipStream_t st) {
  MultiWs* ws = s->multi;
  void** v = ws->vec[kp_index(K)];
  T *x = as<T>(v[0]), *r = as<T>(v[2]), *z = as<T>(v[3]), *t = as<T>(v[4]), *p = as<T>(v[5]);
  T* q = t;  // never live together (solver_create)
  const T* d = SC ? as<T>(s->d) : nullptr;
  PcgState* S = ws->S;
  const ProAllDone<K> pro{S};
  const int64_t nv = multi_rows(s) * K / VecT<T>::W;
  const int eg = int(std::max<int64_t>(1, std::min<int64_t>((nv + int64_t(kThreads) * kElemUnroll - 1) /
                                                                (int64_t(kThreads) * kElemUnroll), kElemBlocksMax)));
  int rc = launch_spmm<T, K>(s, 2, static_cast<const T*>(r), pro, EpiTK<T, K, SC>{t, d}, st);
  if (rc) return rc;
  rc = launch_spmm<T, K>(s, 1, static_cast<const T*>(t), pro,
                         EpiZK<T, K, SC>{z, r, d, T(s->eps), S, ws->partials, ws->ticket}, st);
  if (rc) return rc;
  launch(k_multi_update_p<T, K>, dim3(eg), dim3(kThreads), st, nv, S, z, p, x);
  rc = launch_spmm<T, K>(s, 0, static_cast<const T*>(p), pro, EpiQK<T, K>{q, p, S, ws->partials, ws->ticket}, st);
  if (rc) return rc;
  launch(k_multi_update_r<T, K>, dim3(eg), dim3(kThreads), st, nv, S, q, r);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

// f(T{}, integral_constant<int, Kp>{}) for the solver's dtype and Kp = 2, 4, 8
template <class F>
static int by_dtype_k(int dtype, int Kp, F&& f) {
  return by_dtype(dtype, [&](auto t) {
    if (Kp == 2) return f(t, std::integral_constant<int, 2>{});
    if (Kp == 4) return f(t, std::integral_constant<int, 4>{});
    return f(t, std::integral_constant<int, 8>{});
  });
}

// why this solver has no K-vector solve, or nullptr
static const char* multi_unsupported(const lspcg_solver* s) {
  if (s->precond == LSPCG_PRECOND_IC) return "solve_multi: IC's triangular solves take one vector: solve one by one";
  if (s->precond != LSPCG_PRECOND_EXT_SPAI && s->precond != LSPCG_PRECOND_EXT_SPAI_SCALED)
    return "solve_multi: no preconditioner / diagonal have no K-vector schedule yet: solve one by one";
  if (s->A->block_size != 1) return "solve_multi: BSR 3x3 systems have no K-vector kernels: solve one by one";
  if (s->dot_order != LSPCG_DOT_COMPENSATED) return "solve_multi: the OpenBLAS dot order runs one vector at a time";
  if (s->ro.perm) return "solve_multi: the solver runs on a reordered system (LSPCG_REORDER=0 keeps the numbering)";
  for (int w = 0; w < 3; ++w)
    if (!s->sp[w] || !spmm_supported(*s->sp[w]))
      return "solve_multi: needs SELL-DIA or SELL-64 (16-bit / int32 column) views of A, L and L^T "
             "(lspcg_solver_views kinds 1, 16, 32)";
  return nullptr;
}

}  // namespace lspcg

extern "C" {

int lspcg_solver_solve_multi(lspcg_solver* s, int nrhs, const void* B, void* X, double rtol, int64_t max_iter,
                             int64_t* iters, int32_t* status, double* const* res_hist, double* t_solve_ms) {
  LSPCG_CHECK(s && B && X && iters && status, LSPCG_ERR_ARG, "solve_multi: NULL argument");
  LSPCG_CHECK(nrhs >= 1 && nrhs <= kMultiMax, LSPCG_ERR_ARG,
              "solve_multi: nrhs must be in [1, 8], got " + std::to_string(nrhs));
  if (const char* why = multi_unsupported(s)) {
    set_error(why);
    return LSPCG_ERR_UNSUPPORTED;
  }
  LSPCG_CHECK(s->LT, LSPCG_ERR_ARG, "solve_multi: ext_spai not set");
  if (nrhs == 1) {
    const int rc = lspcg_solver_solve(s, B, X, rtol, max_iter, iters, res_hist ? res_hist[0] : nullptr, t_solve_ms);
    if (rc == LSPCG_OK || rc == LSPCG_NOT_CONVERGED) status[0] = rc;
    return rc;
  }
  LSPCG_HIP(hipSetDevice(s->ctx->device));
  const int64_t n = s->n;
  if (max_iter <= 0) max_iter = n;
  const int Kp = nrhs <= 2 ? 2 : nrhs <= 4 ? 4 : 8;
  hipStream_t st = s->stream;
  if (int rc = multi_workspace(s, Kp)) return rc;
  MultiWs* ws = s->multi;
  std::vector<int64_t> hoff(nrhs + 1, 0);
  for (int j = 0; j < nrhs; ++j) hoff[j + 1] = hoff[j] + ((res_hist && res_hist[j]) ? max_iter + 2 : 0);
  if (int rc = grow_hist(&ws->dhist, &ws->dhist_cap, hoff[nrhs], st)) return rc;
  void** v = ws->vec[kp_index(Kp)];
  const int pg = int(std::max<int64_t>(1, std::min<int64_t>((n * Kp + kThreads - 1) / kThreads, kElemBlocksMax)));

  std::unique_lock<std::mutex> sub(submit_mutex());  // as in lspcg_solver_solve
  LSPCG_HIP(hipEventRecord(s->ev_in, s->ctx->stream));
  LSPCG_HIP(hipStreamWaitEvent(st, s->ev_in, 0));
  LSPCG_HIP(hipEventRecord(s->ev_t0, st));
  by_dtype(s->dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_multi_pack<T>, dim3(pg), dim3(kThreads), st, n, nrhs, Kp, as<T>(B), as<T>(static_cast<const void*>(X)),
           as<T>(v[1]), as<T>(v[0]));
    return 0;
  });
  LSPCG_HIP(hipGetLastError());
  for (int j = 0; j < Kp; ++j)
    ws->hS[j] = initial_state(rtol, s->eps, (j < nrhs && res_hist && res_hist[j]) ? ws->dhist + hoff[j] : nullptr,
                              max_iter);
  LSPCG_HIP(hipMemcpyAsync(ws->S, ws->hS, sizeof(PcgState) * Kp, hipMemcpyHostToDevice, st));
  int rc = by_dtype_k(s->dtype, Kp, [&](auto t, auto k) {
    return enqueue_multi_init<decltype(t), decltype(k)::value>(s, st);
  });
  if (rc) return rc;

  StatePoll poll{Kp, ws->S, ws->hS, {s->ev_poll, s->ev_poll2}, st, sub};
  std::vector<PcgState> cur(Kp);
  const std::vector<int64_t> mi(Kp, max_iter);
  const bool sc = s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED;
  auto one = [&] {
    return by_dtype_k(s->dtype, Kp, [&](auto t, auto k) {
      using T = decltype(t);
      constexpr int K = decltype(k)::value;
      return sc ? enqueue_multi_iteration<T, K, true>(s, st) : enqueue_multi_iteration<T, K, false>(s, st);
    });
  };
  IterationGraphs& graphs = ws->graphs[kp_index(Kp)];
  rc = poll.run(mi.data(), 32, [&](int c) { return graphs.launch(st, c, one); }, cur.data());
  if (rc) return rc;
  const int ug = int(std::max<int64_t>(1, std::min<int64_t>((n * nrhs + kThreads - 1) / kThreads, kElemBlocksMax)));
  by_dtype(s->dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_multi_unpack<T>, dim3(ug), dim3(kThreads), st, n, nrhs, Kp, ws->S, as<T>(v[1]), as<T>(v[0]), as<T>(v[5]),
           as<T>(X));
    return 0;
  });
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipEventRecord(s->ev_t1, st));
  LSPCG_HIP(hipEventRecord(s->ev_out, st));
  LSPCG_HIP(hipStreamWaitEvent(s->ctx->stream, s->ev_out, 0));
  LSPCG_HIP(poll.wait(s->ev_t1));
  float ms = 0.f;
  LSPCG_HIP(hipEventElapsedTime(&ms, s->ev_t0, s->ev_t1));
  if (t_solve_ms) *t_solve_ms = ms;
  return report_states(nrhs, cur.data(), mi.data(), ws->dhist, hoff.data(), iters, status, res_hist);
}

}  // extern "C"
