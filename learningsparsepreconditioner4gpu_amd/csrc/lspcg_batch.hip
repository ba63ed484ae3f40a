// ==== batched lockstep PCG (lspcg_batch_*) =====================================
// A window of independent systems is laid out block-diagonally, every system's rows padded to
// whole SpMV row tiles (256 block rows), and ONE launch per phase covers all of them.  The two
// ext_spai kinds run the split schedule's five launches (KA, KB, UP, KC, UR; the scaled kind with
// EpiT / RowZ's divisions by d = diag(A)); no preconditioner and the diagonal one have no KA / KB
// and run three (UP, KC, UR), UR also reducing the next iteration's dots (‖r‖², ρ = r·z) per
// system.  In every launch
//   * one row tile per workgroup (launch_sell one_tile_per_wg), so a workgroup's dot
//     partial is its tile's and its prologue tests the tile's own system (done systems' tiles
//     leave at once);
//   * per-system last-arriver dot reductions (batch_sys_reduce): the last tile of a system to
//     finish KB / KC sums the system's tile partials and updates its PcgState (scipy's scalars,
//     the top-of-loop test, the iteration count), as the last-arriver schedule does for one system;
//   * elementwise launches (UP, UR) of one 256-row tile per workgroup that read their system's
//     finished scalars; the three-launch UR reduces per system over ELEMENTWISE tiles (bs per SpMV
//     tile), with tickets and partials of its own sized for that launch.
// Padding rows are empty: they stay 0 in every vector and add exact zeros to the dots; the kinds
// that divide by d give them d = 1 at creation (k_batch_pad_d), since diag(A) is 0 there and 0/0
// would put NaN into the system's dots.
//
// The window is solved by an lspcg_solver of the block-diagonal system (lspcg_solver.hpp, created
// in lspcg_pcg.hip).  The epilogues' row bodies and the one-workgroup solve are those of
// lspcg_pcg_kernels.hpp, every state transition is lspcg_pcg_step.hpp's; this unit adds the
// per-system way of finishing the dots and the elementwise kernels of one tile per workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "lspcg_pcg_kernels.hpp"
#include "lspcg_solver.hpp"

using namespace lspcg;

namespace lspcg {

struct BatchMap {
  const int32_t* etile_sys;  // [n / 256] system of each 256-row elementwise tile
  const int32_t* tile0;      // [nsys + 1] first SpMV row tile (256 block rows) of each system
  const int32_t* tk0;        // [nsys] first ticket line of each system: [top | group 0 | group 1 | ...]
  int bs;                    // block size: SpMV tile b covers elementwise tiles bs*b .. bs*b + bs - 1
};

struct ProTile {
  const PcgState* S;
  BatchMap m;
  __device__ __forceinline__ bool exit() const { return S[m.etile_sys[int64_t(blockIdx.x) * m.bs]].done != 0; }
};

// Per-system last-arriver reduction of a batched launch's N dots: each workgroup (= one row tile)
// publishes its tile total and arrives on the system's two-level ticket (publish_dd, ticket_arrive:
// <= 32 serialised arrivals per line instead of a system's few hundred -- the fan-in price), and the system's last arriving tile sums the system's
// tile totals in tile order (fixed tree: the result does not depend on which tile came last);
// thread 0 then runs fin(sys, values).  The elementwise launches read finished per-system scalars.
// sys_reduce_tiles is the reduction itself over tiles [t0, t0 + nt) of system `sys` in the launch's
// own tile numbering (SpMV row tiles, or elementwise tiles for the three-launch UR), `top` the
// system's first ticket line for that launch.
template <int N, class Fin>
__device__ __forceinline__ void sys_reduce_tiles(DD (&v)[N], double* partials, unsigned* top, int sys, int t0, int nt,
                                                 Fin fin) {
  __shared__ DD lds[16 * N];
  __shared__ int s_last;
  block_reduce_dd<N>(v, lds);
  const int64_t tile = blockIdx.x;
  if (threadIdx.x == 0) {
    publish_dd<N>(&partials[size_t(tile) * N * 2], v);
    const bool last = ticket_arrive(top, unsigned(tile - t0), unsigned(nt));
    if (last) ticket_reset(top);  // at once: the partials, not the ticket, carry what the sum below reads
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  DD acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = dd_zero();
  for (int b = threadIdx.x; b < nt; b += blockDim.x) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      acc[j] = dd_add(acc[j], read_dd(&partials[(size_t(t0 + b) * N + j) * 2]));
    }
  }
  __syncthreads();
  block_reduce_dd<N>(acc, lds);
  if (threadIdx.x == 0) {
    double out[N];
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = dd_value(acc[j]);
    fin(sys, out);
  }
}

template <int N, class Fin>
__device__ __forceinline__ void batch_sys_reduce(DD (&v)[N], double* partials, unsigned* tickets, const BatchMap& m,
                                                 Fin fin) {
  const int sys = m.etile_sys[int64_t(blockIdx.x) * m.bs];
  const int t0 = m.tile0[sys];
  sys_reduce_tiles<N>(v, partials, tickets + size_t(kTicketStride) * m.tk0[sys], sys, t0, m.tile0[sys + 1] - t0, fin);
}

// Finishing way 3 of an epilogue's dots (lspcg_pcg_kernels.hpp has the row bodies and the other
// two): the per-system last arriver, which runs the composed epilogue's static fin(state, values).
struct BySystem {
  static constexpr bool CUSTOM_FINISH = true;
  PcgState* S;
  double* partials;
  unsigned* tickets;
  BatchMap m;
};
template <class Epi>
__device__ __forceinline__ void finish_by_system(const Epi& e, DD (&dd)[Epi::NDOT]) {
  PcgState* Sb = e.S;
  batch_sys_reduce<Epi::NDOT>(dd, e.partials, e.tickets, e.m, [Sb](int sys, const double* v) { Epi::fin(Sb + sys, v); });
}

// init: r_0 = b - A x0 ; ‖r_0‖², ‖b‖² -> the system's initial state.  PRE = NONE / DIAGONAL
// (three-launch schedule): Jacobi's z_0 = r_0/d and ρ_0, and the last arriver also runs iteration
// 0's top-of-loop test, which the ext_spai kinds leave to KB
template <typename T, int PRE = LSPCG_PRECOND_EXT_SPAI>
struct EpiResidB : RowResid<T, PRE>, BySystem {
  static constexpr bool CG = PRE == LSPCG_PRECOND_NONE || PRE == LSPCG_PRECOND_DIAGONAL;
  static constexpr int NDOT = RowResid<T, PRE>::NDOT;
  __device__ __forceinline__ void finish(DD (&dd)[NDOT]) const { finish_by_system(*this, dd); }
  __device__ static __forceinline__ void fin(PcgState* St, const double* v) {
    const double rtol = St->rtol;
    double* const hist = St->hist;
    const int64_t max_iter = CG ? St->max_iter : 0;
    init_state<T, CG>(St, rtol, hist, v[0], v[1], v[PRE == LSPCG_PRECOND_DIAGONAL ? 2 : 0], max_iter);
  }
};

// KB: z = L t + ε r ; ρ_k = r·z, ‖r_k‖² -> the system's last arriver keeps ρ_k and runs scipy's
// top-of-loop test on ‖r_k‖: every tile of the system has already passed this launch's prologue,
// so setting `done` here is seen first by UP.
// (RowZ's body on members of its own, in the kernel-argument order this epilogue was measured with:
// with RowZ as a base the compiler schedules the SELL-DIA row loop differently, 153.1 vs 150.7 us per
// launch on a window of 8 x 1 M rows)
template <typename T, bool SCALED = false>
struct EpiZB {
  static constexpr int NDOT = 2;
  static constexpr bool CUSTOM_FINISH = true;
  T* z;
  const T* r;
  T eps;
  PcgState* S;
  double* partials;
  unsigned* tickets;
  BatchMap m;
  const T* d = nullptr;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, T s, DD* dots) const {
    RowZ<T, SCALED>{z, r, d, eps}.row(i, s, dots);
  }
  __device__ __forceinline__ void finish(DD (&dd)[2]) const { finish_by_system(*this, dd); }
  __device__ static __forceinline__ void fin(PcgState* St, const double* v) {
    const int64_t k = St->iter, max_iter = St->max_iter;
    const double rho_old = St->rho, rr0 = St->rr, atol = St->atol;  // ‖r_0‖² from the init
    double* const hist = St->hist;
    const double rrk = keep_z<T>(St, k, rho_old, hist, v[0], v[1]);
    const int code = loop_test<T>(k, max_iter, k > 0 ? rrk : rr0, atol);
    if (code) St->done = code;
  }
};

// KC: q = A p ; π_k = p·q -> α_k = ρ_k/π_k, iteration k+1
template <typename T>
struct EpiQB : RowQ<T>, BySystem {
  __device__ __forceinline__ void finish(DD (&dd)[1]) const { finish_by_system(*this, dd); }
  __device__ static __forceinline__ void fin(PcgState* St, const double* v) {
    const int64_t k = St->iter;
    double* const coef = St->coef;
    keep_q<T, true>(St, k, coef, St->rho, v[0]);
  }
};

// UP: x += α_{k-1} p_{k-1} (k > 0) ; p_k = p_{k-1}β + z with β = ρ_k/ρ_{k-1}, one 256-row tile of
// one system per workgroup
template <typename T>
__global__ void __launch_bounds__(kThreads) k_batch_update_p(BatchMap m, const PcgState* S, const T* __restrict__ z,
                                                             T* __restrict__ p, T* __restrict__ x) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const T zi = z[i], pi = p[i], xi = x[i];
  const PcgState* St = S + m.etile_sys[blockIdx.x];
  if (St->done) return;
  const bool first = St->iter == 0;
  const T beta = first ? T(0) : T(St->rho) / T(St->rho_prev);
  const T alpha = T(St->alpha);
  if (!first) x[i] = xi + alpha * pi;
  p[i] = first ? zi : (pi * beta) + zi;
}

// UR: r_{k+1} = r_k - α_k q
template <typename T>
__global__ void __launch_bounds__(kThreads) k_batch_update_r(BatchMap m, const PcgState* S, const T* __restrict__ q,
                                                             T* __restrict__ r) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const T ri = r[i], qi = q[i];
  const PcgState* St = S + m.etile_sys[blockIdx.x];
  if (St->done) return;
  r[i] = ri - T(St->alpha) * qi;
}

// The elementwise tile's row of the three-launch UR: r_{k+1} = r_k - α q stored, then r_dots_row
// (dots[0] = ‖r_{k+1}‖², dots[ND - 1] = ρ_{k+1})
template <typename T, int PRE>
__device__ __forceinline__ void update_r_row(int64_t i, T ri, T qi, T alpha, T* __restrict__ r,
                                             const T* __restrict__ d, T* __restrict__ z,
                                             DD (&dots)[PRE == LSPCG_PRECOND_DIAGONAL ? 2 : 1]) {
  const T rn = ri - alpha * qi;
  r[i] = rn;
  r_dots_row<T, PRE, false>(i, rn, d, z, dots[0], dots[PRE == LSPCG_PRECOND_DIAGONAL ? 1 : 0]);
}

// UR of the three-launch schedule (no preconditioner / Jacobi), last-arriver mode: the update, then
// the per-system reduction over the system's ELEMENTWISE tiles (m.bs per SpMV tile: tickets `tk0`
// / `tickets` and `partials` are this launch's own, sized for it).  KC's last arriver has already
// counted the iteration (EpiQB), so the system's last arriver here keeps ‖r_{k+1}‖² and ρ_{k+1}
// and runs iteration k+1's top-of-loop test: every tile of the system has read
// `done` and α by then, and UP is the first launch to see the new `done`.
template <typename T, int PRE>
__global__ void __launch_bounds__(kThreads) k_batch_update_r_dots(BatchMap m, PcgState* S, const T* __restrict__ q,
                                                                  T* __restrict__ r, const T* __restrict__ d,
                                                                  T* __restrict__ z, double* partials,
                                                                  unsigned* tickets, const int32_t* __restrict__ tk0) {
  constexpr int ND = PRE == LSPCG_PRECOND_DIAGONAL ? 2 : 1;
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const T ri = r[i], qi = q[i];
  const int sys = m.etile_sys[blockIdx.x];
  PcgState* Sb = S;
  if (Sb[sys].done) return;  // workgroup-uniform
  DD dots[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) dots[j] = dd_zero();
  update_r_row<T, PRE>(i, ri, qi, T(Sb[sys].alpha), r, d, z, dots);
  const int t0 = m.tile0[sys] * m.bs, nt = (m.tile0[sys + 1] - m.tile0[sys]) * m.bs;
  sys_reduce_tiles<ND>(dots, partials, tickets + size_t(kTicketStride) * tk0[sys], sys, t0, nt,
                       [Sb](int s, const double* v) {
                         PcgState* St = Sb + s;
                         const int64_t it = St->iter, max_iter = St->max_iter;  // it = k + 1 (EpiQB)
                         const double rho_old = St->rho, atol = St->atol;
                         double* const hist = St->hist;
                         const double rr2 = keep_r<T, true>(St, it, rho_old, hist, v[0], v[ND - 1]);
                         const int code = loop_test<T>(it, max_iter, rr2, atol);
                         if (code) St->done = code;
                       });
}

// ---- consumer-sum mode (windows whose systems have <= 128 tiles each): KB / KC only store
// per-tile partials (grid_partial_groups, gsz = 1: no tickets) and every UP / UR workgroup sums its
// system's tile partials itself (group_sum_dd, one wave for <= 256) ------------------------------
// init: r_0 = b - A x0 ; per-tile partials of ‖r_0‖², ‖b‖² (PRE = DIAGONAL: + z_0 = r_0/d and ρ_0)
template <typename T, int PRE = LSPCG_PRECOND_EXT_SPAI>
using EpiResidTile = EpiGroups<RowResid<T, PRE>>;

// one workgroup per system: the init state from the system's tile partials
template <typename T, int PRE = LSPCG_PRECOND_EXT_SPAI>
__global__ void __launch_bounds__(kThreads) k_batch_init(PcgState* S, const int32_t* __restrict__ tile0,
                                                         const double* __restrict__ gi) {
  constexpr int ND = PRE == LSPCG_PRECOND_DIAGONAL ? 3 : 2;
  const int sys = blockIdx.x;
  const int t0 = tile0[sys], t1 = tile0[sys + 1];
  double v[ND];
  group_sum_dd<ND>(gi + size_t(t0) * 2 * ND, t1 - t0, v);
  if (threadIdx.x) return;
  PcgState* St = S + sys;
  const double rtol = St->rtol;
  double* const hist = St->hist;
  init_state<T>(St, rtol, hist, v[0], v[1], v[PRE == LSPCG_PRECOND_DIAGONAL ? 2 : 0]);
}

// consumer-sum mode: UP of the split schedule for the tile's system, summing the system's tile
// partials itself
// CG (three-launch schedule): gz holds UR's per-ELEMENTWISE-tile partials (bs per SpMV tile) of
// ρ_k, ‖r_k‖² for k > 0 (iteration 0 takes both from the init state), z is r without a
// preconditioner, and the system's first workgroup leaves ρ_k in the state for UR (rho_k), which
// overwrites gz
template <typename T, bool CG = false>
__global__ void __launch_bounds__(kThreads) k_batch_update_p_sums(BatchMap m, PcgState* S, const double* __restrict__ gz,
                                                             const T* __restrict__ z, T* __restrict__ p,
                                                             T* __restrict__ x) {
  const int sys = m.etile_sys[blockIdx.x];
  PcgState* St = S + sys;
  // `done` is loaded once and tested only after the group sums: group_sum_dd may hold workgroup
  // barriers, and this system's first workgroup can write `done` during this launch
  const int32_t done = St->done;
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const T zi = z[i], pi = p[i], xi = x[i];
  const int t0 = m.tile0[sys], t1 = m.tile0[sys + 1];
  const int64_t k = St->iter;
  const int per = CG ? m.bs : 1;
  double v[2];
  group_sum_dd<2>(gz + size_t(t0) * per * 4, (t1 - t0) * per, v);
  if (done) return;
  const double rho = (!CG || k > 0) ? round_to<T>(v[0]) : St->rho;
  const double rr = k > 0 ? round_to<T>(v[1]) : St->rr;
  const int code = loop_test<T>(k, St->max_iter, rr, St->atol);
  if (int64_t(blockIdx.x) == int64_t(t0) * m.bs && threadIdx.x == 0) {
    keep_rr<T>(St, k, St->hist, rr);
    if (code) St->done = code;
    else if constexpr (CG) St->rho_k = rho;
  }
  if (code) return;
  const bool first = k == 0;
  const T beta = first ? T(0) : T(rho) / T(St->rho);
  const T alpha = T(St->alpha);
  if (!first) x[i] = xi + alpha * pi;
  p[i] = first ? zi : (pi * beta) + zi;
}

// consumer-sum mode: UR of the split schedule for the tile's system
template <typename T>
__global__ void __launch_bounds__(kThreads) k_batch_update_r_sums(BatchMap m, PcgState* S, const double* __restrict__ gz,
                                                             const double* __restrict__ gq, const T* __restrict__ q,
                                                             T* __restrict__ r) {
  const int sys = m.etile_sys[blockIdx.x];
  PcgState* St = S + sys;
  if (St->done) return;
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const T ri = r[i], qi = q[i];
  const int t0 = m.tile0[sys], t1 = m.tile0[sys + 1];
  double vz[2], vq[1];
  group_sum_dd<2>(gz + size_t(t0) * 4, t1 - t0, vz);
  group_sum_dd<1>(gq + size_t(t0) * 2, t1 - t0, vq);
  const double rho = round_to<T>(vz[0]);
  const double pq = round_to<T>(vq[0]);
  const T alpha = T(rho) / T(pq);
  if (int64_t(blockIdx.x) == int64_t(t0) * m.bs && threadIdx.x == 0) {
    const double rho_old = St->rho;
    const int64_t k = St->iter;
    double* const coef = St->coef;
    commit_step<T>(St, coef, rho_old, rho, pq, alpha, k + 1);
  }
  r[i] = ri - alpha * qi;
}

// consumer-sum mode: UR of the three-launch schedule for the tile's system:
// α_k = ρ_k/π_k from the state's ρ_k (UP) and KC's tile partials, the update, and this elementwise
// tile's partials of ρ_{k+1}, ‖r_{k+1}‖² for the next UP (plain stores: read after the kernel boundary)
template <typename T, int PRE>
__global__ void __launch_bounds__(kThreads) k_batch_update_r_sums_cg(BatchMap m, PcgState* S,
                                                                     const double* __restrict__ gq,
                                                                     const T* __restrict__ q, T* __restrict__ r,
                                                                     const T* __restrict__ d, T* __restrict__ z,
                                                                     double* __restrict__ gz) {
  constexpr int ND = PRE == LSPCG_PRECOND_DIAGONAL ? 2 : 1;
  __shared__ DD lds[16 * ND];
  const int sys = m.etile_sys[blockIdx.x];
  PcgState* St = S + sys;
  if (St->done) return;  // written by UP only: uniform over this launch
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const T ri = r[i], qi = q[i];
  const int t0 = m.tile0[sys], t1 = m.tile0[sys + 1];
  const double rho = St->rho_k;
  double vq[1];
  group_sum_dd<1>(gq + size_t(t0) * 2, t1 - t0, vq);
  const double pq = round_to<T>(vq[0]);
  const T alpha = T(rho) / T(pq);
  if (int64_t(blockIdx.x) == int64_t(t0) * m.bs && threadIdx.x == 0) {
    const double rho_old = St->rho;
    const int64_t k = St->iter;
    double* const coef = St->coef;
    commit_step<T>(St, coef, rho_old, rho, pq, alpha, k + 1);
  }
  DD dots[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) dots[j] = dd_zero();
  update_r_row<T, PRE>(i, ri, qi, alpha, r, d, z, dots);
  block_reduce_dd<ND>(dots, lds);
  if (threadIdx.x == 0) {
    double* out = gz + size_t(blockIdx.x) * 4;  // [ρ | ‖r‖²], DD each
    out[0] = dots[ND - 1].s;
    out[1] = dots[ND - 1].c;
    out[2] = dots[0].s;
    out[3] = dots[0].c;
  }
}

// padding rows of the block-diagonal system get d = 1 (diag(A) is 0 there): the divisions by d of
// the diagonal and scaled kinds then keep them exactly 0
template <typename T>
__global__ void __launch_bounds__(kThreads) k_batch_pad_d(BatchMap m, const int32_t* __restrict__ boff,
                                                          const int32_t* __restrict__ bn, T* __restrict__ d) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  const int sys = m.etile_sys[blockIdx.x];
  if (i >= int64_t(boff[sys]) + bn[sys]) d[i] = T(1);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) k_batch_x_fixup(BatchMap m, const PcgState* S, const T* __restrict__ p,
                                                            T* __restrict__ x) {
  const PcgState* St = S + m.etile_sys[blockIdx.x];
  if (St->iter < 1 || St->bb == 0.0) return;
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  x[i] = x[i] + T(St->alpha) * p[i];
}

// block-diagonal assembly: rows [0, cnt) of one system at its row offset (rows >= nb empty)
__global__ void k_cat_rowptr(int64_t cnt, int64_t nb, const int32_t* __restrict__ rp, int32_t e0,
                             int32_t* __restrict__ out) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < cnt; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = rp[i < nb ? i : nb] + e0;
}
__global__ void k_cat_colind(int64_t nnz, const int32_t* __restrict__ c, int32_t off, int32_t* __restrict__ out) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < nnz; k += int64_t(gridDim.x) * blockDim.x)
    out[k] = c[k] + off;
}


// One given matrix of an update window (lspcg_batch_update): the caller's arrays beside the
// system's slice of the block-diagonal copy, which holds the pattern shifted by the system's entry
// offset e0 (rowptr) and block-row offset brow (colind): k_cat_rowptr / k_cat_colind
struct CatSlice {
  const int32_t* rp;   // [nb + 1] the caller's
  const int32_t* ci;   // [nnzb]
  const void* vals;    // [nval]
  const int32_t* crp;  // the slice of Acat / Lcat
  const int32_t* cci;
  void* cvals;
  int64_t nb, nnzb, nval;  // block rows, stored blocks, values (bs * bs per block)
  int32_t e0, brow;
};

// every given matrix of the window against its slice, matrices over gridDim.y: any difference sets
// the flag (rows past nb of a slice are empty and repeat rowptr[nb]; they hold no caller's data)
__global__ void __launch_bounds__(kThreads) k_cat_same_pattern(int nmat, const CatSlice* __restrict__ tab,
                                                               int* __restrict__ flag) {
  for (int m = blockIdx.y; m < nmat; m += gridDim.y) {
    const CatSlice d = tab[m];
    const int64_t nr = d.nb + 1, tot = nr + d.nnzb;
    bool diff = false;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < tot; i += int64_t(gridDim.x) * blockDim.x) {
      if (i < nr) diff |= uint32_t(d.rp[i]) + uint32_t(d.e0) != uint32_t(d.crp[i]);
      else diff |= uint32_t(d.ci[i - nr]) + uint32_t(d.brow) != uint32_t(d.cci[i - nr]);
    }
    if (diff) atomicOr(flag, 1);
  }
}

// the given matrices' values into their slices, in place
template <typename T>
__global__ void __launch_bounds__(kThreads) k_cat_copy_values(int nmat, const CatSlice* __restrict__ tab) {
  for (int m = blockIdx.y; m < nmat; m += gridDim.y) {
    const CatSlice d = tab[m];
    const T* __restrict__ src = static_cast<const T*>(d.vals);
    T* __restrict__ dst = static_cast<T*>(d.cvals);
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < d.nval; i += int64_t(gridDim.x) * blockDim.x)
      dst[i] = src[i];
  }
}

}  // namespace lspcg

struct lspcg_batch {
  lspcg_ctx* ctx = nullptr;
  int nsys = 0;
  int bs = 1;
  int dtype = LSPCG_F64;
  int precond = LSPCG_PRECOND_EXT_SPAI;  // none / diagonal: the three-launch iteration
  lspcg_mat* Acat = nullptr;
  lspcg_mat* Lcat = nullptr;
  lspcg_solver* s = nullptr;  // solver of the block-diagonal system: views, vectors, stream
  std::vector<int64_t> off, n;  // scalar row offset and size of every system
  int64_t ntot = 0;             // padded scalar rows
  int32_t* etile_sys = nullptr;
  int32_t* tile0 = nullptr;
  int32_t* tk0 = nullptr;
  double* partials = nullptr;  // per-tile dot partials of the reducing launch in flight (<= 3 dots, DD each;
                               // SpMV row tiles, or elementwise tiles in the three-launch UR)
  unsigned* tickets = nullptr;  // per system: top line + one line per kTicketGroup tiles (batch_sys_reduce)
  int32_t* etk0 = nullptr;      // three-launch UR: first ticket line of each system in etickets, which
  unsigned* etickets = nullptr;  // has one line per kTicketGroup ELEMENTWISE tiles (bs per SpMV tile)
  bool sums = false;            // consumer-sum reductions (every system <= 128 tiles; LSPCG_BATCH_REDUCE)
  bool small = false;           // every system fits the one-workgroup solve: one launch, one workgroup per system
  int64_t max_n = 0;
  int32_t* boff = nullptr;      // [nsys] scalar row offset / size of each system (small mode)
  int32_t* bn = nullptr;
  double* gsum = nullptr;       // consumer-sum partials: init (<= 3 dots) | gz | gq, per tile
  double* gz = nullptr;         // ... ρ, ‖r‖²: KB's per SpMV tile, or the three-launch UR's per elementwise tile
  double* gq = nullptr;         // ... π: KC's per SpMV tile
  int64_t ntiles = 0;
  PcgState* S = nullptr;
  PcgState* hS = nullptr;  // pinned: 2 poll slots x nsys
  double* dhist = nullptr;
  int64_t dhist_cap = 0;
  lspcg::IterationGraphs graphs;  // of enqueue_batch_iteration
  // lspcg_batch_update: every system's block rows and stored blocks of A and L, its entry offsets in
  // Acat / Lcat, the descriptor table of one update (allocated by the first) and its timing events
  std::vector<int64_t> nb, brow, annz, lnnz, ae0, le0;
  lspcg::CatSlice* utab = nullptr;
  hipEvent_t ev_u0 = nullptr, ev_u1 = nullptr;
  bool update_failed = false;  // the last lspcg_batch_update failed past its checks: solves return update_rc
  int update_rc = LSPCG_OK;
};

namespace lspcg {

static BatchMap batch_map(const lspcg_batch* bt) { return BatchMap{bt->etile_sys, bt->tile0, bt->tk0, bt->bs}; }

// SpMV of iteration view w over the block-diagonal system, one row tile per workgroup
template <typename T, class Pro, class Epi>
static int launch_it_tiles(lspcg_solver* s, int w, const T* x, Pro pro, Epi epi, hipStream_t st) {
  const SellPattern* P = s->sp[w];
  if (!P) return LSPCG_ERR_UNSUPPORTED;
  if constexpr (sizeof(T) == 8) {
    if (s->svd[w] == LSPCG_F32) return launch_sell<T, float>(*P, s->sv[w], GatherVec<T>{x}, pro, epi, st, true);
  }
  return launch_sell<T, T>(*P, s->sv[w], GatherVec<T>{x}, pro, epi, st, true);
}

template <typename T>
static int enqueue_batch_init(lspcg_batch* bt, hipStream_t st) {
  lspcg_solver* s = bt->s;
  const T* x = as<T>(s->x);
  // PRE: EXT_SPAI stands for both ext_spai kinds (their init has no preconditioner part)
  auto go = [&](auto pre) -> int {
    constexpr int PRE = decltype(pre)::value;
    const RowResid<T, PRE> row{as<T>(s->r), as<T>(s->b), as<T>(s->d), as<T>(s->z)};
    if (bt->sums) {
      int rc = launch_it_tiles<T>(s, 0, x, ProNone{}, EpiResidTile<T, PRE>{row, {nullptr, nullptr, bt->gsum, 1}}, st);
      if (rc) return rc;
      launch(k_batch_init<T, PRE>, dim3(bt->nsys), dim3(kThreads), st, bt->S, bt->tile0, bt->gsum);
      LSPCG_HIP(hipGetLastError());
      return LSPCG_OK;
    }
    return launch_it_tiles<T>(s, 0, x, ProNone{},
                              EpiResidB<T, PRE>{row, {bt->S, bt->partials, bt->tickets, batch_map(bt)}}, st);
  };
  if (bt->precond == LSPCG_PRECOND_NONE) return go(std::integral_constant<int, LSPCG_PRECOND_NONE>{});
  if (bt->precond == LSPCG_PRECOND_DIAGONAL) return go(std::integral_constant<int, LSPCG_PRECOND_DIAGONAL>{});
  return go(std::integral_constant<int, LSPCG_PRECOND_EXT_SPAI>{});
}

// the three-launch iteration of the kinds without KA / KB (no preconditioner, Jacobi): UP, KC, UR
template <typename T, int PRE>
static int enqueue_batch_iteration_cg(lspcg_batch* bt, hipStream_t st) {
  lspcg_solver* s = bt->s;
  T *x = as<T>(s->x), *r = as<T>(s->r), *z = as<T>(s->z), *p = as<T>(s->p), *q = as<T>(s->q);
  const T* d = as<T>(s->d);
  const T* zp = PRE == LSPCG_PRECOND_NONE ? r : z;  // z = r without a preconditioner
  const BatchMap m = batch_map(bt);
  const ProTile pro{bt->S, m};
  const BySystem by{bt->S, bt->partials, bt->tickets, m};
  const dim3 eg(unsigned(bt->ntot / kThreads)), eb(kThreads);
  int rc = LSPCG_OK;
  if (bt->sums) {
    launch(k_batch_update_p_sums<T, true>, eg, eb, st, m, bt->S, bt->gz, zp, p, x);
    rc = launch_it_tiles<T>(s, 0, p, pro, EpiQG<T>{{q, p}, {nullptr, nullptr, bt->gq, 1}}, st);
    if (rc) return rc;
    launch(k_batch_update_r_sums_cg<T, PRE>, eg, eb, st, m, bt->S, bt->gq, q, r, d, z, bt->gz);
  } else {
    launch(k_batch_update_p<T>, eg, eb, st, m, bt->S, zp, p, x);
    rc = launch_it_tiles<T>(s, 0, p, pro, EpiQB<T>{{q, p}, by}, st);
    if (rc) return rc;
    launch(k_batch_update_r_dots<T, PRE>, eg, eb, st, m, bt->S, q, r, d, z, bt->partials, bt->etickets, bt->etk0);
  }
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

template <typename T, bool SC>
static int enqueue_batch_iteration_spai(lspcg_batch* bt, hipStream_t st) {
  lspcg_solver* s = bt->s;
  T *x = as<T>(s->x), *r = as<T>(s->r), *z = as<T>(s->z), *t = as<T>(s->t), *p = as<T>(s->p), *q = as<T>(s->q);
  const BatchMap m = batch_map(bt);
  const ProTile pro{bt->S, m};
  const BySystem by{bt->S, bt->partials, bt->tickets, m};
  const dim3 eg(unsigned(bt->ntot / kThreads)), eb(kThreads);
  const T* d = SC ? as<T>(s->d) : nullptr;
  const RowZ<T, SC> rowz{z, r, d, T(s->eps)};
  int rc = launch_it_tiles<T>(s, 2, r, pro, EpiT<T, SC>{t, d}, st);
  if (rc) return rc;
  if (bt->sums) {
    rc = launch_it_tiles<T>(s, 1, t, pro, EpiZG<T, SC>{rowz, {nullptr, nullptr, bt->gz, 1}}, st);
    if (rc) return rc;
    launch(k_batch_update_p_sums<T>, eg, eb, st, m, bt->S, bt->gz, z, p, x);
    rc = launch_it_tiles<T>(s, 0, p, pro, EpiQG<T>{{q, p}, {nullptr, nullptr, bt->gq, 1}}, st);
    if (rc) return rc;
    launch(k_batch_update_r_sums<T>, eg, eb, st, m, bt->S, bt->gz, bt->gq, q, r);
  } else {
    rc = launch_it_tiles<T>(s, 1, t, pro, EpiZB<T, SC>{z, r, T(s->eps), bt->S, bt->partials, bt->tickets, m, d}, st);
    if (rc) return rc;
    launch(k_batch_update_p<T>, eg, eb, st, m, bt->S, z, p, x);
    rc = launch_it_tiles<T>(s, 0, p, pro, EpiQB<T>{{q, p}, by}, st);
    if (rc) return rc;
    launch(k_batch_update_r<T>, eg, eb, st, m, bt->S, q, r);
  }
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

template <typename T>
static int enqueue_batch_iteration(lspcg_batch* bt, hipStream_t st) {
  switch (bt->precond) {
    case LSPCG_PRECOND_NONE: return enqueue_batch_iteration_cg<T, LSPCG_PRECOND_NONE>(bt, st);
    case LSPCG_PRECOND_DIAGONAL: return enqueue_batch_iteration_cg<T, LSPCG_PRECOND_DIAGONAL>(bt, st);
    case LSPCG_PRECOND_EXT_SPAI_SCALED: return enqueue_batch_iteration_spai<T, true>(bt, st);
    default: return enqueue_batch_iteration_spai<T, false>(bt, st);
  }
}

// block-diagonal copy of M[0..nsys) with system k's block rows starting at brow[k] (padded)
static int cat_matrices(lspcg_ctx* ctx, int nsys, const lspcg_mat* const* M, const std::vector<int64_t>& brow,
                        lspcg_mat** out) {
  const int bs = M[0]->block_size;
  int64_t nnz = 0;
  for (int k = 0; k < nsys; ++k) nnz += M[k]->nnzb;
  LSPCG_CHECK(nnz < (int64_t(1) << 31), LSPCG_ERR_ARG, "batch: more than 2^31 stored blocks in the window");
  lspcg_mat* C = nullptr;
  if (int rc = mat_alloc(ctx, brow[nsys], nnz, bs, M[0]->dtype, &C)) return rc;
  hipStream_t st = ctx->stream;
  const size_t vb = (M[0]->dtype == LSPCG_F32 ? 4 : 8) * size_t(bs) * bs;
  int64_t e0 = 0;
  for (int k = 0; k < nsys; ++k) {
    const int64_t cnt = brow[k + 1] - brow[k] + (k == nsys - 1 ? 1 : 0);
    launch(k_cat_rowptr, dim3(unsigned(std::min<int64_t>((cnt + 255) / 256, 1024))), dim3(256), st, cnt, M[k]->nb,
           M[k]->rowptr, int32_t(e0), C->rowptr + brow[k]);
    if (M[k]->nnzb) {
      launch(k_cat_colind, dim3(unsigned(std::min<int64_t>((M[k]->nnzb + 255) / 256, 1024))), dim3(256), st,
             M[k]->nnzb, M[k]->colind, int32_t(brow[k]), C->colind + e0);
      LSPCG_HIP(hipMemcpyAsync(static_cast<char*>(C->vals) + vb * e0, M[k]->vals, vb * M[k]->nnzb,
                               hipMemcpyDeviceToDevice, st));
    }
    e0 += M[k]->nnzb;
  }
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipStreamSynchronize(st));
  *out = C;
  return LSPCG_OK;
}

// d = diag of the block-diagonal system (solver_create / set_spai / update_matrix) gets 1 on padding rows
static int pad_d(lspcg_batch* bt) {
  by_dtype(bt->dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_batch_pad_d<T>, dim3(unsigned(bt->ntot / kThreads)), dim3(kThreads), bt->ctx->stream, batch_map(bt),
           bt->boff, bt->bn, as<T>(bt->s->d));
    return 0;
  });
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipStreamSynchronize(bt->ctx->stream));
  return LSPCG_OK;
}

}  // namespace lspcg

extern "C" {

int lspcg_batch_views(const lspcg_batch* bt, int* col_kind, int* value_bytes) {
  LSPCG_CHECK(bt && bt->s, LSPCG_ERR_ARG, "batch_views: NULL argument");
  return lspcg_solver_views(bt->s, col_kind, value_bytes);
}

int lspcg_batch_destroy(lspcg_batch* bt) {
  if (!bt) return LSPCG_OK;
  (void)hipSetDevice(bt->ctx->device);
  if (bt->s) (void)hipStreamSynchronize(bt->s->stream);
  bt->graphs.clear();
  if (bt->s) lspcg_solver_destroy(bt->s);
  if (bt->Acat) lspcg_mat_destroy(bt->Acat);
  if (bt->Lcat) lspcg_mat_destroy(bt->Lcat);
  for (void* v : {(void*)bt->boff, (void*)bt->bn, (void*)bt->etile_sys, (void*)bt->tile0, (void*)bt->tk0, (void*)bt->etk0, (void*)bt->etickets, (void*)bt->gsum, (void*)bt->partials, (void*)bt->tickets, (void*)bt->S,
                  (void*)bt->dhist})
    (void)hipFree(v);
  (void)hipHostFree(bt->hS);
  (void)hipFree(bt->utab);
  if (bt->ev_u0) (void)hipEventDestroy(bt->ev_u0);
  if (bt->ev_u1) (void)hipEventDestroy(bt->ev_u1);
  delete bt;
  return LSPCG_OK;
}

int lspcg_batch_create(lspcg_ctx* ctx, int nsys, const lspcg_mat* const* A, const lspcg_mat* const* L,
                       double epsilon, lspcg_batch** out) {
  return lspcg_batch_create_precond(ctx, nsys, A, L, LSPCG_PRECOND_EXT_SPAI, epsilon, out);
}

int lspcg_batch_create_precond(lspcg_ctx* ctx, int nsys, const lspcg_mat* const* A, const lspcg_mat* const* L,
                               int precond, double epsilon, lspcg_batch** out) {
  LSPCG_CHECK(ctx && A && out && nsys >= 1, LSPCG_ERR_ARG, "batch_create: NULL argument or nsys < 1");
  LSPCG_CHECK(precond != LSPCG_PRECOND_IC, LSPCG_ERR_UNSUPPORTED,
              "batch_create: IC's triangular solves do not run in lockstep: solve one by one");
  LSPCG_CHECK(precond >= LSPCG_PRECOND_NONE && precond <= LSPCG_PRECOND_EXT_SPAI_SCALED, LSPCG_ERR_ARG,
              "batch_create: unknown preconditioner " + std::to_string(precond));
  const bool spai = precond == LSPCG_PRECOND_EXT_SPAI || precond == LSPCG_PRECOND_EXT_SPAI_SCALED;
  const bool needs_d = precond == LSPCG_PRECOND_DIAGONAL || precond == LSPCG_PRECOND_EXT_SPAI_SCALED;
  LSPCG_CHECK(spai ? L != nullptr : L == nullptr, LSPCG_ERR_ARG,
              spai ? "batch_create: the ext_spai kinds need L" : "batch_create: L must be NULL for none / diagonal");
  if (!spai) epsilon = 0.0;
  for (int k = 0; k < nsys; ++k) {
    LSPCG_CHECK(A[k] && (!spai || L[k]), LSPCG_ERR_ARG, "batch_create: NULL matrix " + std::to_string(k));
    LSPCG_CHECK(A[k]->dtype == A[0]->dtype && (!spai || L[k]->dtype == A[0]->dtype), LSPCG_ERR_ARG,
                "batch_create: every A and L must have one dtype");
    LSPCG_CHECK(A[k]->block_size == A[0]->block_size && (!spai || L[k]->block_size == A[0]->block_size), LSPCG_ERR_ARG,
                "batch_create: every A and L must have one block size");
    LSPCG_CHECK((!spai || L[k]->n == A[k]->n) && A[k]->n >= 1, LSPCG_ERR_ARG,
                "batch_create: system " + std::to_string(k) + ": L and A differ in size or are empty");
  }
  LSPCG_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<lspcg_batch, int (*)(lspcg_batch*)> bt(new lspcg_batch(), lspcg_batch_destroy);
  bt->ctx = ctx;
  bt->precond = precond;
  bt->nsys = nsys;
  bt->bs = A[0]->block_size;
  bt->dtype = A[0]->dtype;
  // block-row offsets, each system padded to whole SpMV row tiles (kSellWG block rows)
  std::vector<int64_t> brow(nsys + 1, 0);
  for (int k = 0; k < nsys; ++k) brow[k + 1] = brow[k] + (A[k]->nb + kSellWG - 1) / kSellWG * kSellWG;
  LSPCG_CHECK(brow[nsys] * bt->bs < (int64_t(1) << 31), LSPCG_ERR_ARG, "batch_create: window exceeds 2^31 rows");
  for (int k = 0; k < nsys; ++k) {
    bt->off.push_back(brow[k] * bt->bs);
    bt->n.push_back(A[k]->n);
    bt->nb.push_back(A[k]->nb);
    bt->ae0.push_back(k ? bt->ae0[k - 1] + bt->annz[k - 1] : 0);
    bt->annz.push_back(A[k]->nnzb);
    if (spai) {
      bt->le0.push_back(k ? bt->le0[k - 1] + bt->lnnz[k - 1] : 0);
      bt->lnnz.push_back(L[k]->nnzb);
    }
  }
  bt->brow = brow;
  bt->ntot = brow[nsys] * bt->bs;
  if (int rc = cat_matrices(ctx, nsys, A, brow, &bt->Acat)) return rc;
  if (spai)
    if (int rc = cat_matrices(ctx, nsys, L, brow, &bt->Lcat)) return rc;
  // one workgroup per system when every system fits the one-workgroup solve (scalar views; its
  // row and LDS bounds, small_path); LSPCG_BATCH_SMALL=0 keeps the lockstep phases.  Decided before
  // the views are built: that mode reads 4-entry-group SELL copies, not SELL-DIA
  for (int k = 0; k < nsys; ++k) bt->max_n = std::max<int64_t>(bt->max_n, bt->n[k]);
  {
    const char* e = std::getenv("LSPCG_BATCH_SMALL");
    const char* en = std::getenv("LSPCG_SMALL_N");
    const int64_t small_n = en ? std::max<int64_t>(0, std::atoll(en)) : kSmallNDefault;
    const int64_t row_cap = int64_t(kSmallThreadsBig) * 3;
    bt->small = !(e && e[0] == '0') && bt->bs == 1 && bt->max_n <= std::min<int64_t>(row_cap, small_n) &&
                3 * bt->max_n * int64_t(esize(bt->dtype)) <= kSmallLds;
  }
  if (int rc = solver_create(ctx, bt->Acat, precond, !bt->small, false, &bt->s)) return rc;
  if (spai)
    if (int rc = lspcg_solver_set_spai(bt->s, bt->Lcat, epsilon, nullptr)) return rc;
  LSPCG_CHECK(bt->s->sp[0] && (!spai || (bt->s->sp[1] && bt->s->sp[2])), LSPCG_ERR_UNSUPPORTED,
              "batch_create: no SELL view of the block-diagonal system (irregular rows): solve one by one");
  // tile maps
  const int64_t ntiles = brow[nsys] / kSellWG;
  std::vector<int32_t> esys(size_t(bt->ntot / kThreads)), t0(nsys + 1);
  for (int k = 0; k < nsys; ++k) {
    t0[k] = int32_t(brow[k] / kSellWG);
    for (int64_t e = bt->off[k] / kThreads; e < (bt->off[k] + (brow[k + 1] - brow[k]) * bt->bs) / kThreads; ++e)
      esys[size_t(e)] = k;
  }
  t0[nsys] = int32_t(ntiles);
  std::vector<int32_t> tk(nsys);
  int64_t lines = 0;
  for (int k = 0; k < nsys; ++k) {
    tk[k] = int32_t(lines);
    lines += 1 + (t0[k + 1] - t0[k] + kTicketGroup - 1) / kTicketGroup;
  }
  LSPCG_HIP(hipMalloc(&bt->tk0, sizeof(int32_t) * nsys));
  LSPCG_HIP(hipMemcpy(bt->tk0, tk.data(), sizeof(int32_t) * nsys, hipMemcpyHostToDevice));
  LSPCG_HIP(hipMalloc(&bt->etile_sys, sizeof(int32_t) * esys.size()));
  LSPCG_HIP(hipMalloc(&bt->tile0, sizeof(int32_t) * t0.size()));
  LSPCG_HIP(hipMemcpy(bt->etile_sys, esys.data(), sizeof(int32_t) * esys.size(), hipMemcpyHostToDevice));
  LSPCG_HIP(hipMemcpy(bt->tile0, t0.data(), sizeof(int32_t) * t0.size(), hipMemcpyHostToDevice));
  // partials: <= 3 dots per SpMV tile (Jacobi's init), <= 2 per elementwise tile (three-launch UR)
  const int64_t netiles = bt->ntot / kThreads;  // = ntiles * bs
  LSPCG_HIP(hipMalloc(&bt->partials, sizeof(double) * std::max<int64_t>(6 * ntiles, 4 * netiles)));
  if (!spai) {  // the three-launch UR's tickets: per system, top line + one line per kTicketGroup elementwise tiles
    std::vector<int32_t> etk(nsys);
    int64_t elines = 0;
    for (int k = 0; k < nsys; ++k) {
      etk[k] = int32_t(elines);
      elines += 1 + (int64_t(t0[k + 1] - t0[k]) * bt->bs + kTicketGroup - 1) / kTicketGroup;
    }
    LSPCG_HIP(hipMalloc(&bt->etk0, sizeof(int32_t) * nsys));
    LSPCG_HIP(hipMemcpy(bt->etk0, etk.data(), sizeof(int32_t) * nsys, hipMemcpyHostToDevice));
    LSPCG_HIP(hipMalloc(&bt->etickets, sizeof(unsigned) * kTicketStride * elines));
    LSPCG_HIP(hipMemset(bt->etickets, 0, sizeof(unsigned) * kTicketStride * elines));
  }
  // reductions: consumer sums when every system has <= 128 tiles (C5 heat, <= 117 tiles: 25.6 vs
  // 26.8 us per lockstep iteration), else per-system last arrivers (8 x Poisson 256^2, 256 tiles:
  // 47.1 vs 49.9); LSPCG_BATCH_REDUCE=0 / 1 forces either
  int max_nt = 0;
  for (int k = 0; k < nsys; ++k) max_nt = std::max(max_nt, t0[k + 1] - t0[k]);
  bt->sums = max_nt <= 128;
  if (const char* e = std::getenv("LSPCG_BATCH_REDUCE")) bt->sums = e[0] == '1';
  bt->ntiles = ntiles;
  // consumer-sum partials: init (<= 3 dots per SpMV tile) | gz (2 dots per SpMV tile from KB, or per
  // elementwise tile from the three-launch UR) | gq (1 dot per SpMV tile)
  {
    const int64_t ni = spai ? 4 * ntiles : 6 * ntiles, nz = spai ? 4 * ntiles : 4 * netiles;
    LSPCG_HIP(hipMalloc(&bt->gsum, sizeof(double) * (ni + nz + 2 * ntiles)));
    LSPCG_HIP(hipMemset(bt->gsum, 0, sizeof(double) * (ni + nz + 2 * ntiles)));
    bt->gz = bt->gsum + ni;
    bt->gq = bt->gz + nz;
  }
  if (bt->small || needs_d) {
    std::vector<int32_t> ho(nsys), hn(nsys);
    for (int k = 0; k < nsys; ++k) {
      ho[k] = int32_t(bt->off[k]);
      hn[k] = int32_t(bt->n[k]);
    }
    LSPCG_HIP(hipMalloc(&bt->boff, sizeof(int32_t) * nsys));
    LSPCG_HIP(hipMalloc(&bt->bn, sizeof(int32_t) * nsys));
    LSPCG_HIP(hipMemcpy(bt->boff, ho.data(), sizeof(int32_t) * nsys, hipMemcpyHostToDevice));
    LSPCG_HIP(hipMemcpy(bt->bn, hn.data(), sizeof(int32_t) * nsys, hipMemcpyHostToDevice));
  }
  if (needs_d)
    if (int rc = pad_d(bt.get())) return rc;
  LSPCG_HIP(hipMalloc(&bt->tickets, sizeof(unsigned) * kTicketStride * lines));
  LSPCG_HIP(hipMemset(bt->tickets, 0, sizeof(unsigned) * kTicketStride * lines));
  LSPCG_HIP(hipMalloc(&bt->S, sizeof(PcgState) * nsys));
  LSPCG_HIP(hipHostMalloc(&bt->hS, 2 * sizeof(PcgState) * nsys, hipHostMallocDefault));
  *out = bt.release();
  return LSPCG_OK;
}

int lspcg_batch_update(lspcg_batch* bt, const lspcg_mat* const* A, const lspcg_mat* const* L, double epsilon,
                       double* t_ms, int* graphs_kept) {
  LSPCG_CHECK(bt, LSPCG_ERR_ARG, "batch_update: NULL");
  if (graphs_kept) *graphs_kept = 0;
  const bool spai = bt->precond == LSPCG_PRECOND_EXT_SPAI || bt->precond == LSPCG_PRECOND_EXT_SPAI_SCALED;
  const bool needs_d = bt->precond == LSPCG_PRECOND_DIAGONAL || bt->precond == LSPCG_PRECOND_EXT_SPAI_SCALED;
  LSPCG_CHECK(spai || !L, LSPCG_ERR_ARG, "batch_update: L must be NULL for none / diagonal");
  if (!spai) epsilon = bt->s->eps;
  const int ns = bt->nsys;
  const int64_t bb = int64_t(bt->bs) * bt->bs;
  std::vector<CatSlice> tab;
  bool anyA = false, anyL = false;
  for (int pass = 0; pass < 2; ++pass) {  // every A, then every L
    const lspcg_mat* const* M = pass ? L : A;
    if (!M) continue;
    const lspcg_mat* C = pass ? bt->Lcat : bt->Acat;
    const std::vector<int64_t>& nnz = pass ? bt->lnnz : bt->annz;
    const std::vector<int64_t>& e0 = pass ? bt->le0 : bt->ae0;
    const std::string what = std::string("batch_update: ") + (pass ? "L" : "A") + " of system ";
    for (int k = 0; k < ns; ++k) {
      const lspcg_mat* m = M[k];
      if (!m) continue;
      LSPCG_CHECK(m->dtype == bt->dtype && m->storage_dtype() == bt->dtype, LSPCG_ERR_ARG,
                  what + std::to_string(k) + " has another dtype than the batch");
      LSPCG_CHECK(m->block_size == bt->bs && m->n == bt->n[k] && m->nb == bt->nb[k] && m->nnzb == nnz[k],
                  LSPCG_ERR_FORMAT,
                  what + std::to_string(k) + " has another block size, size or entry count (nothing written)");
      tab.push_back(CatSlice{m->rowptr, m->colind, m->vals, C->rowptr + bt->brow[k], C->colind + e0[k],
                             static_cast<char*>(C->vals) + esize(bt->dtype) * size_t(bb) * size_t(e0[k]), m->nb,
                             m->nnzb, m->nnzb * bb, int32_t(e0[k]), int32_t(bt->brow[k])});
      (pass ? anyL : anyA) = true;
    }
  }
  lspcg_solver* s = bt->s;
  LSPCG_HIP(hipSetDevice(bt->ctx->device));
  hipStream_t cst = bt->ctx->stream;
  const int nmat = int(tab.size());
  if (!bt->utab) {
    LSPCG_HIP(hipMalloc(&bt->utab, sizeof(CatSlice) * 2 * size_t(ns)));
    LSPCG_HIP(hipEventCreate(&bt->ev_u0));
    LSPCG_HIP(hipEventCreate(&bt->ev_u1));
  }
  LSPCG_HIP(hipEventRecord(bt->ev_u0, cst));
  // one launch of <= ~2048 workgroups over all given matrices (gridDim.y of them, the rest strided)
  int64_t most = 1;
  for (const CatSlice& d : tab) most = std::max<int64_t>(most, d.nb + 1 + std::max(d.nnzb, d.nval));
  const unsigned gy = unsigned(std::min(std::max(nmat, 1), 2048));
  const unsigned gx = unsigned(std::max<int64_t>(1, std::min<int64_t>((most + kThreads - 1) / kThreads, 2048 / gy)));
  if (nmat) {
    // the pattern check: every given matrix against its slice in one launch, one flag read.  Before it
    // has passed nothing is written, so a refused window leaves every system and every L as it was
    LSPCG_HIP(hipMemcpyAsync(bt->utab, tab.data(), sizeof(CatSlice) * nmat, hipMemcpyHostToDevice, cst));
    LSPCG_HIP(hipMemsetAsync(s->flag, 0, sizeof(int), cst));
    launch(k_cat_same_pattern, dim3(gx, gy), dim3(kThreads), cst, nmat, bt->utab, s->flag);
    LSPCG_HIP(hipGetLastError());
    int differs = 0;
    LSPCG_HIP(hipMemcpyAsync(&differs, s->flag, sizeof(int), hipMemcpyDeviceToHost, cst));
    LSPCG_HIP(hipStreamSynchronize(cst));
    LSPCG_CHECK(!differs, LSPCG_ERR_FORMAT,
                "batch_update: a given matrix has another pattern than the system it replaces (nothing written)");
  }
  LSPCG_HIP(hipStreamSynchronize(s->stream));  // a running solve reads everything rewritten below
  const GraphKey key_before = graph_key(s);
  // From here values are written and views may move: a failure drops the graphs, which hold the old
  // addresses by value, solves return its code, and the update that follows it reports none kept
  const bool after_failure = bt->update_failed;
  bt->update_failed = true;
  auto steps = [&]() -> int {
    if (nmat) {
      by_dtype(bt->dtype, [&](auto t) {
        launch(k_cat_copy_values<decltype(t)>, dim3(gx, gy), dim3(kThreads), cst, nmat, bt->utab);
        return 0;
      });
      LSPCG_HIP(hipGetLastError());
    }
    if (anyA)
      if (int rc = lspcg_solver_update_matrix(s, nullptr, nullptr)) return rc;
    const bool new_spai = spai && (anyL || epsilon != s->eps);
    if (new_spai) {  // Lcat is the installed handle and its pattern has just been checked
      s->same_L_pattern = true;
      const int rc = lspcg_solver_set_spai(s, bt->Lcat, epsilon, nullptr);
      s->same_L_pattern = false;
      if (rc) return rc;
    }
    if (needs_d && (anyA || new_spai))  // both recompute d = diag(A), 0 on padding rows
      if (int rc = pad_d(bt)) return rc;
    float ms = 0.f;
    LSPCG_HIP(hipEventRecord(bt->ev_u1, cst));
    LSPCG_HIP(hipEventSynchronize(bt->ev_u1));
    LSPCG_HIP(hipEventElapsedTime(&ms, bt->ev_u0, bt->ev_u1));
    if (t_ms) *t_ms = ms;
    return LSPCG_OK;
  };
  if (int rc = steps()) {
    bt->graphs.clear();
    bt->update_rc = rc;
    return rc;
  }
  bt->update_failed = false;
  bt->update_rc = LSPCG_OK;
  const bool kept = !after_failure && graph_key(s) == key_before;
  if (!kept) bt->graphs.clear();
  if (graphs_kept) *graphs_kept = kept ? 1 : 0;
  return LSPCG_OK;
}

int lspcg_batch_solve(lspcg_batch* bt, const void* const* b, void* const* x, double rtol, int64_t max_iter,
                      int64_t* iters, int32_t* status, double* const* res_hist, double* t_solve_ms) {
  return lspcg_batch_solve_coef(bt, b, x, rtol, max_iter, iters, status, res_hist, t_solve_ms, nullptr);
}

int lspcg_batch_solve_coef(lspcg_batch* bt, const void* const* b, void* const* x, double rtol, int64_t max_iter,
                           int64_t* iters, int32_t* status, double* const* res_hist, double* t_solve_ms,
                           double* const* coef) {
  LSPCG_CHECK(bt && b && x && iters && status, LSPCG_ERR_ARG, "batch_solve: NULL argument");
  const int ns = bt->nsys;
  for (int k = 0; k < ns; ++k) LSPCG_CHECK(b[k] && x[k], LSPCG_ERR_ARG, "batch_solve: NULL vector " + std::to_string(k));
  if (bt->update_failed) {
    set_error("batch_solve: the last lspcg_batch_update failed and left views that may have moved; update again first");
    return bt->update_rc;
  }
  lspcg_solver* s = bt->s;
  LSPCG_HIP(hipSetDevice(bt->ctx->device));
  hipStream_t st = s->stream;
  const size_t es = esize(bt->dtype);
  std::vector<int64_t> mi(ns), hoff(ns + 1, 0), coff(ns + 1, 0);
  for (int k = 0; k < ns; ++k) {
    mi[k] = max_iter > 0 ? max_iter : bt->n[k];
    hoff[k + 1] = hoff[k] + ((res_hist && res_hist[k]) ? mi[k] + 2 : 0);
  }
  // the recorded (ρ_k, π_k) pairs follow the histories in the same buffer, at even offsets (16-B stores)
  coff[0] = (hoff[ns] + 1) / 2 * 2;
  for (int k = 0; k < ns; ++k) coff[k + 1] = coff[k] + ((coef && coef[k]) ? 2 * (mi[k] + 1) : 0);
  if (int rc = grow_hist(&bt->dhist, &bt->dhist_cap, coff[ns], st)) return rc;
  std::unique_lock<std::mutex> sub(submit_mutex());  // as in lspcg_solver_solve
  LSPCG_HIP(hipEventRecord(s->ev_in, bt->ctx->stream));
  LSPCG_HIP(hipStreamWaitEvent(st, s->ev_in, 0));
  LSPCG_HIP(hipEventRecord(s->ev_t0, st));
  char* cb = static_cast<char*>(s->b);
  char* cx = static_cast<char*>(s->x);
  for (int k = 0; k < ns; ++k) {  // padding rows stay 0 (zeroed at creation, never written)
    LSPCG_HIP(hipMemcpyAsync(cb + es * bt->off[k], b[k], es * bt->n[k], hipMemcpyDeviceToDevice, st));
    LSPCG_HIP(hipMemcpyAsync(cx + es * bt->off[k], x[k], es * bt->n[k], hipMemcpyDeviceToDevice, st));
  }
  for (int k = 0; k < ns; ++k)
    bt->hS[k] = initial_state(rtol, s->eps, (res_hist && res_hist[k]) ? bt->dhist + hoff[k] : nullptr, mi[k],
                              (coef && coef[k]) ? bt->dhist + coff[k] : nullptr);
  LSPCG_HIP(hipMemcpyAsync(bt->S, bt->hS, sizeof(PcgState) * ns, hipMemcpyHostToDevice, st));
  int rc = by_dtype(bt->dtype, [&](auto t) { return enqueue_batch_init<decltype(t)>(bt, st); });
  if (rc) return rc;

  // every system's state through the poll loop (small mode: one launch)
  StatePoll poll{ns, bt->S, bt->hS, {s->ev_poll, s->ev_poll2}, st, sub};
  std::vector<PcgState> cur(ns);
  if (bt->small) {  // every system in its own workgroup: the whole loop in one launch
    rc = by_dtype(bt->dtype, [&](auto t) {
      return launch_pcg_small<decltype(t)>(bt->precond, ns, s, bt->max_n, bt->S, bt->boff, bt->bn, st);
    });
    if (!rc) rc = poll.post();
    if (!rc) rc = poll.take(cur.data());
  } else {
    auto one = [&] { return by_dtype(bt->dtype, [&](auto t) { return enqueue_batch_iteration<decltype(t)>(bt, st); }); };
    rc = poll.run(mi.data(), 32, [&](int c) { return bt->graphs.launch(st, c, one); }, cur.data());
  }
  if (rc) return rc;
  by_dtype(bt->dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_batch_x_fixup<T>, dim3(unsigned(bt->ntot / kThreads)), dim3(kThreads), st, batch_map(bt), bt->S,
           as<T>(s->p), as<T>(s->x));
    return 0;
  });
  LSPCG_HIP(hipGetLastError());
  for (int k = 0; k < ns; ++k) {
    const char* src = (cur[k].bb == 0.0) ? cb : cx;  // scipy returns b when ‖b‖ = 0
    LSPCG_HIP(hipMemcpyAsync(x[k], src + es * bt->off[k], es * bt->n[k], hipMemcpyDeviceToDevice, st));
  }
  LSPCG_HIP(hipEventRecord(s->ev_t1, st));
  LSPCG_HIP(hipEventRecord(s->ev_out, st));
  LSPCG_HIP(hipStreamWaitEvent(bt->ctx->stream, s->ev_out, 0));
  LSPCG_HIP(poll.wait(s->ev_t1));
  float ms = 0.f;
  LSPCG_HIP(hipEventElapsedTime(&ms, s->ev_t0, s->ev_t1));
  if (t_solve_ms) *t_solve_ms = ms;
  return report_states(ns, cur.data(), mi.data(), bt->dhist, hoff.data(), iters, status, res_hist, coff.data(), coef);
}

}  // extern "C"
