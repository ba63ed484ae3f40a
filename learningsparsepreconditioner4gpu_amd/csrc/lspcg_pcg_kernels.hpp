// Device code of the PCG loop shared by the single-system solver (lspcg_pcg.hip), the batched
// lockstep solver (lspcg_batch.hip) and solve_multi (lspcg_multi.hip): the SpMV prologues, the row
// bodies of every phase's epilogue and their compositions with a way of finishing the dots, the
// update kernels and the one-workgroup solve -- templates only, so that each unit instantiates what
// it launches.  The loop's state and scipy's scalar recurrence are in lspcg_pcg_step.hpp; every
// kernel and epilogue here calls it.  Schedules: lspcg_pcg.hip's header and DESIGN.md §5.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "lspcg_internal.hpp"
#include "lspcg_pcg_step.hpp"
#include "lspcg_sell.hpp"
#include "lspcg_spmv.hpp"

namespace lspcg {

// the top-of-loop test as a launch's prologue (k_update_p of the last-arriver schedules)
template <typename T>
struct ProCheck {
  PcgState* S;
  __device__ __forceinline__ bool exit() const {
    if (S->done) return true;
    const int code = loop_test<T>(S->iter, S->max_iter, S->rr, S->atol);
    if (code && blockIdx.x == 0 && threadIdx.x == 0) S->done = code;
    return code != 0;
  }
};

struct ProDone {
  const PcgState* S;
  __device__ __forceinline__ bool exit() const { return S->done != 0; }
};

// KA (ext_spai): t = Lᵀ r  (scaled variant: t = (Lᵀ r)/d)
template <typename T, bool SCALED>
struct EpiT {
  static constexpr int NDOT = 0;
  T* t;
  const T* d;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, T s, DD*) const {
    if constexpr (SCALED) gst(t + i, s / gld(d + i));
    else gst(t + i, s);
  }
  __device__ __forceinline__ void fin(const double*) const {}
};

// ---- epilogues = a phase's row body x a way of finishing its dots ---------------------------
// Row bodies (what a row's SpMV sum s becomes, and the row's terms of the phase's dots).  Where the
// SELL kernels can load the row's own entry before its gathers, the body has prefetch() / row_pf()
// (lspcg_sell.hpp; used where the composed epilogue sets PREFETCH).

// init: r_0 = b - A x0 ; ‖r_0‖², ‖b‖² (+ z_0 = r_0/d, ρ_0 = r_0·z_0 for Jacobi)
// (scipy: r = b - matvec(x) if x.any() else b.copy(); with x0 = 0 the subtraction returns b)
template <typename T, int PRE>
struct RowResid {
  static constexpr int NDOT = PRE == LSPCG_PRECOND_DIAGONAL ? 3 : 2;
  T* r;
  const T* b;
  const T* d;
  T* z;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, T s, DD* dots) const {
    const T bi = gld(b + i);
    const T ri = bi - s;
    gst(r + i, ri);
    dd_fma(dots[0], double(ri), double(ri));
    dd_fma(dots[1], double(bi), double(bi));
    if constexpr (PRE == LSPCG_PRECOND_DIAGONAL) {
      const T zi = ri / gld(d + i);
      gst(z + i, zi);
      dd_fma(dots[2], double(ri), double(zi));
    }
  }
};

// KB: z = L t + ε r  (scaled: z = L t + (ε r)/d);  ρ = r·z and ‖r‖² in the same reduction
template <typename T, bool SCALED>
struct RowZ {
  static constexpr int NDOT = 2;
  T* z;
  const T* r;
  const T* d;
  T eps;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ T prefetch(int64_t i) const { return gld(r + i); }
  __device__ __forceinline__ void row_pf(int64_t i, T s, DD* dots, T ri) const {
    T zi;
    if constexpr (SCALED) zi = s + (eps * ri) / gld(d + i);
    else zi = s + eps * ri;
    gst(z + i, zi);
    dd_fma(dots[0], double(ri), double(zi));
    dd_fma(dots[1], double(ri), double(ri));
  }
  __device__ __forceinline__ void row(int64_t i, T s, DD* dots) const { row_pf(i, s, dots, prefetch(i)); }
};

// KC / KD: q = A p ; π = p·q
template <typename T>
struct RowQ {
  static constexpr int NDOT = 1;
  T* q;
  const T* p;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ T prefetch(int64_t i) const { return gld(p + i); }
  __device__ __forceinline__ void row_pf(int64_t i, T s, DD* dots, T pi) const {
    gst(q + i, s);
    dd_fma(dots[0], double(pi), double(s));
  }
  __device__ __forceinline__ void row(int64_t i, T s, DD* dots) const { row_pf(i, s, dots, prefetch(i)); }
};

// Finishing way 1: the launch's last arriver sums the workgroup partials (grid_reduce_dd) and runs
// the composed epilogue's fin(values) on the state.
struct ByLastArriver {
  PcgState* S;
  double* partials;
  unsigned* ticket;
};

// Finishing way 2: the launch only pre-reduces per group of workgroups (grid_partial_groups); the
// elementwise launches that consume the scalars sum the group totals -- the split schedules
// (DESIGN.md "PCG schedule") and the batch's consumer-sum mode.  PF: the SELL kernels prefetch the
// row's own entry (measured per phase: set for z when not scaled, and for q).
struct ByGroups {
  static constexpr bool GROUPS = true;
  double* partials;
  unsigned* ticket;
  double* group_out;
  int gsz;
  __device__ __forceinline__ void fin(const double*) const {}
};
template <class Row, bool PF = false>
struct EpiGroups : Row, ByGroups {
  static constexpr bool PREFETCH = PF;
};
template <typename T, bool SCALED>
using EpiZG = EpiGroups<RowZ<T, SCALED>, !SCALED>;
template <typename T>
using EpiQG = EpiGroups<RowQ<T>, true>;

// (way 3, the batch's per-system last arrivers: lspcg_batch.hip)

// KB of the last-arriver schedule (the top-of-loop test on ‖r_k‖ then runs in the p update;
// r_0's norm comes from the init)
template <typename T, bool SCALED>
struct EpiZ : RowZ<T, SCALED>, ByLastArriver {
  __device__ __forceinline__ void fin(const double* v) const {
    const int64_t k = S->iter;
    const double rho_old = S->rho;
    double* const hist = S->hist;
    keep_z<T>(S, k, rho_old, hist, v[0], v[1]);
  }
};

// KD of the last-arriver schedule (INC: this launch also completes the iteration -- ext_spai,
// whose r update carries no reduction)
template <typename T, bool INC = false>
struct EpiQ : RowQ<T>, ByLastArriver {
  __device__ __forceinline__ void fin(const double* v) const {
    double* const coef = S->coef;
    // not INC: the r update counts the iteration after this launch, and only a recorded pair needs k
    const int64_t k = (INC || coef) ? S->iter : 0;
    keep_q<T, INC>(S, k, coef, S->rho, v[0]);
  }
};

template <typename T, int PRE>
struct EpiResid : RowResid<T, PRE>, ByLastArriver {
  __device__ __forceinline__ void fin(const double* v) const {
    const double rtol = S->rtol;
    double* const hist = S->hist;
    init_state<T>(S, rtol, hist, v[0], v[1], v[PRE == LSPCG_PRECOND_DIAGONAL ? 2 : 0]);
  }
};

// ---- elementwise kernels: 16-B vectors, 2 vectors per lane, grid <= kReduceGridMax
template <typename T>
struct VecT {
  static constexpr int W = 16 / sizeof(T);
  using type = T __attribute__((ext_vector_type(W)));
};
constexpr int kElemUnroll = 2;

template <typename T>
static int elem_vec_grid(int64_t n) {
  const int64_t nv = n / VecT<T>::W;
  const int64_t g = (nv + int64_t(kThreads) * kElemUnroll - 1) / (int64_t(kThreads) * kElemUnroll);
  return int(std::max<int64_t>(1, std::min<int64_t>(g, kReduceGridMax)));
}

// KC: x += α_{k-1} p_{k-1} (deferred, k > 0) ; p_k = p_{k-1}β + z (scipy `p *= beta; p += z`),
// p_0 = z.  `Pro` = ProCheck (the top-of-loop test) in every last-arriver schedule.
template <typename T, typename Pro>
__global__ void __launch_bounds__(kThreads) k_update_p(int64_t n, Pro pro, const PcgState* S,
                                                       const T* __restrict__ z, T* __restrict__ p,
                                                       T* __restrict__ x) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  if (pro.exit()) return;
  const bool first = S->iter == 0;
  const T beta = first ? T(0) : T(S->rho) / T(S->rho_prev);
  const T alpha = T(S->alpha);
  const int64_t nv = n / W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  for (int64_t j0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j0 < nv; j0 += ts * kElemUnroll) {
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
        if (!first) reinterpret_cast<V*>(x)[j] = xx[u] + alpha * pp[u];
        reinterpret_cast<V*>(p)[j] = first ? zz[u] : (pp[u] * beta) + zz[u];
      }
    }
  }
  for (int64_t i = nv * W + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += ts) {
    const T pi = p[i];
    if (!first) x[i] = x[i] + alpha * pi;
    p[i] = first ? z[i] : (pi * beta) + z[i];
  }
}

// The per-row body of an r update that reduces: ri = r_{k+1}[i] (already stored) adds its term to
// ‖r_{k+1}‖², Jacobi stores z = r/d and adds to ρ_{k+1} = r·z; BOTH: without a preconditioner ρ is
// accumulated too (= r·r, for consumers that read the two sums side by side).
template <typename T, int PRE, bool BOTH>
__device__ __forceinline__ void r_dots_row(int64_t i, T ri, const T* __restrict__ d, T* __restrict__ z, DD& rr,
                                           DD& rho) {
  dd_fma(rr, double(ri), double(ri));
  if constexpr (PRE == LSPCG_PRECOND_DIAGONAL) {
    const T zi = ri / d[i];
    z[i] = zi;
    dd_fma(rho, double(ri), double(zi));
  } else if constexpr (BOTH) {
    dd_fma(rho, double(ri), double(ri));
  }
}

// KE: r -= α q ; ‖r‖² (+ Jacobi z = r/d, ρ = r·z) ; iteration count
template <typename T, int PRE>
__global__ void __launch_bounds__(kThreads) k_update_r(int64_t n, PcgState* S, const T* __restrict__ q,
                                                       T* __restrict__ r, const T* __restrict__ d, T* __restrict__ z,
                                                       double* partials, unsigned* ticket) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  constexpr int ND = PRE == LSPCG_PRECOND_DIAGONAL ? 2 : 1;
  if (S->done) return;
  const T alpha = T(S->alpha);
  DD dots[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) dots[j] = dd_zero();
  const int64_t nv = n / W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  auto elem = [&](T ri, int64_t i) { r_dots_row<T, PRE, false>(i, ri, d, z, dots[0], dots[ND - 1]); };
  for (int64_t j0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j0 < nv; j0 += ts * kElemUnroll) {
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
        const V rn = rr[u] - alpha * qq[u];
        reinterpret_cast<V*>(r)[j] = rn;
#pragma unroll
        for (int w = 0; w < W; ++w) elem(rn[w], j * W + w);
      }
    }
  }
  for (int64_t i = nv * W + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += ts) {
    const T ri = r[i] - alpha * q[i];
    r[i] = ri;
    elem(ri, i);
  }
  grid_reduce_dd<ND>(dots, partials, ticket, [&](const double* v) {
    constexpr bool RHO = PRE == LSPCG_PRECOND_NONE || PRE == LSPCG_PRECOND_DIAGONAL;  // IC: k_dot_rho
    const int64_t it = S->iter + 1;
    const double rho_old = RHO ? S->rho : 0.0;
    double* const hist = S->hist;
    S->iter = it;
    keep_r<T, RHO>(S, it, rho_old, hist, v[0], v[ND - 1]);
  });
}

// ext_spai: r -= α q only (‖r‖² is reduced by the next L SpMV, the iteration count by KC)
template <typename T>
__global__ void __launch_bounds__(kThreads) k_update_r_nodot(int64_t n, const PcgState* S, const T* __restrict__ q,
                                                             T* __restrict__ r) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  if (S->done) return;
  const T alpha = T(S->alpha);
  const int64_t nv = n / W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  for (int64_t j0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j0 < nv; j0 += ts * kElemUnroll) {
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
      if (j < nv) reinterpret_cast<V*>(r)[j] = rr[u] - alpha * qq[u];
    }
  }
  for (int64_t i = nv * W + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += ts) r[i] = r[i] - alpha * q[i];
}

// ---- split-reduction ext_spai schedule (SELL views; DESIGN.md "PCG schedule") --------------
// KB and KC only pre-reduce their dot partials per group of workgroups (grid_partial_groups);
// the elementwise launches that consume the scalars sum the <= 64 group totals themselves:
//   KA  t = Lᵀ r_k
//   KB  z = L t + ε r_k ; groups of ρ_k = r_k·z and ‖r_k‖²                 -> GZ
//   UP  ρ_k, ‖r_k‖ from GZ ; top-of-loop test ; x += α_{k-1} p_{k-1} ; p_k = p_{k-1}β + z
//   KC  q = A p_k ; groups of π_k = p_k·q                                  -> GQ
//   UR  α_k = ρ_k/π_k from GZ, GQ ; r_{k+1} = r_k - α_k q ; persists ρ_k, α_k, iteration k+1
// Workgroup 0 of UP / UR is the only writer of the persistent state, which only later launches
// read; every workgroup computes the same scalars (same group totals, same summation tree).
// UP.  The first chunk's vector loads are issued before the group sums, so their latency overlaps
// the scalar reduction instead of following it.  x is read and written with non-temporal accesses:
// nothing else in the iteration touches it, and streaming it past the caches keeps its 8 B per row
// out of the loop's Infinity-Cache working set (kuhn101: 69.2 vs 71.0 us per iteration,
// tools/loop_ab.py, profiles/r4_loop_ab_v1.jsonl).
template <typename T>
__global__ void __launch_bounds__(kThreads) k_update_p_g(int64_t n, PcgState* S, const double* __restrict__ gz, int ngz,
                                                         const T* __restrict__ z, T* __restrict__ p,
                                                         T* __restrict__ x) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  const int64_t nv = n / W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  const int64_t jt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  V zz[kElemUnroll], pp[kElemUnroll], xx[kElemUnroll];
  auto load = [&](int64_t j0) {
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        zz[u] = reinterpret_cast<const V*>(z)[j];
        pp[u] = reinterpret_cast<const V*>(p)[j];
        xx[u] = __builtin_nontemporal_load(reinterpret_cast<const V*>(x) + j);
      }
    }
  };
  // the first chunk, the group totals and every state field are all loaded before the first test:
  // one memory latency instead of a state read followed by the loads (the state fields are read
  // into registers up front -- workgroup 0's state stores below would otherwise order the later
  // ρ_{k-1} / α_{k-1} reads after them, a second scalar round trip for every wave)
  load(jt);
  const int32_t done = S->done;
  const int64_t k = S->iter;
  const int64_t max_iter = S->max_iter;
  const double atol = S->atol, rr0 = S->rr, rho_prev = S->rho, alpha_prev = S->alpha;
  double* const hist = S->hist;
  double v[2];
  group_sum_dd<2>(gz, ngz, v);
  if (done) return;
  const double rho = round_to<T>(v[0]);
  const double rr = k > 0 ? round_to<T>(v[1]) : rr0;  // ‖r_0‖² from the init launch
  const int code = loop_test<T>(k, max_iter, rr, atol);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    keep_rr<T>(S, k, hist, rr);
    if (code) S->done = code;
    else S->rho_k = rho;
  }
  if (code) return;
  const bool first = k == 0;
  const T beta = first ? T(0) : T(rho) / T(rho_prev);  // ρ_{k-1}
  const T alpha = T(alpha_prev);                        // α_{k-1}
  for (int64_t j0 = jt; j0 < nv; j0 += ts * kElemUnroll) {
    if (j0 != jt) load(j0);
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        if (!first) __builtin_nontemporal_store(xx[u] + alpha * pp[u], reinterpret_cast<V*>(x) + j);
        reinterpret_cast<V*>(p)[j] = first ? zz[u] : (pp[u] * beta) + zz[u];
      }
    }
  }
  for (int64_t i = nv * W + jt; i < n; i += ts) {
    const T pi = p[i];
    if (!first) x[i] = x[i] + alpha * pi;
    p[i] = first ? z[i] : (pi * beta) + z[i];
  }
}

// UR (first chunk loaded before the group sum, as in UP).  ρ_k is read from the state, where UP's
// workgroup 0 stored the value every UP workgroup summed from KB's groups (one scalar load instead
// of a second group sum here; the same bits).
template <typename T>
__global__ void __launch_bounds__(kThreads) k_update_r_g(int64_t n, PcgState* S, const double* __restrict__ gq,
                                                         int ngq, const T* __restrict__ q, T* __restrict__ r) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  const int64_t nv = n / W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  const int64_t jt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  V rr[kElemUnroll], qq[kElemUnroll];
  auto load = [&](int64_t j0) {
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        rr[u] = reinterpret_cast<const V*>(r)[j];
        qq[u] = reinterpret_cast<const V*>(q)[j];
      }
    }
  };
  load(jt);  // first chunk, group totals and state line together (as in UP)
  const int32_t done = S->done;
  const int64_t k = S->iter;
  const double rho_prev = S->rho;
  const double rho = S->rho_k;
  double* const coef = S->coef;
  double vq[1];
  group_sum_dd<1>(gq, ngq, vq);
  if (done) return;
  const double pq = round_to<T>(vq[0]);
  const T alpha = T(rho) / T(pq);
  if (blockIdx.x == 0 && threadIdx.x == 0) commit_step<T>(S, coef, rho_prev, rho, pq, alpha, k + 1);
  for (int64_t j0 = jt; j0 < nv; j0 += ts * kElemUnroll) {
    if (j0 != jt) load(j0);
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) reinterpret_cast<V*>(r)[j] = rr[u] - alpha * qq[u];
    }
  }
  for (int64_t i = nv * W + jt; i < n; i += ts) r[i] = r[i] - alpha * q[i];
}

// UR of the split CG / Jacobi schedule (no preconditioner or the diagonal one): as k_update_r_g --
// α_k = ρ_k/π_k from KC's groups, r_{k+1} = r_k - α_k q -- plus, for the next iteration's UP, the
// groups of ρ_{k+1} = r·z (z = r / d for Jacobi; r·r without a preconditioner) and ‖r_{k+1}‖², the
// dots the ext_spai schedule takes from KB.
template <typename T, int PRE>
__global__ void __launch_bounds__(kThreads) k_update_r_gd(int64_t n, PcgState* S, const double* __restrict__ gq,
                                                          int ngq, const T* __restrict__ q, T* __restrict__ r,
                                                          const T* __restrict__ d, T* __restrict__ z,
                                                          double* partials, unsigned* ticket, int gsz,
                                                          double* __restrict__ gz) {
  using V = typename VecT<T>::type;
  constexpr int W = VecT<T>::W;
  const int64_t nv = n / W;
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  const int64_t jt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  V rr[kElemUnroll], qq[kElemUnroll];
  auto load = [&](int64_t j0) {
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        rr[u] = reinterpret_cast<const V*>(r)[j];
        qq[u] = reinterpret_cast<const V*>(q)[j];
      }
    }
  };
  load(jt);  // first chunk, group totals and state line together (as in UP)
  const int32_t done = S->done;
  const int64_t k = S->iter;
  const double rho_prev = S->rho;
  const double rho = S->rho_k;
  double* const coef = S->coef;
  double vq[1];
  group_sum_dd<1>(gq, ngq, vq);
  if (done) return;  // uniform: UP exits too, nobody reads the groups
  const double pq = round_to<T>(vq[0]);
  const T alpha = T(rho) / T(pq);
  if (blockIdx.x == 0 && threadIdx.x == 0) commit_step<T>(S, coef, rho_prev, rho, pq, alpha, k + 1);
  DD dots[2] = {dd_zero(), dd_zero()};  // ρ_{k+1}, ‖r_{k+1}‖²
  auto elem = [&](T ri, int64_t i) { r_dots_row<T, PRE, true>(i, ri, d, z, dots[1], dots[0]); };
  for (int64_t j0 = jt; j0 < nv; j0 += ts * kElemUnroll) {
    if (j0 != jt) load(j0);
#pragma unroll
    for (int u = 0; u < kElemUnroll; ++u) {
      const int64_t j = j0 + u * ts;
      if (j < nv) {
        const V rn = rr[u] - alpha * qq[u];
        reinterpret_cast<V*>(r)[j] = rn;
#pragma unroll
        for (int c = 0; c < W; ++c) elem(rn[c], j * W + c);
      }
    }
  }
  for (int64_t i = nv * W + jt; i < n; i += ts) {
    const T ri = r[i] - alpha * q[i];
    r[i] = ri;
    elem(ri, i);
  }
  grid_partial_groups<2>(dots, partials, ticket, gsz, gz);
}

// ---- small systems: the whole solve in ONE workgroup --------------------------------------
// Below a few thousand unknowns an iteration of the multi-kernel schedules is 5 dependent
// launches of almost no work (~16 us per iteration at n = 900).  k_pcg_small runs
// scipy's loop (iterative.py:359-418) in one 512-thread workgroup, the phases separated by
// workgroup barriers instead of kernel boundaries.  Thread `tid` owns rows tid + 512 m (m < R):
// their x, r, z, p, q live in registers; the three gathered vectors (r for Lᵀ, t for L, p for A)
// are mirrored in LDS, so a row sum's gathers are LDS reads and its global loads (the row's
// column indices and values, L2-resident after the first iteration) are independent of the
// iteration and issued 8 at a time.  Expressions are those of the split schedule: row sums in
// CSR index order (scipy's csr_matvec), T arithmetic, compensated dots rounded to T, the same
// top-of-loop test and history; x's last update is left to k_x_fixup (x and p are stored at the
// end).  The loop is bounded by max_iter, so every launch ends.
struct CsrView {
  const int32_t* rp;
  const int32_t* ci;
  const void* v;
  int f32;  // values stored as fp32 (compact view of an fp32-exact fp64 matrix, or T = float)
  // the solver's SELL-64 copy of the same view (lspcg_sell.hpp) when gp != nullptr: lane-major
  // 4-entry groups, so a wave's row loads are contiguous 16-B accesses (the CSR row-per-lane
  // loads touch ~12 cache lines per instruction and bound the one-CU solve on L1/L2 requests)
  const int32_t* gp;
  const void* scol;
  const void* sv;
  int sf32;
  int cmode;             // SELL column storage: 0 int32, 1 16-bit offsets
};

constexpr int kSmallThreads = 512;  // 2 waves per SIMD: the compensated reductions are VALU work
constexpr int kSmallThreadsBig = 1024;  // n > 1024: 4 waves per SIMD keep rows per thread <= 3
constexpr int64_t kSmallLds = 61440;  // dynamic LDS: 3 gathered vectors
constexpr int64_t kSmallNDefault = 3072;  // LSPCG_SMALL_N default
constexpr int kSmallQB = 2;  // SELL groups (4 entries each) loaded per wait (4 measured slower: 13.0 vs 9.8 us per iteration)

// row i; [b, e): its CSR entry range, or (SELL) its slice's group range; gx(c) reads the
// gathered vector (LDS in the one-workgroup solve)
template <typename T, int QB, class Gx>
__device__ __forceinline__ T sell_row(const CsrView& M, int32_t b, int32_t e, int32_t i, Gx gx) {
  T acc = T(0);
  if (M.gp) {
    const int32_t lane = i & 63, base = i & ~63;
    for (int32_t q0 = b; q0 < e; q0 += QB) {
      T v[4 * QB];
      int32_t c[4 * QB];
      bool ok[4 * QB];
#pragma unroll
      for (int u = 0; u < QB; ++u) {
        const size_t off = 256 * size_t(min(q0 + u, e - 1)) + 4 * lane;
        if (M.sf32) {
          const f32x4 a = *(const __attribute__((address_space(1))) f32x4*)(static_cast<const float*>(M.sv) + off);
          v[4 * u + 0] = T(a.x); v[4 * u + 1] = T(a.y); v[4 * u + 2] = T(a.z); v[4 * u + 3] = T(a.w);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[4 * u + j] = gld(static_cast<const T*>(M.sv) + off + j);
        }
        int o[4];
        if (M.cmode == 1) {
          const i16x4 cc = *(const __attribute__((address_space(1))) i16x4*)(static_cast<const int16_t*>(M.scol) + off);
          o[0] = cc.x; o[1] = cc.y; o[2] = cc.z; o[3] = cc.w;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ok[4 * u + j] = o[j] != kSellPad16 && q0 + u < e;
            c[4 * u + j] = ok[4 * u + j] ? base + o[j] : i;  // masked slots gather the row's own entry
          }
        } else {
          const i32x4 cc = *(const __attribute__((address_space(1))) i32x4*)(static_cast<const int32_t*>(M.scol) + off);
          o[0] = cc.x; o[1] = cc.y; o[2] = cc.z; o[3] = cc.w;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ok[4 * u + j] = o[j] >= 0 && q0 + u < e;
            c[4 * u + j] = ok[4 * u + j] ? o[j] : i;
          }
        }
      }
      T xv[4 * QB];
#pragma unroll
      for (int u = 0; u < 4 * QB; ++u) xv[u] = gx(c[u]);
#pragma unroll
      for (int u = 0; u < 4 * QB; ++u)
        if (ok[u]) acc = acc + v[u] * xv[u];
    }
    return acc;
  }
  for (int32_t k0 = b; k0 < e; k0 += 8) {
    int32_t c[8];
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int32_t k = min(k0 + u, e - 1);
      c[u] = gld(M.ci + k);
      v[u] = M.f32 ? T(gld(static_cast<const float*>(M.v) + k)) : gld(static_cast<const T*>(M.v) + k);
    }
    T xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) xv[u] = gx(c[u]);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k0 + u < e) acc = acc + v[u] * xv[u];
  }
  return acc;
}

// row i (global index) of M with the gathered vector mirrored in LDS from global row `off` on
template <typename T>
__device__ __forceinline__ T small_row(const CsrView& M, int32_t b, int32_t e, int32_t i, const T* xs, int32_t off) {
  return sell_row<T, kSmallQB>(M, b, e, i, [xs, off](int32_t c) { return xs[c - off]; });
}

// fixed-order workgroup sum of N compensated dots, rounded to T, returned to every thread: wave
// butterflies, one barrier, then every wave sums the 8 wave totals with an 8-lane butterfly and
// takes lane 0's (one LDS round trip instead of a serial sum in thread 0 and a broadcast).  `lds`
// is written again only after later barriers (each reduction site has its own buffer).
template <typename T, int N, int TH>
__device__ __forceinline__ void small_dots(DD (&v)[N], DD* lds, double (&out)[N]) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  wave_reduce_dd<N>(v);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) lds[wid * N + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) {
    DD a = lane < TH / 64 ? lds[lane * N + j] : dd_zero();
#pragma unroll
    for (int m = 1; m < TH / 64; m <<= 1) a = dd_add(a, dd_shfl_xor(a, m));
    out[j] = round_to<T>(dd_value(DD{__shfl(a.s, 0, 64), __shfl(a.c, 0, 64)}));
  }
}

// boff / bn (batched solves, lspcg_batch_solve): workgroup k solves system k of a block-diagonal
// window -- rows [boff[k], boff[k] + bn[k]) of the views and vectors, state S[k]; nullptr: the one
// system of n rows.
template <typename T, int PRE, int R, int TH>
__global__ void __launch_bounds__(TH) k_pcg_small(int32_t n, PcgState* S, CsrView A, CsrView L, CsrView LT,
                                                  const T* __restrict__ d, T* x, T* r, T* p,
                                                  const int32_t* __restrict__ boff, const int32_t* __restrict__ bn) {
  constexpr bool SPAI = PRE == LSPCG_PRECOND_EXT_SPAI || PRE == LSPCG_PRECOND_EXT_SPAI_SCALED;
  constexpr bool SCALED = PRE == LSPCG_PRECOND_EXT_SPAI_SCALED;
  int32_t off = 0;
  if (boff) {
    off = boff[blockIdx.x];
    n = bn[blockIdx.x];
    S += blockIdx.x;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char small_lds[];
  T* rs = reinterpret_cast<T*>(small_lds);
  T* ts = rs + n;
  T* ps = ts + n;
  __shared__ DD lds_z[TH / 64 * 2];
  __shared__ DD lds_q[TH / 64];
  if (S->done) return;  // ‖b‖ = 0 (init)
  const int tid = threadIdx.x;
  const T eps = T(S->eps);
  const double atol = S->atol;
  const int64_t max_iter = S->max_iter;
  double* hist = S->hist;
  double* const coef = S->coef;
  const double rr0 = S->rr;
  double rho_prev = S->rho, rho = S->rho, pq = S->pq;
  T alpha = T(S->alpha);
  int64_t k = S->iter;
  int code = 0;
  bool own[R];
  int32_t row[R], ab[R], ae[R], lb[R], le[R], tb[R], te[R];
  T xr[R], rr_[R], pr[R], dr[R];
#pragma unroll
  for (int m = 0; m < R; ++m) {
    row[m] = tid + TH * m;
    own[m] = row[m] < n;
    const int32_t i = off + (own[m] ? row[m] : 0);  // global row
    auto range = [&](const CsrView& M, int32_t& b, int32_t& e) {  // CSR entries or SELL groups
      const int32_t* rp = M.gp ? M.gp : M.rp;
      const int32_t j = M.gp ? (i >> 6) : i;
      b = rp[j];
      e = own[m] ? rp[j + 1] : b;
    };
    range(A, ab[m], ae[m]);
    if constexpr (SPAI) {
      range(L, lb[m], le[m]);
      range(LT, tb[m], te[m]);
    }
    xr[m] = own[m] ? x[i] : T(0);
    rr_[m] = own[m] ? r[i] : T(0);
    pr[m] = T(0);
    if constexpr (SCALED || PRE == LSPCG_PRECOND_DIAGONAL) dr[m] = own[m] ? d[i] : T(1);
    if (own[m]) rs[row[m]] = rr_[m];
  }
  __syncthreads();
  for (;; ++k) {
    // z = M⁻¹ r ; ρ_k = r·z ; ‖r_k‖²
    if constexpr (SPAI) {
#pragma unroll
      for (int m = 0; m < R; ++m) {
        if (!own[m]) continue;
        const T s = small_row<T>(LT, tb[m], te[m], off + row[m], rs, off);
        if constexpr (SCALED) ts[row[m]] = s / dr[m];
        else ts[row[m]] = s;
      }
      __syncthreads();
    }
    DD dz[2] = {dd_zero(), dd_zero()};
    T zr[R];
#pragma unroll
    for (int m = 0; m < R; ++m) {
      const T ri = rr_[m];
      T zi;
      if constexpr (SCALED) zi = small_row<T>(L, lb[m], le[m], off + row[m], ts, off) + (eps * ri) / dr[m];
      else if constexpr (SPAI) zi = small_row<T>(L, lb[m], le[m], off + row[m], ts, off) + eps * ri;
      else if constexpr (PRE == LSPCG_PRECOND_DIAGONAL) zi = ri / dr[m];
      else zi = ri;
      zr[m] = zi;
      if (own[m]) {
        dd_fma(dz[0], double(ri), double(zi));
        dd_fma(dz[1], double(ri), double(ri));
      }
    }
    double v2[2];
    small_dots<T, 2, TH>(dz, lds_z, v2);
    const double rr = k > 0 ? v2[1] : rr0;
    code = loop_test<T>(k, max_iter, rr, atol);
    if (tid == 0 && k > 0) keep_rr<T>(S, k, hist, rr);  // (one branch: k > 0 again inside folds away)
    if (code) break;
    rho_prev = rho;
    rho = v2[0];
    // x += α_{k-1} p_{k-1} ; p_k = p_{k-1}β + z
    const bool first = k == 0;
    const T beta = first ? T(0) : T(rho) / T(rho_prev);
#pragma unroll
    for (int m = 0; m < R; ++m) {
      if (!first) xr[m] = xr[m] + alpha * pr[m];
      pr[m] = first ? zr[m] : (pr[m] * beta) + zr[m];
      if (own[m]) ps[row[m]] = pr[m];
    }
    __syncthreads();
    // q = A p ; π = p·q ; α = ρ/π ; r -= α q
    DD dq[1] = {dd_zero()};
    T qr[R];
#pragma unroll
    for (int m = 0; m < R; ++m) {
      qr[m] = own[m] ? small_row<T>(A, ab[m], ae[m], off + row[m], ps, off) : T(0);
      if (own[m]) dd_fma(dq[0], double(pr[m]), double(qr[m]));
    }
    double v1[1];
    small_dots<T, 1, TH>(dq, lds_q, v1);
    pq = v1[0];
    alpha = T(rho) / T(pq);
    if (tid == 0) keep_coef(coef, k, rho, pq);
#pragma unroll
    for (int m = 0; m < R; ++m) {
      rr_[m] = rr_[m] - alpha * qr[m];
      if (own[m]) rs[row[m]] = rr_[m];
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < R; ++m) {
    if (!own[m]) continue;
    x[off + row[m]] = xr[m];
    p[off + row[m]] = pr[m];
  }
  if (tid == 0) {
    commit_step<T>(S, nullptr, rho_prev, rho, pq, alpha, k);
    S->done = code;
  }
}

// IC: ρ = r·z after the two triangular solves
template <typename T>
__global__ void __launch_bounds__(kThreads) k_dot_rho(int64_t n, PcgState* S, const T* __restrict__ r,
                                                      const T* __restrict__ z, double* partials, unsigned* ticket) {
  if (S->done) return;
  DD dots[1] = {dd_zero()};
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    dd_fma(dots[0], double(r[i]), double(z[i]));
  grid_reduce_dd<1>(dots, partials, ticket, [&](const double* v) {
    S->rho_prev = S->rho;
    S->rho = round_to<T>(v[0]);
  });
}

// after the loop: the deferred x += α_{k-1} p_{k-1} of the last completed iteration
template <typename T>
__global__ void __launch_bounds__(kThreads) k_x_fixup(int64_t n, const PcgState* S, const T* __restrict__ p,
                                                      T* __restrict__ x) {
  if (S->iter < 1 || S->bb == 0.0) return;
  const T alpha = T(S->alpha);
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    x[i] = x[i] + alpha * p[i];
}

}  // namespace lspcg
