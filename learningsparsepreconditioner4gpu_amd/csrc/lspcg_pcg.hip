// Device-resident preconditioned CG (replaces pymathprim.linalg.PreconditionedConjugateGradient,
// call sites neural_cg/utils/validate.py:54-160; arithmetic of scipy 1.15 iterative.py:359-418,
// the reference's CPU restatement validate.py:163-341).
//
// Schedules, all with scipy's exact floating-point expressions, so every schedule
// produces the same iterate and residual history bit for bit:
//   * split ext_spai schedule (SELL views): five launches per iteration
//       KA  t = Lᵀ r_k                                         [SpMV Lᵀ]
//       KB  z = L t + ε r_k ; group partials of ρ_k = r_k·z, ‖r_k‖²   [SpMV L]
//       UP  top-of-loop test on ‖r_k‖ ; x += α_{k-1} p_{k-1} ; p_k = p_{k-1}β + z
//       KC  q = A p_k ; group partials of π_k = p_k·q              [SpMV A]
//       UR  α_k = ρ_k/π_k ; r_{k+1} = r_k - α_k q
//   * the same five phases with last-arriver grid reductions (CSR / BSR views, CG, Jacobi, IC);
//   * one-workgroup solve (k_pcg_small) for n <= LSPCG_SMALL_N.
// Every multi-launch kernel is predicated on a device `done` flag, so the host replays
// graph-captured chunks of iterations and polls once per chunk without changing the iteration
// count or the iterate; the deferred x update of the last iteration is one fix-up launch.
//
// This unit: the single-system host code and the lspcg_solver_* ABI.  scipy's scalar recurrence
// (state, top-of-loop test, every transition) is in lspcg_pcg_step.hpp, the loop's device code in
// lspcg_pcg_kernels.hpp, the parity dots in lspcg_pcg_parity.hpp, the solver handle and the host
// control code shared with the batched solver (lspcg_batch.hip) in lspcg_solver.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "lspcg_factor.hpp"
#include "lspcg_pcg_kernels.hpp"
#include "lspcg_pcg_parity.hpp"
#include "lspcg_solver.hpp"

using namespace lspcg;

// device code of the single-system path alone (non-template kernels: defined in this unit only)
namespace lspcg {

// the split CG / Jacobi schedule's first UP reads ρ_0 from the groups: group 0 <- (ρ_0, ‖r_0‖²) of
// the init launch's state, the other groups <- 0 (exact in the dd sums)
__global__ void k_seed_groups(const PcgState* S, double* __restrict__ gz, int ng) {
  for (int i = threadIdx.x; i < 4 * ng; i += blockDim.x) {
    double v = 0.0;
    if (i == 0) v = S->rho;
    if (i == 2) v = S->rr;
    gz[i] = v;
  }
}

// ---- storage optimisation helpers (see DESIGN.md "PCG storage")
__global__ void k_f32_inexact(int64_t n, const double* __restrict__ v, int* __restrict__ flag) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const double a = v[i];
    if (!(double(float(a)) == a)) atomicOr(flag, 1);  // also true for NaN
  }
}
__global__ void k_to_f32(int64_t n, const double* __restrict__ v, float* __restrict__ out) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    out[i] = float(v[i]);
}
__global__ void k_i32_neq(int64_t n, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                          int* __restrict__ flag) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    if (a[i] != b[i]) atomicOr(flag, 2);
}

static int elem_grid(int64_t n) {  // 2 elements per lane, >= 2 pairs per lane, <= 1024 partials
  const int64_t g = (n + kThreads * 4 - 1) / (kThreads * 4);
  return int(std::max<int64_t>(1, std::min<int64_t>(g, 1024)));
}

}  // namespace lspcg

// (Re)build the SELL copy of iteration view w (0 = A, 1 = L, 2 = Lᵀ); L and Lᵀ reuse A's
// pattern when make_view found the same index arrays.
static int build_sell_bsr3(lspcg_solver* s, int w, const lspcg_mat* view);

static int build_sell(lspcg_solver* s, int w, const lspcg_mat* view) {
  hipStream_t st = s->ctx->stream;
  if (s->sv[w] || s->spat[w].gp) LSPCG_HIP(hipStreamSynchronize(s->stream));  // a solve may use them
  // L / Lᵀ on A's pattern again (a new L for the same system): refill the value array in place, so
  // its address -- and with it every captured iteration graph -- stays valid (graph_key)
  // (the pattern may have been rebuilt at the same host address -- set_dot_order's switch back to the
  // unpermuted A -- so the array's entry count must match the pattern's, not just the pointers)
  // The same holds for a pattern of L's / Lᵀ's own when the caller vouches for it (same_L_pattern: the
  // installed handle with new values only, lspcg_batch_update): refilled, not rebuilt.
  const bool on_A = s->sp[w] && s->sp[w] == s->sp[0] && view->rowptr == s->Av.rowptr && view->colind == s->Av.colind;
  const bool on_own = s->same_L_pattern && s->sp[w] == &s->spat[w] &&
                      !(s->sp[0] && view->rowptr == s->Av.rowptr && view->colind == s->Av.colind);
  if (w > 0 && s->use_sell && s->sv[w] && s->sp[w] && (on_A || on_own) && view->storage_dtype() == s->svd[w] &&
      s->svn[w] == s->sp[w]->slots()) {
    const SellPattern* P = s->sp[w];
    const int vd = view->storage_dtype();
    return P->bs == 3 ? bsell_fill_values(*P, view->vals, vd, vd, st, &s->sv[w])
                      : sell_fill_values(*P, view->colind, view->vals, vd, vd, st, &s->sv[w]);
  }
  (void)hipFree(s->sv[w]);
  s->sv[w] = nullptr;
  s->spat[w].release();
  s->sp[w] = nullptr;
  if (!s->use_sell || view->n == 0 || view->nnzb == 0) return LSPCG_OK;
  if (view->block_size == 3) return build_sell_bsr3(s, w, view);
  if (view->block_size != 1) return LSPCG_OK;
  const SellPattern* P = nullptr;
  if (w > 0 && s->sp[0] && view->rowptr == s->Av.rowptr && view->colind == s->Av.colind) {
    P = s->sp[0];
  } else {
    // SELL-DIA except for systems the one-workgroup solve takes (its per-thread rows load 4-entry
    // groups with one 16-B load; slot-by-slot loads measured 16.0 vs 9.8 us per iteration at n = 900)
    const bool dia = s->dia_ok && view->n > std::min<int64_t>(s->small_n, int64_t(kSmallThreadsBig) * 3);
    const int rc = sell_build_pattern(view->n, view->nnzb, view->rowptr, view->colind, sell_max_pad(),
                                      kSellCol16 | (dia ? kSellColDia | kSellColJag | kSellColXs : 0) |
                                          (dia && sellc_allowed(view->n) ? kSellColCode : 0),
                                      st, &s->spat[w]);
    if (rc == LSPCG_ERR_UNSUPPORTED) return LSPCG_OK;  // padding too large: CSR kernel
    if (rc) return rc;
    P = &s->spat[w];
  }
  const int vd = view->storage_dtype();
  if (int rc = sell_fill_values(*P, view->colind, view->vals, vd, vd, st, &s->sv[w])) return rc;
  s->svd[w] = vd;
  s->svn[w] = P->slots();
  s->sp[w] = P;
  return LSPCG_OK;
}

// BSR 3x3 views: the BSELL-64 block layout (lspcg_sell.hpp), pattern shared with A's when the
// index arrays are A's, values in the view's storage dtype (fp32 when lossless)
static int build_sell_bsr3(lspcg_solver* s, int w, const lspcg_mat* view) {
  hipStream_t st = s->ctx->stream;
  const bool shared = w > 0 && s->sp[0] && view->rowptr == s->Av.rowptr && view->colind == s->Av.colind;
  const SellPattern* P = nullptr;
  if (shared) {
    P = s->sp[0];
  } else {
    const int rc = bsell_build_pattern(view->nb, view->nnzb, view->rowptr, view->colind, sell_max_pad(), true,
                                       s->dia_ok && bsdia_allowed(), st, &s->spat[w]);
    if (rc == LSPCG_ERR_UNSUPPORTED) return LSPCG_OK;  // padding too large: the staged block kernel
    if (rc) return rc;
    P = &s->spat[w];
  }
  const int vd = view->storage_dtype();
  if (int rc = bsell_fill_values(*P, view->vals, vd, vd, st, &s->sv[w])) return rc;
  s->svd[w] = vd;
  s->svn[w] = P->slots();
  s->sp[w] = P;
  return LSPCG_OK;
}

// New values in A's iteration view, same pattern (lspcg_solver_update_matrix): the SELL / BSELL
// value array is refilled in place, or allocated anew when the view's storage type changed (values
// that became, or stopped being, fp32-exact).  The pattern is never rebuilt.
static int refill_sell_A(lspcg_solver* s) {
  const SellPattern* P = s->sp[0];
  if (!P) return LSPCG_OK;  // the staged CSR / BSR kernel reads the view itself
  const int vd = s->Av.storage_dtype();
  if (s->sv[0] && (vd != s->svd[0] || s->svn[0] != P->slots())) {
    (void)hipFree(s->sv[0]);
    s->sv[0] = nullptr;
  }
  hipStream_t st = s->ctx->stream;
  const int rc = P->bs == 3 ? bsell_fill_values(*P, s->Av.vals, vd, vd, st, &s->sv[0])
                            : sell_fill_values(*P, s->Av.colind, s->Av.vals, vd, vd, st, &s->sv[0]);
  if (rc) return rc;
  s->svd[0] = vd;
  s->svn[0] = P->slots();
  return LSPCG_OK;
}

static int flag_run(lspcg_solver* s, hipStream_t st, int* out) {
  int h = 0;
  LSPCG_HIP(hipMemcpyAsync(&h, s->flag, sizeof(int), hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  *out = h;
  return LSPCG_OK;
}

// view <- M; compact fp64 values to fp32 when exact; share `base`'s index arrays when equal.
// Both checks run before ONE host read of the flag (bit 0: some value not fp32-exact, bit 1:
// index arrays differ).  `known` (optional) supplies that flag instead -- Lᵀ from the
// symmetric-pattern transpose has L's pattern and a permutation of L's values.  Returns the
// flag in *flag_out (optional).
static int make_view(lspcg_solver* s, const lspcg_mat* M, lspcg_mat* view, const lspcg_mat* base, void** own,
                     const int* known = nullptr, int* flag_out = nullptr, int64_t* own_n = nullptr) {
  hipStream_t st = s->ctx->stream;
  const int64_t ne = M->nnzb * M->block_size * M->block_size;
  if (*own) {
    LSPCG_HIP(hipStreamSynchronize(s->stream));
    if (!own_n || *own_n != ne) {  // an fp32 copy of the same length is refilled in place below
      (void)hipFree(*own);
      *own = nullptr;
    }
  }
  *view = *M;
  const bool try_compact = M->dtype == LSPCG_F64 && M->storage_dtype() == LSPCG_F64 && ne > 0;
  const bool try_share = base && base != M && base->nb == M->nb && base->nnzb == M->nnzb &&
                         base->block_size == M->block_size;
  int f = 3;
  if (known) {
    f = *known;
  } else if (try_compact || try_share) {
    LSPCG_HIP(hipMemsetAsync(s->flag, 0, sizeof(int), st));
    if (try_compact)
      hipLaunchKernelGGL(k_f32_inexact, dim3(elem_grid(ne)), dim3(kThreads), 0, st, ne,
                         static_cast<const double*>(M->vals), s->flag);
    if (try_share) {
      hipLaunchKernelGGL(k_i32_neq, dim3(elem_grid(M->nb + 1)), dim3(kThreads), 0, st, M->nb + 1, M->rowptr,
                         base->rowptr, s->flag);
      if (M->nnzb)
        hipLaunchKernelGGL(k_i32_neq, dim3(elem_grid(M->nnzb)), dim3(kThreads), 0, st, M->nnzb, M->colind,
                           base->colind, s->flag);
    }
    if (int rc = flag_run(s, st, &f)) return rc;
    if (!try_compact) f |= 1;
    if (!try_share) f |= 2;
  }
  if (flag_out) *flag_out = f;
  if (*own && !(try_compact && !(f & 1))) {  // the new matrix is not stored compactly
    (void)hipFree(*own);
    *own = nullptr;
  }
  if (try_compact && !(f & 1)) {
    float* v = static_cast<float*>(*own);
    if (!v) {
      LSPCG_HIP(hipMalloc(&v, sizeof(float) * (ne + kEntryPad)));
      *own = v;
      if (own_n) *own_n = ne;
      LSPCG_HIP(hipMemsetAsync(v + ne, 0, sizeof(float) * kEntryPad, st));
    }
    hipLaunchKernelGGL(k_to_f32, dim3(elem_grid(ne)), dim3(kThreads), 0, st, ne, static_cast<const double*>(M->vals), v);
    view->vals = v;
    view->val_dtype = LSPCG_F32;
  }
  if (try_share && !(f & 2)) {
    view->rowptr = base->rowptr;
    view->colind = base->colind;
  }
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

// lspcg_solver_time_kernels: the next launch is stamped with its own start / end events
static void arm(lspcg_solver* s) {
  if (s->tk) kernel_timer() = &s->tk[s->tk_i++];
}

template <typename T, bool SC>
static int enqueue_iteration_split(lspcg_solver* s, hipStream_t st) {
  const int64_t n = s->n;
  PcgState* S = s->S;
  T *x = as<T>(s->x), *r = as<T>(s->r), *z = as<T>(s->z), *t = as<T>(s->t), *p = as<T>(s->p), *q = as<T>(s->q);
  const T* d = as<T>(s->d);
  double* gz = s->groups;
  double* gq = s->groups + 4096 * 2 * 2;
  const dim3 eg(elem_vec_grid<T>(n)), eb(kThreads);
  arm(s);
  int rc = launch_it<T>(s, 2, r, ProDone{S}, EpiT<T, SC>{t, d}, st);
  if (rc) return rc;
  arm(s);
  rc = launch_it<T>(s, 1, t, ProDone{S},
                    EpiZG<T, SC>{{z, r, d, T(s->eps)}, {s->partials, s->ticket, gz, s->gsz_l}}, st);
  if (rc) return rc;
  arm(s);
  LSPCG_LAUNCH_SPMV(k_update_p_g<T>, eg, eb, 0, st, n, S, static_cast<const double*>(gz), s->ng_l,
                    static_cast<const T*>(z), p, x);
  arm(s);
  rc = launch_it<T>(s, 0, p, ProDone{S}, EpiQG<T>{{q, p}, {s->partials, s->ticket, gq, s->gsz_a}}, st);
  if (rc) return rc;
  arm(s);
  LSPCG_LAUNCH_SPMV(k_update_r_g<T>, eg, eb, 0, st, n, S, static_cast<const double*>(gq), s->ng_a,
                    static_cast<const T*>(q), r);
  kernel_timer() = nullptr;
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

template <typename T>
static int enqueue_iteration(lspcg_solver* s, hipStream_t st) {
  if (s->split)
    return by_flag(s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED,
                   [&](auto sc) { return enqueue_iteration_split<T, decltype(sc)::value>(s, st); });
  const int64_t n = s->n;
  T *x = as<T>(s->x), *r = as<T>(s->r), *z = as<T>(s->z), *t = as<T>(s->t), *p = as<T>(s->p), *q = as<T>(s->q);
  const T* d = as<T>(s->d);
  PcgState* S = s->S;
  const ByLastArriver last{S, s->partials, s->ticket};
  const dim3 eg(elem_vec_grid<T>(n)), eb(kThreads);
  int rc = LSPCG_OK;
  if (s->split_cg) {  // UP (ρ_k, ‖r_k‖² from UR's groups) -> KC (π groups) -> UR (+ next dots' groups)
    double* gz = s->groups;
    double* gq = s->groups + 4096 * 2 * 2;
    const bool jac = s->precond == LSPCG_PRECOND_DIAGONAL;
    launch(k_update_p_g<T>, eg, eb, st, n, S, gz, s->ng_r, jac ? z : r, p, x);
    rc = launch_it<T>(s, 0, p, ProDone{S}, EpiQG<T>{{q, p}, {s->partials, s->ticket, gq, s->gsz_a}}, st);
    if (rc) return rc;
    if (jac)
      launch(k_update_r_gd<T, LSPCG_PRECOND_DIAGONAL>, eg, eb, st, n, S, gq, s->ng_a, q, r, d, z, s->partials,
             s->ticket, s->gsz_r, gz);
    else
      launch(k_update_r_gd<T, LSPCG_PRECOND_NONE>, eg, eb, st, n, S, gq, s->ng_a, q, r, d, z, s->partials, s->ticket,
             s->gsz_r, gz);
    LSPCG_HIP(hipGetLastError());
    return LSPCG_OK;
  }
  const bool spai = s->precond == LSPCG_PRECOND_EXT_SPAI || s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED;
  const T* zp = z;  // what UP adds to p: z = M⁻¹ r, r itself without a preconditioner
  switch (s->precond) {
    case LSPCG_PRECOND_EXT_SPAI:
    case LSPCG_PRECOND_EXT_SPAI_SCALED:
      rc = by_flag(s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED, [&](auto scf) {
        constexpr bool SC = decltype(scf)::value;
        if (int r2 = launch_it<T>(s, 2, r, ProDone{S}, EpiT<T, SC>{t, d}, st)) return r2;
        return launch_it<T>(s, 1, t, ProDone{S}, EpiZ<T, SC>{{z, r, d, T(s->eps)}, last}, st);
      });
      if (rc) return rc;
      enqueue_ob<kObZ>(s, st, 2, r, z, r, r);
      break;
    case LSPCG_PRECOND_NONE: zp = r; break;
    case LSPCG_PRECOND_DIAGONAL: break;
    case LSPCG_PRECOND_IC: {
      // z = L⁻ᵀ L⁻¹ r (t holds L⁻¹ r), ρ = r·z
      const int32_t* done = &S->done;
      if ((rc = enqueue_trsv(s->icL, s->planL, true, r, t, done, st))) return rc;
      if ((rc = enqueue_trsv(s->icU, s->planU, false, t, z, done, st))) return rc;
      launch(k_dot_rho<T>, eg, eb, st, n, S, r, z, s->partials, s->ticket);
      enqueue_ob<kObRho>(s, st, 1, r, z);
      break;
    }
    default:
      set_error("unknown preconditioner");
      return LSPCG_ERR_ARG;
  }
  // top-of-loop test on ‖r_k‖ (reduced by KB, the previous UR or the init) before the first update of
  // iteration k
  launch(k_update_p<T, ProCheck<T>>, eg, eb, st, n, ProCheck<T>{S}, S, zp, p, x);
  rc = spai ? launch_it<T>(s, 0, p, ProDone{S}, EpiQ<T, true>{{q, p}, last}, st)
            : launch_it<T>(s, 0, p, ProDone{S}, EpiQ<T>{{q, p}, last}, st);
  if (rc) return rc;
  if (spai) enqueue_ob<kObQ, false, true>(s, st, 1, p, q);  // (EpiQ<T, true> has counted the iteration)
  else enqueue_ob<kObQ>(s, st, 1, p, q);
  switch (s->precond) {
    case LSPCG_PRECOND_EXT_SPAI:
    case LSPCG_PRECOND_EXT_SPAI_SCALED: launch(k_update_r_nodot<T>, eg, eb, st, n, S, q, r); break;
    case LSPCG_PRECOND_NONE:
      launch(k_update_r<T, LSPCG_PRECOND_NONE>, eg, eb, st, n, S, q, r, d, z, s->partials, s->ticket);
      enqueue_ob<kObR>(s, st, 1, r, r);
      break;
    case LSPCG_PRECOND_DIAGONAL:
      launch(k_update_r<T, LSPCG_PRECOND_DIAGONAL>, eg, eb, st, n, S, q, r, d, z, s->partials, s->ticket);
      enqueue_ob<kObR, true>(s, st, 2, r, r, r, z);
      break;
    default:  // IC
      launch(k_update_r<T, LSPCG_PRECOND_EXT_SPAI>, eg, eb, st, n, S, q, r, d, z, s->partials, s->ticket);
      enqueue_ob<kObRR>(s, st, 1, r, r);
  }
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

template <typename T>
static int enqueue_init(lspcg_solver* s, hipStream_t st) {
  T *r = as<T>(s->r), *z = as<T>(s->z);
  const T *b = as<T>(s->b), *d = as<T>(s->d), *x = as<T>(s->x);
  const ByLastArriver last{s->S, s->partials, s->ticket};
  const int rc = s->precond == LSPCG_PRECOND_DIAGONAL
                     ? launch_it<T>(s, 0, x, ProNone{}, EpiResid<T, LSPCG_PRECOND_DIAGONAL>{{r, b, d, z}, last}, st)
                     : launch_it<T>(s, 0, x, ProNone{}, EpiResid<T, LSPCG_PRECOND_NONE>{{r, b, d, z}, last}, st);
  if (rc) return rc;
  if (s->split_cg) launch(k_seed_groups, dim3(1), dim3(256), st, s->S, s->groups, s->ng_r);
  if (s->precond == LSPCG_PRECOND_DIAGONAL) enqueue_ob<kObInit, true>(s, st, 3, r, r, b, b, r, z);
  else enqueue_ob<kObInit>(s, st, 2, r, r, b, b);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

template <typename T>
static int enqueue_fixup(lspcg_solver* s, hipStream_t st) {
  launch(k_x_fixup<T>, dim3(elem_grid(s->n)), dim3(kThreads), st, s->n, s->S, as<T>(s->p), as<T>(s->x));
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

static bool small_path(const lspcg_solver* s) {
  if (s->dot_order != LSPCG_DOT_COMPENSATED) return false;  // parity mode: the multi-kernel schedule
  if (s->n <= 0 || s->n > s->small_n || s->precond == LSPCG_PRECOND_IC || s->Av.block_size != 1) return false;
  if (s->n > int64_t(kSmallThreadsBig) * 3 || 3 * s->n * int64_t(esize(s->dtype)) > kSmallLds) return false;
  if (s->precond == LSPCG_PRECOND_EXT_SPAI || s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED)
    return s->Lv.block_size == 1 && s->LTv.block_size == 1;
  return true;
}

// diag(A) into s->d in the loop's numbering.  lspcg_mat_diagonal binary-searches sorted rows, so
// a permuted solver takes the caller's (sorted) A's diagonal and permutes it (s->z is scratch here:
// no solve is in flight while the preconditioner is installed).
static int solver_diagonal(lspcg_solver* s) {
  if (!s->ro.perm) return lspcg_mat_diagonal(s->A, s->d);  // issues on ctx stream
  if (int rc = lspcg_mat_diagonal(s->A_user, s->z)) return rc;
  const int bs = s->A->block_size;
  return vec_permute(s->dtype, s->n / bs, bs, s->ro.perm, s->z, s->d, false, s->ctx->stream);
}

// reducing grid of iteration view w's SpMV (the SELL / SELL-DIA copy, else the staged CSR kernel)
static int64_t view_reduce_grid(const lspcg_solver* s, int w) {
  if (s->sp[w]) return sell_grid(*s->sp[w], true);
  const lspcg_mat& V = w == 0 ? s->Av : (w == 1 ? s->Lv : s->LTv);
  const int64_t cap = std::min<int64_t>(kReduceGridMax, kElemBlocksMax);
  const int64_t g = V.block_size == 3 ? spmv_grid_t<256, 3>(V.nb) : spmv_grid_t<256, 1>(V.nb);
  return std::min<int64_t>(g, cap);
}

// group size / count of a reducing launch of `grid` workgroups (see lspcg_solver_set_spai)
static void split_groups(int mode, int64_t grid, int* gsz, int* ng) {
  const bool nogroups = mode == 2 || (mode < 0 && grid <= kNoGroupGrid);
  *gsz = nogroups ? 1 : int((grid + kMaxGroups - 1) / kMaxGroups);
  *ng = int((grid + *gsz - 1) / *gsz);
}

// CG / Jacobi on the split reductions: compensated dot order, fp64 / fp32 alike, the multi-kernel
// schedule (the one-workgroup solve has its own loop)
static void setup_split_cg(lspcg_solver* s) {
  s->split_cg = false;
  if (!(s->precond == LSPCG_PRECOND_NONE || s->precond == LSPCG_PRECOND_DIAGONAL)) return;
  if (!s->allow_split || s->dot_order != LSPCG_DOT_COMPENSATED || s->n == 0) return;
  split_groups(s->split_mode, view_reduce_grid(s, 0), &s->gsz_a, &s->ng_a);
  const int64_t eg = s->dtype == LSPCG_F64 ? elem_vec_grid<double>(s->n) : elem_vec_grid<float>(s->n);
  split_groups(s->split_mode, eg, &s->gsz_r, &s->ng_r);
  s->split_cg = s->gsz_a <= kMaxGroups && s->gsz_r <= kMaxGroups && s->ng_a <= 4096 && s->ng_r <= 4096;
}

// The A side of the solver: (optionally) the permuted system, its iteration view and SELL copy,
// the diagonal of the Jacobi preconditioner.
static int setup_A(lspcg_solver* s) {
  s->A = s->A_user;
  if (s->Ap) {
    lspcg_mat_destroy(s->Ap);
    s->Ap = nullptr;
  }
  s->ro.release();
  bool applied = false;
  if (s->reorder_ok && s->n > s->small_n) {
    if (int rc = rcm_reorder(s->A_user, s->reorder_mode, &s->ro, &applied)) return rc;
    if (applied) {
      if (int rc = mat_permute(s->A_user, s->ro, &s->Ap)) return rc;
      s->A = s->Ap;
    }
  }
  if (int rc = make_view(s, s->A, &s->Av, nullptr, &s->own_A, nullptr, nullptr, &s->own_A_n)) return rc;
  if (int rc = build_sell(s, 0, &s->Av)) return rc;
  setup_split_cg(s);
  if (s->precond == LSPCG_PRECOND_DIAGONAL) {
    if (int rc = solver_diagonal(s)) return rc;
    LSPCG_HIP(hipStreamSynchronize(s->ctx->stream));
  }
  return LSPCG_OK;
}

int lspcg::solver_create(lspcg_ctx* ctx, const lspcg_mat* A, int precond, bool dia_ok, bool reorder_ok,
                         lspcg_solver** out) {
  LSPCG_CHECK(ctx && A && out, LSPCG_ERR_ARG, "solver_create: NULL argument");
  LSPCG_CHECK(precond >= LSPCG_PRECOND_NONE && precond <= LSPCG_PRECOND_IC, LSPCG_ERR_ARG,
              "solver_create: unknown preconditioner " + std::to_string(precond));
  LSPCG_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<lspcg_solver> s(new lspcg_solver());
  s->ctx = ctx;
  s->A = A;
  s->A_user = A;
  s->dia_ok = dia_ok;
  s->reorder_ok = reorder_ok && precond != LSPCG_PRECOND_IC;
  s->precond = precond;
  s->dtype = A->dtype;
  s->n = A->n;
  const size_t vb = esize(s->dtype) * std::max<int64_t>(s->n, 1);
  LSPCG_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  // q (KC -> UR) and t (KA -> KB; the IC solve's intermediate) are never live together: one
  // buffer, 8 B per row less in the loop's working set (kuhn101: 78 vs 84 us per iteration with
  // two buffers, profiles/r3_tq_probe_v7.txt -- the loop sits at the Infinity Cache's size)
  for (void** v : {&s->x, &s->b, &s->r, &s->z, &s->t, &s->p, &s->q, &s->d}) {
    if (v == &s->q) {
      s->q = s->t;
      continue;
    }
    LSPCG_HIP(hipMalloc(v, vb));
    LSPCG_HIP(hipMemsetAsync(*v, 0, vb, s->stream));
  }
  LSPCG_HIP(hipMalloc(&s->S, sizeof(PcgState)));
  LSPCG_HIP(hipHostMalloc(&s->hS, 2 * sizeof(PcgState), hipHostMallocDefault));
  // partial slots: largest grid of any reducing launch (SpMV grid of A / L, element grid) x 2 dots
  // (n/255 bounds the grid of a CSR (256 rows/WG) and a BSR3 (85 block rows/WG) launch,
  // so L / Lᵀ in either layout fit too)
  const int64_t g = std::max<int64_t>((A->n + 254) / 255 + 1, 4096);
  LSPCG_HIP(hipMalloc(&s->partials, sizeof(double) * 2 * 2 * (g + 1)));
  LSPCG_HIP(hipMalloc(&s->ticket, sizeof(unsigned) * kTicketWords));
  LSPCG_HIP(hipMemsetAsync(s->ticket, 0, sizeof(unsigned) * kTicketWords, s->stream));
  LSPCG_HIP(hipMalloc(&s->groups, sizeof(double) * 4096 * 2 * 3));
  LSPCG_HIP(hipMemsetAsync(s->groups, 0, sizeof(double) * 4096 * 2 * 3, s->stream));
  LSPCG_HIP(hipMemsetAsync(s->S, 0, sizeof(PcgState), s->stream));
  for (hipEvent_t* e : {&s->ev_in, &s->ev_out, &s->ev_poll, &s->ev_poll2}) LSPCG_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  LSPCG_HIP(hipEventCreate(&s->ev_t0));
  LSPCG_HIP(hipEventCreate(&s->ev_t1));
  LSPCG_HIP(hipMalloc(&s->flag, sizeof(int)));
  LSPCG_HIP(hipMalloc(&s->ob_part, sizeof(double) * 3 * kObMaxThreads));
  if (const char* e = std::getenv("LSPCG_NO_SELL")) s->use_sell = e[0] == '0';
  if (const char* e = std::getenv("LSPCG_SMALL_N")) s->small_n = std::max<int64_t>(0, std::atoll(e));
  if (const char* e = std::getenv("LSPCG_SMALL_SELL")) s->small_sell = e[0] != '0';
  if (const char* e = std::getenv("LSPCG_SPLIT_REDUCE")) {
    s->allow_split = e[0] != '0';
    s->split_mode = std::atoi(e);
  }
  if (const char* e = std::getenv("LSPCG_REORDER")) s->reorder_mode = e[0] == 'a' ? -1 : std::atoi(e) ? 1 : 0;
  if (int rc = setup_A(s.get())) return rc;
  LSPCG_HIP(hipStreamSynchronize(s->stream));
  *out = s.release();
  return LSPCG_OK;
}

namespace lspcg {

GraphKey graph_key(const lspcg_solver* s) {
  GraphKey k;
  auto put = [&](auto x) {
    if constexpr (std::is_pointer<decltype(x)>::value) k.v.push_back(int64_t(reinterpret_cast<intptr_t>(x)));
    else k.v.push_back(int64_t(x));
  };
  for (int w = 0; w < 3; ++w) {
    const lspcg_mat& V = w == 0 ? s->Av : (w == 1 ? s->Lv : s->LTv);
    put(s->sp[w]);
    if (const SellPattern* P = s->sp[w]) P->each_field(put);  // a rebuilt pattern may reuse the host address
    put(s->sv[w]);
    put(V.rowptr);
    put(V.colind);
    put(V.vals);
    put(s->svd[w]);
    put(V.val_dtype);
  }
  put(s->split);
  put(s->split_cg);
  put(s->gsz_l);
  put(s->ng_l);
  put(s->gsz_a);
  put(s->ng_a);
  put(s->dot_order);
  for (const lspcg_mat* T : {s->icL, s->icU}) {  // the triangular solves' operands (IC)
    put(T ? T->rowptr : nullptr);
    put(T ? T->colind : nullptr);
  }
  for (const TrsvPlan* pl : {&s->planL, &s->planU}) {
    put(pl->pad);
    put(pl->npad);
    put(pl->head);
    put(pl->sv);
    put(pl->inv);
    put(pl->c);
  }
  k.eps = s->eps;
  return k;
}

}  // namespace lspcg

extern "C" {

int lspcg_solver_create(lspcg_ctx* ctx, const lspcg_mat* A, int precond, lspcg_solver** out) {
  return solver_create(ctx, A, precond, true, true, out);
}

int lspcg_solver_set_spai(lspcg_solver* s, const lspcg_mat* L, double epsilon, double* t_prec_ms) {
  LSPCG_CHECK(s && L, LSPCG_ERR_ARG, "set_spai: NULL");
  LSPCG_CHECK(s->precond == LSPCG_PRECOND_EXT_SPAI || s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED, LSPCG_ERR_ARG,
              "set_spai: solver was not created with an ext_spai preconditioner");
  LSPCG_CHECK(L->n == s->n, LSPCG_ERR_ARG, "set_spai: L has a different size than A");
  LSPCG_CHECK(L->dtype == s->dtype, LSPCG_ERR_ARG, "set_spai: L dtype differs from A dtype");
  hipStream_t cst = s->ctx->stream;
  const GraphKey key_before = graph_key(s);
  LSPCG_HIP(hipStreamSynchronize(s->stream));  // Lᵀ below may be referenced by a running solve
  LSPCG_HIP(hipEventRecord(s->ev_t0, cst));
  // Lᵀ (and, reordered, P L Pᵀ / P Lᵀ Pᵀ) of the previous factor are overwritten in place when the
  // new L has its shape: no free / allocate per sample, and the iteration views keep their addresses
  // (so the captured graphs survive, graph_key below)
  auto renew = [](lspcg_mat** slot, lspcg_mat* keep, int rc) {
    if (keep && keep != *slot) lspcg_mat_destroy(keep);
    return rc;
  };
  bool lt_same = false;
  lspcg_mat** raw_slot = s->ro.perm ? &s->LTo : &s->LT;  // Lᵀ in the ORIGINAL numbering: rows in scipy's order
  lspcg_mat* keep = *raw_slot;
  *raw_slot = nullptr;
  int rc = renew(raw_slot, keep, mat_transpose(L, raw_slot, &lt_same, keep));
  if (rc) return rc;
  const lspcg_mat* Lu = L;
  if (s->ro.perm) {  // reordered solver: P L Pᵀ and P Lᵀ Pᵀ, every row's entries in their original order
    LSPCG_CHECK(L->block_size == s->A->block_size, LSPCG_ERR_ARG, "set_spai: L and A block sizes differ");
    keep = s->Lp;
    s->Lp = nullptr;
    if ((rc = renew(&s->Lp, keep, mat_permute(L, s->ro, &s->Lp, keep)))) return rc;
    keep = s->LT;
    s->LT = nullptr;
    if ((rc = renew(&s->LT, keep, mat_permute(s->LTo, s->ro, &s->LT, keep)))) return rc;
    Lu = s->Lp;
  }
  if (s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED) {
    LSPCG_HIP(hipStreamSynchronize(s->stream));  // s->z is the permuted path's scratch
    rc = solver_diagonal(s);
    if (rc) return rc;
  }
  int lflag = 3;
  if ((rc = make_view(s, Lu, &s->Lv, &s->Av, &s->own_L, nullptr, &lflag, &s->own_L_n))) return rc;
  if ((rc = make_view(s, s->LT, &s->LTv, &s->Av, &s->own_LT, lt_same ? &lflag : nullptr, nullptr, &s->own_LT_n)))
    return rc;
  if ((rc = build_sell(s, 1, &s->Lv))) return rc;
  if ((rc = build_sell(s, 2, &s->LTv))) return rc;
  // the split schedule runs on any iteration views (SELL copies or the staged CSR kernel, whose
  // epilogues finish their dots the same way; round 5 -- before, it needed SELL views of A, L, Lᵀ)
  s->split_ok = s->allow_split;
  s->split = s->split_ok && s->dot_order == LSPCG_DOT_COMPENSATED;
  if (s->split_ok) {
    // <= 64 groups per reducing launch; no groups at all (the consumers sum every workgroup's
    // partial) for grids of <= kNoGroupGrid workgroups -- mid-size systems, where the group ticket's
    // round trip costs more than the consumers' extra loads (Poisson 256^2: 20.6 vs 22.0 us per
    // iteration; at 1 M rows, 1536 workgroups, the groups win: 91.4 vs 94.3).
    // LSPCG_SPLIT_REDUCE=1 / 2 force groups / no groups.
    split_groups(s->split_mode, view_reduce_grid(s, 1), &s->gsz_l, &s->ng_l);
    split_groups(s->split_mode, view_reduce_grid(s, 0), &s->gsz_a, &s->ng_a);
    LSPCG_CHECK(s->gsz_l <= kMaxGroups && s->gsz_a <= kMaxGroups, LSPCG_ERR_UNSUPPORTED,
                "set_spai: reducing grid too large for one-wave group sums");
  }
  LSPCG_HIP(hipEventRecord(s->ev_t1, cst));
  LSPCG_HIP(hipEventSynchronize(s->ev_t1));
  float ms = 0.f;
  LSPCG_HIP(hipEventElapsedTime(&ms, s->ev_t0, s->ev_t1));
  if (t_prec_ms) *t_prec_ms = ms;
  s->L = L;
  s->eps = epsilon;
  // graphs capture the views' addresses and ε: drop them unless the new L kept every one of them
  if (!(graph_key(s) == key_before)) {
    s->graphs.clear();
    multi_clear_graphs(s);
  }
  return LSPCG_OK;
}

// IC preconditioner: factor (given, or IC(0) of A computed on the device), its explicit transpose
// and both level orders
static int install_ic(lspcg_solver* s, const lspcg_mat* given, double* t_prec_ms) {
  LSPCG_CHECK(s, LSPCG_ERR_ARG, "set_ic: NULL");
  LSPCG_CHECK(s->precond == LSPCG_PRECOND_IC, LSPCG_ERR_ARG, "set_ic: solver was not created with LSPCG_PRECOND_IC");
  LSPCG_HIP(hipSetDevice(s->ctx->device));
  LSPCG_HIP(hipStreamSynchronize(s->stream));
  if (given) {
    LSPCG_CHECK(given->n == s->n && given->block_size == 1 && given->dtype == s->dtype &&
                    given->storage_dtype() == given->dtype,
                LSPCG_ERR_ARG, "set_ic_factor: L must be a scalar CSR of the solver's size and dtype");
    // lower triangular with the diagonal stored last in every row, and a nonzero diagonal (host
    // check; scipy's spsolve_triangular, the reference's apply, raises LinAlgError "A is singular:
    // zero entry on diagonal" there -- validate.py:344-419)
    std::vector<int32_t> rp(size_t(s->n) + 1), ci(size_t(std::max<int64_t>(given->nnzb, 1)));
    std::vector<double> vd(given->dtype == LSPCG_F64 ? ci.size() : 0);
    std::vector<float> vf(given->dtype == LSPCG_F32 ? ci.size() : 0);
    void* vals = given->dtype == LSPCG_F64 ? static_cast<void*>(vd.data()) : static_cast<void*>(vf.data());
    if (int rc = lspcg_mat_copy_out(given, rp.data(), ci.data(), vals)) return rc;
    for (int64_t i = 0; i < s->n; ++i) {
      bool ok = rp[i + 1] > rp[i] && ci[rp[i + 1] - 1] == i;
      for (int32_t p = rp[i]; ok && p < rp[i + 1] - 1; ++p) ok = ci[p] < ci[p + 1];
      LSPCG_CHECK(ok, LSPCG_ERR_FORMAT,
                  "set_ic_factor: row " + std::to_string(i) + " is not lower triangular with its diagonal last");
      const int32_t dp = rp[i + 1] - 1;
      const double dv = given->dtype == LSPCG_F64 ? vd[dp] : double(vf[dp]);
      LSPCG_CHECK(dv != 0.0, LSPCG_ERR_SINGULAR,
                  "set_ic_factor: A is singular: zero entry on diagonal (row " + std::to_string(i) + ")");
    }
  }
  hipStream_t cst = s->ctx->stream;
  LSPCG_HIP(hipEventRecord(s->ev_t0, cst));
  for (lspcg_mat** m : {&s->icL, &s->icU}) {
    if (*m) lspcg_mat_destroy(*m);
    *m = nullptr;
  }
  s->planL.release();
  s->planU.release();
  int rc = given ? lspcg_mat_create_csr(s->ctx, given->n, given->nnzb, given->rowptr, given->colind, given->vals,
                                        given->dtype, &s->icL)
                 : ic0_factor(s->A, &s->icL, &s->ic_lev);
  s->ic_own = !given;
  s->ic_broken = false;
  if (!rc) rc = lspcg_mat_transpose(s->icL, &s->icU);
  if (!rc) rc = trsv_plan_build(s->icL, true, &s->planL);
  if (!rc) rc = trsv_plan_build(s->icU, false, &s->planU);
  if (rc) return rc;
  LSPCG_HIP(hipEventRecord(s->ev_t1, cst));
  LSPCG_HIP(hipEventSynchronize(s->ev_t1));
  float ms = 0.f;
  LSPCG_HIP(hipEventElapsedTime(&ms, s->ev_t0, s->ev_t1));
  if (t_prec_ms) *t_prec_ms = ms;
  s->graphs.clear();
  multi_clear_graphs(s);
  return LSPCG_OK;
}

int lspcg_solver_set_ic(lspcg_solver* s, double* t_prec_ms) { return install_ic(s, nullptr, t_prec_ms); }

// lspcg_solver_update_matrix's steps; any error return leaves views that may have moved
static int update_matrix_steps(lspcg_solver* s) {
  int rc = LSPCG_OK;
  if (s->ro.perm) {  // P A Pᵀ with the kept permutation, over the previous one
    lspcg_mat* out = nullptr;
    if ((rc = mat_permute(s->A_user, s->ro, &out, s->Ap))) return rc;
    if (out != s->Ap) {  // (the SELL pattern and the L views read Ap's index arrays)
      lspcg_mat_destroy(out);
      set_error("update_matrix: the solver's matrix no longer has the shape it was created with");
      return LSPCG_ERR_FORMAT;
    }
  }
  // the fp32 copy refilled in place, or the switch to / from it when the values' fp32-exactness changed
  if ((rc = make_view(s, s->A, &s->Av, nullptr, &s->own_A, nullptr, nullptr, &s->own_A_n))) return rc;
  if ((rc = refill_sell_A(s))) return rc;
  if (s->precond == LSPCG_PRECOND_DIAGONAL || s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED) {
    if ((rc = solver_diagonal(s))) return rc;
  }
  if (s->precond == LSPCG_PRECOND_IC && s->icL && s->ic_own) {
    // numeric-only IC(0) into icL, its transpose into icU, the plans' scaled values; the levels, the
    // padded orders and the counter words belong to the pattern
    s->ic_broken = true;
    if ((rc = ic0_numeric(s->A, s->icL, s->ic_lev))) return rc;
    lspcg_mat* keep = s->icU;
    s->icU = nullptr;
    rc = mat_transpose(s->icL, &s->icU, nullptr, keep);
    if (keep && keep != s->icU) lspcg_mat_destroy(keep);
    if (rc) return rc;
    if ((rc = trsv_plan_refill(s->icL, true, s->planL))) return rc;
    if ((rc = trsv_plan_refill(s->icU, false, s->planU))) return rc;
    s->ic_broken = false;
  }
  return LSPCG_OK;
}

int lspcg_solver_update_matrix(lspcg_solver* s, double* t_ms, int* graphs_kept) {
  LSPCG_CHECK(s, LSPCG_ERR_ARG, "update_matrix: NULL");
  LSPCG_HIP(hipSetDevice(s->ctx->device));
  if (graphs_kept) *graphs_kept = 0;
  hipStream_t cst = s->ctx->stream;
  const GraphKey key_before = graph_key(s);
  LSPCG_HIP(hipStreamSynchronize(s->stream));  // a running solve reads everything rewritten below
  // From here the views may move (the fp32 copy, a SELL value array of another storage type): a
  // failed update -- an IC(0) breakdown, an allocation -- drops the graphs, which hold the old
  // addresses by value, and the update that follows it reports none kept.
  const bool after_failure = s->update_failed;
  s->update_failed = true;
  auto fail = [&](int rc) {
    s->graphs.clear();
    multi_clear_graphs(s);
    return rc;
  };
  if (hipEventRecord(s->ev_t0, cst) != hipSuccess) return fail(LSPCG_ERR_HIP);
  if (int rc = update_matrix_steps(s)) return fail(rc);
  float ms = 0.f;
  if (hipEventRecord(s->ev_t1, cst) != hipSuccess || hipEventSynchronize(s->ev_t1) != hipSuccess ||
      hipEventElapsedTime(&ms, s->ev_t0, s->ev_t1) != hipSuccess) {
    set_error("update_matrix: timing the update on the context's stream failed");
    return fail(LSPCG_ERR_HIP);
  }
  if (t_ms) *t_ms = ms;
  s->update_failed = false;
  // graphs hold the views' addresses and kinds by value: they survive exactly when none moved
  const bool kept = !after_failure && graph_key(s) == key_before;
  if (!kept) {
    s->graphs.clear();
    multi_clear_graphs(s);
  }
  if (graphs_kept) *graphs_kept = kept ? 1 : 0;
  return LSPCG_OK;
}

int lspcg_solver_set_ic_factor(lspcg_solver* s, const lspcg_mat* L, double* t_prec_ms) {
  LSPCG_CHECK(L, LSPCG_ERR_ARG, "set_ic_factor: NULL factor");
  return install_ic(s, L, t_prec_ms);
}

int lspcg_solver_solve(lspcg_solver* s, const void* b, void* x, double rtol, int64_t max_iter, int64_t* iters,
                       double* res_hist, double* t_solve_ms) {
  return lspcg_solver_solve_coef(s, b, x, rtol, max_iter, iters, res_hist, t_solve_ms, nullptr);
}

int lspcg_solver_solve_coef(lspcg_solver* s, const void* b, void* x, double rtol, int64_t max_iter, int64_t* iters,
                            double* res_hist, double* t_solve_ms, double* coef) {
  LSPCG_CHECK(s && b && x && iters, LSPCG_ERR_ARG, "solve: NULL argument");
  LSPCG_CHECK(!(s->precond == LSPCG_PRECOND_EXT_SPAI || s->precond == LSPCG_PRECOND_EXT_SPAI_SCALED) || s->LT,
              LSPCG_ERR_ARG, "solve: ext_spai not set");
  LSPCG_CHECK(s->precond != LSPCG_PRECOND_IC || s->icL, LSPCG_ERR_ARG, "solve: IC factor not set (lspcg_solver_set_ic)");
  LSPCG_CHECK(!s->ic_broken, LSPCG_ERR_BREAKDOWN,
              "solve: the last lspcg_solver_update_matrix broke down in IC(0); update the matrix again first");
  LSPCG_HIP(hipSetDevice(s->ctx->device));
  const int64_t n = s->n;
  if (max_iter <= 0) max_iter = n;
  hipStream_t st = s->stream;
  const size_t vb = esize(s->dtype) * n;
  double* dhist = nullptr;  // the solver's persistent history buffer, grown on demand
  if (res_hist) {
    if (s->dhist_cap < max_iter + 2) {
      LSPCG_HIP(hipStreamSynchronize(st));
      (void)hipFree(s->dhist);
      (void)hipHostFree(s->hhist);
      s->dhist = nullptr;
      s->hhist = nullptr;
      s->dhist_cap = 0;
      LSPCG_HIP(hipMalloc(&s->dhist, sizeof(double) * (max_iter + 2)));
      LSPCG_HIP(hipHostMalloc(&s->hhist, sizeof(double) * (max_iter + 2), hipHostMallocDefault));
      s->dhist_cap = max_iter + 2;
    }
    dhist = s->dhist;
  }
  double* dcoef = nullptr;  // the recorded (ρ_k, π_k) pairs: the same handling
  if (coef) {
    if (s->dcoef_cap < 2 * (max_iter + 1)) {
      LSPCG_HIP(hipStreamSynchronize(st));
      (void)hipFree(s->dcoef);
      (void)hipHostFree(s->hcoef);
      s->dcoef = nullptr;
      s->hcoef = nullptr;
      s->dcoef_cap = 0;
      LSPCG_HIP(hipMalloc(&s->dcoef, sizeof(double) * 2 * (max_iter + 1)));
      LSPCG_HIP(hipHostMalloc(&s->hcoef, sizeof(double) * 2 * (max_iter + 1), hipHostMallocDefault));
      s->dcoef_cap = 2 * (max_iter + 1);
    }
    dcoef = s->dcoef;
  }

  // every enqueue below runs under the process-wide submission lock, released around each host
  // wait (lspcg_internal.hpp: concurrent solves from several host threads)
  std::unique_lock<std::mutex> sub(submit_mutex());
  LSPCG_HIP(hipEventRecord(s->ev_in, s->ctx->stream));
  LSPCG_HIP(hipStreamWaitEvent(st, s->ev_in, 0));
  LSPCG_HIP(hipEventRecord(s->ev_t0, st));
  if (n && s->ro.perm) {  // into the permuted numbering
    const int bs = s->A->block_size;
    if (int r2 = vec_permute(s->dtype, n / bs, bs, s->ro.perm, b, s->b, false, st)) return r2;
    if (int r2 = vec_permute(s->dtype, n / bs, bs, s->ro.perm, x, s->x, false, st)) return r2;
  } else if (n) {
    LSPCG_HIP(hipMemcpyAsync(s->b, b, vb, hipMemcpyDeviceToDevice, st));
    LSPCG_HIP(hipMemcpyAsync(s->x, x, vb, hipMemcpyDeviceToDevice, st));
  }
  *s->hS = initial_state(rtol, s->eps, dhist, max_iter, dcoef);
  LSPCG_HIP(hipMemcpyAsync(s->S, s->hS, sizeof(PcgState), hipMemcpyHostToDevice, st));
  int rc = by_dtype(s->dtype, [&](auto t) { return enqueue_init<decltype(t)>(s, st); });
  if (rc) return rc;

  // graphs hold <= ~4096 nodes (IC: one launch per level of each triangular solve)
  const int kpi = s->precond == LSPCG_PRECOND_IC ? 2 * kTrsvLaunches + 4 : 5;
  const int max_chunk = std::max(1, std::min(32, 4096 / kpi));
  StatePoll poll{1, s->S, s->hS, {s->ev_poll, s->ev_poll2}, st, sub};
  PcgState fin{};  // the state the loop ended in (later, early-exit launches leave it unchanged)
  if (small_path(s)) {  // one launch runs the whole loop (k_pcg_small)
    rc = by_dtype(s->dtype, [&](auto t) {
      return launch_pcg_small<decltype(t)>(s->precond, 1, s, n, s->S, nullptr, nullptr, st);
    });
    if (!rc) rc = poll.post();
    if (!rc) rc = poll.take(&fin);
  } else {
    auto one = [&] { return by_dtype(s->dtype, [&](auto t) { return enqueue_iteration<decltype(t)>(s, st); }); };
    rc = poll.run(&max_iter, max_chunk, [&](int c) { return s->graphs.launch(st, c, one); }, &fin);
  }
  if (rc) return rc;
  rc = by_dtype(s->dtype, [&](auto t) { return enqueue_fixup<decltype(t)>(s, st); });
  if (rc) return rc;
  const void* src = (fin.bb == 0.0) ? s->b : s->x;  // scipy returns b when ‖b‖ = 0
  if (n && s->ro.perm) {  // back to the caller's numbering
    if (int r2 = vec_permute(s->dtype, n / s->A->block_size, s->A->block_size, s->ro.perm, src, x, true, st)) return r2;
  } else if (n) {
    LSPCG_HIP(hipMemcpyAsync(x, src, vb, hipMemcpyDeviceToDevice, st));
  }
  LSPCG_HIP(hipEventRecord(s->ev_t1, st));
  // the tail's device-to-host copies (IC timeout flags, the residual history) are enqueued behind the
  // solve into pinned mirrors, so the last host wait is the only one and the submission lock is not
  // held through it (a blocking copy under the lock serialised concurrent solves' tails)
  const bool ic = s->precond == LSPCG_PRECOND_IC;
  if (ic) {
    if (!s->hflags) LSPCG_HIP(hipHostMalloc(&s->hflags, 2 * sizeof(unsigned), hipHostMallocDefault));
    s->hflags[0] = s->hflags[1] = 0;
    if (s->planL.head)
      LSPCG_HIP(hipMemcpyAsync(&s->hflags[0], s->planL.head + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (s->planU.head)
      LSPCG_HIP(hipMemcpyAsync(&s->hflags[1], s->planU.head + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  }
  const SolveTail tail(fin, max_iter);
  if (res_hist) LSPCG_HIP(hipMemcpyAsync(s->hhist, dhist, sizeof(double) * tail.written, hipMemcpyDeviceToHost, st));
  if (coef && tail.pairs() > 0)
    LSPCG_HIP(hipMemcpyAsync(s->hcoef, dcoef, sizeof(double) * 2 * tail.pairs(), hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipEventRecord(s->ev_out, st));
  LSPCG_HIP(hipStreamWaitEvent(s->ctx->stream, s->ev_out, 0));
  sub.unlock();
  LSPCG_HIP(hipEventSynchronize(s->ev_out));
  if (ic && (s->hflags[0] || s->hflags[1])) {  // a timed-out sync-free hand-off fails the solve loudly
    sub.lock();
    if (int r2 = trsv_check_timeout(s->planL, st)) return r2;  // resets the flag, sets the message
    if (int r2 = trsv_check_timeout(s->planU, st)) return r2;
  }
  float ms = 0.f;
  LSPCG_HIP(hipEventElapsedTime(&ms, s->ev_t0, s->ev_t1));
  if (t_solve_ms) *t_solve_ms = ms;
  static const bool prof = [] {
    const char* e = std::getenv("LSPCG_SOLVE_PROFILE");
    return e && e[0] == '1';
  }();
  if (prof)
    std::fprintf(stderr, "[lspcg solve] n=%lld iters=%lld launched=%lld in %lld graphs, %.3f ms\n",
                 static_cast<long long>(n), static_cast<long long>(tail.iters), static_cast<long long>(poll.launched),
                 static_cast<long long>(poll.nlaunch), double(ms));
  *iters = tail.iters;
  if (res_hist) {
    std::memcpy(res_hist, s->hhist, sizeof(double) * tail.written);
    tail.nan_fill(res_hist);
  }
  if (coef) {
    std::memcpy(coef, s->hcoef, sizeof(double) * 2 * tail.pairs());
    tail.nan_fill_coef(coef);
  }
  return (fin.done == 1) ? LSPCG_OK : LSPCG_NOT_CONVERGED;
}

int lspcg_solver_set_dot_order(lspcg_solver* s, int order, int threads) {
  LSPCG_CHECK(s, LSPCG_ERR_ARG, "set_dot_order: NULL");
  LSPCG_CHECK(order == LSPCG_DOT_COMPENSATED || order == LSPCG_DOT_OPENBLAS, LSPCG_ERR_ARG,
              "set_dot_order: unknown order " + std::to_string(order));
  LSPCG_CHECK(order == LSPCG_DOT_COMPENSATED || (threads >= 1 && threads <= kObMaxThreads), LSPCG_ERR_ARG,
              "set_dot_order: threads must be in [1, 16]");
  LSPCG_CHECK(order == LSPCG_DOT_COMPENSATED || s->dtype == LSPCG_F64, LSPCG_ERR_UNSUPPORTED,
              "set_dot_order: the OpenBLAS order is the fp64 ddot's (the reference solves in fp64)");
  LSPCG_HIP(hipStreamSynchronize(s->stream));
  s->dot_order = order;
  s->dot_threads = order == LSPCG_DOT_OPENBLAS ? threads : 1;
  if (order == LSPCG_DOT_OPENBLAS && s->reorder_ok) {
    // numpy's ddot order runs over the ORIGINAL numbering: back to the unpermuted system for good
    s->reorder_ok = false;
    if (s->ro.perm) {
      if (int rc = setup_A(s)) return rc;
      if (s->L) {
        if (int rc = lspcg_solver_set_spai(s, s->L, s->eps, nullptr)) return rc;
      }
    }
  }
  s->split = s->split_ok && order == LSPCG_DOT_COMPENSATED;
  setup_split_cg(s);
  s->graphs.clear();
  multi_clear_graphs(s);
  return LSPCG_OK;
}

int lspcg_solver_time_kernels(lspcg_solver* s, const void* b, int64_t iters, double* kernel_ms, int* nk) {
  LSPCG_CHECK(s && b && kernel_ms && nk && iters > 0, LSPCG_ERR_ARG, "time_kernels: bad argument");
  *nk = 0;
  LSPCG_CHECK(s->split, LSPCG_ERR_UNSUPPORTED, "time_kernels: only the split ext_spai schedule (LSPCG_SPLIT_REDUCE != 0)");
  LSPCG_HIP(hipSetDevice(s->ctx->device));
  const int64_t n = s->n;
  hipStream_t st = s->stream;
  const size_t vb = esize(s->dtype) * n;
  LSPCG_HIP(hipEventRecord(s->ev_in, s->ctx->stream));
  LSPCG_HIP(hipStreamWaitEvent(st, s->ev_in, 0));
  if (s->ro.perm) {
    if (int r2 = vec_permute(s->dtype, n / s->A->block_size, s->A->block_size, s->ro.perm, b, s->b, false, st)) return r2;
  } else {
    LSPCG_HIP(hipMemcpyAsync(s->b, b, vb, hipMemcpyDeviceToDevice, st));
  }
  LSPCG_HIP(hipMemsetAsync(s->x, 0, vb, st));
  *s->hS = initial_state(0.0, s->eps, nullptr, iters + 1);  // atol 0: no convergence stop, `iters` full iterations
  LSPCG_HIP(hipMemcpyAsync(s->S, s->hS, sizeof(PcgState), hipMemcpyHostToDevice, st));
  int rc = by_dtype(s->dtype, [&](auto t) { return enqueue_init<decltype(t)>(s, st); });
  if (rc) return rc;
  // each launch timed by its own start / end stamps (KernelTimer: the kernel durations rocprofv3's
  // trace reports, without the in-stream boundaries event pairs between launches would add)
  constexpr int K = 5;
  KernelTimer kt[K];
  for (auto& t : kt) {
    LSPCG_HIP(hipEventCreate(&t.start));
    LSPCG_HIP(hipEventCreate(&t.stop));
  }
  double acc[K] = {0, 0, 0, 0, 0};
  for (int64_t it = 0; it < iters && rc == LSPCG_OK; ++it) {
    s->tk = kt;
    s->tk_i = 0;
    rc = by_dtype(s->dtype, [&](auto t) { return enqueue_iteration<decltype(t)>(s, st); });
    s->tk = nullptr;
    kernel_timer() = nullptr;
    if (rc) break;
    LSPCG_HIP(hipEventSynchronize(kt[K - 1].stop));
    for (int k = 0; k < K; ++k) {
      float ms = 0.f;
      LSPCG_HIP(hipEventElapsedTime(&ms, kt[k].start, kt[k].stop));
      acc[k] += ms;
    }
  }
  for (auto& t : kt) {
    (void)hipEventDestroy(t.start);
    (void)hipEventDestroy(t.stop);
  }
  if (rc) return rc;
  for (int k = 0; k < K; ++k) kernel_ms[k] = acc[k] / double(iters);
  *nk = K;
  LSPCG_HIP(hipEventRecord(s->ev_out, st));
  LSPCG_HIP(hipStreamWaitEvent(s->ctx->stream, s->ev_out, 0));
  return LSPCG_OK;
}

int lspcg_solver_views(const lspcg_solver* s, int* col_kind, int* value_bytes) {
  LSPCG_CHECK(s && col_kind && value_bytes, LSPCG_ERR_ARG, "solver_views: NULL argument");
  for (int w = 0; w < 3; ++w) {
    const SellPattern* P = s->sp[w];
    col_kind[w] = P ? P->col_bits : 0;
    value_bytes[w] = !P ? 0 : s->svd[w] == LSPCG_F32 ? 4 : 8;
  }
  return LSPCG_OK;
}

int lspcg_solver_reorder_info(const lspcg_solver* s, int* applied, double* mean_offset_before,
                              double* mean_offset_after) {
  LSPCG_CHECK(s && applied, LSPCG_ERR_ARG, "reorder_info: NULL argument");
  *applied = s->ro.perm ? 1 : 0;
  if (mean_offset_before) *mean_offset_before = s->ro.off_before;
  if (mean_offset_after) *mean_offset_after = s->ro.off_after;
  return LSPCG_OK;
}

int lspcg_solver_destroy(lspcg_solver* s) {
  if (!s) return LSPCG_OK;
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->stream);
  s->graphs.clear();
  multi_destroy(s);
  for (void* v : {s->x, s->b, s->r, s->z, s->t, s->p, s->d}) (void)hipFree(v);
  if (s->q != s->t) (void)hipFree(s->q);
  (void)hipFree(s->S);
  (void)hipHostFree(s->hS);
  (void)hipFree(s->partials);
  (void)hipFree(s->ticket);
  (void)hipFree(s->groups);
  for (hipEvent_t e : {s->ev_in, s->ev_out, s->ev_poll, s->ev_poll2, s->ev_t0, s->ev_t1}) (void)hipEventDestroy(e);
  if (s->LT) lspcg_mat_destroy(s->LT);
  if (s->Lp) lspcg_mat_destroy(s->Lp);
  if (s->LTo) lspcg_mat_destroy(s->LTo);
  if (s->Ap) lspcg_mat_destroy(s->Ap);
  s->ro.release();
  if (s->icL) lspcg_mat_destroy(s->icL);
  if (s->icU) lspcg_mat_destroy(s->icU);
  s->planL.release();
  s->planU.release();
  for (void* p : {s->own_A, s->own_L, s->own_LT}) (void)hipFree(p);
  for (int w = 0; w < 3; ++w) {
    (void)hipFree(s->sv[w]);
    s->spat[w].release();
  }
  (void)hipFree(s->flag);
  (void)hipFree(s->ob_part);
  (void)hipFree(s->dhist);
  (void)hipHostFree(s->hhist);
  (void)hipFree(s->dcoef);
  (void)hipHostFree(s->hcoef);
  (void)hipHostFree(s->hflags);
  (void)hipStreamDestroy(s->stream);
  delete s;
  return LSPCG_OK;
}

}  // extern "C"

