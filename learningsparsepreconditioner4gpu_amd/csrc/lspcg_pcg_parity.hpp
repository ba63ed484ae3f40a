// Parity (OpenBLAS-order) dots of the single-system PCG loop: the k_dot_openblas* kernels and the
// launcher that follows every reducing launch in that mode.  Included by lspcg_pcg.hip only (the
// batched solver has no parity mode).
#pragma once

#include "lspcg_pcg_kernels.hpp"
#include "lspcg_solver.hpp"

namespace lspcg {

// ---- OpenBLAS-order dots (lspcg_solver_set_dot_order(s, LSPCG_DOT_OPENBLAS, threads)) --------
// Parity mode: the dots and norms of the loop are recomputed in the summation order of the
// reference's own recorded runs -- numpy's cblas_ddot = OpenBLAS 0.3.29, SkylakeX kernel, split
// over `threads` OpenBLAS threads for n > 10000 (oracle/openblas_ddot.c restates the algorithm and
// cites it): per chunk, 32 FMA accumulators (element i into i % 32) over the 32-aligned prefix,
// folded 8 -> 4 lanes, one 16-element step on 4 x 4 lanes, a fixed lane tree, then a sequential
// FMA tail; chunks summed in order.  One workgroup; each wave owns one (dot, chunk) item at a
// time, lanes 0..31 its accumulators.  The launch follows the reducing launch whose scalars it
// replaces (same predicate on `done`), so the loop's order of state updates is unchanged.
constexpr int kObMaxThreads = 16;
constexpr int kObBlock = 512;  // 8 waves: <= 256 VGPRs for the two register buffers
constexpr int64_t kObSplitN = 131072;  // from this n the parity dots run one workgroup per (dot, chunk)

// chunk c of OpenBLAS's blas_level1_thread split of [0, n) (width = ceil(rest / threads left))
__device__ __forceinline__ void ob_chunk(int64_t n, int nch, int c, int64_t* start, int64_t* width) {
  int64_t m = n, s = 0, w = 0;
  for (int t = 0; t <= c; ++t) {
    w = (m + (nch - t) - 1) / (nch - t);
    m -= w;
    if (m < 0) w += m;
    if (t < c) s += w;
  }
  *start = s;
  *width = w > 0 ? w : 0;
}

// dot_compute(w, x, y) of one chunk (ob_chains, then ob_finish); the result is returned to every
// lane of the wave.  Each accumulator's FMA chain is sequential, so the loads set the time: groups
// of kObU 32-element steps are double-buffered in registers (group g + 1's loads in flight while group g's
// FMAs run; prefetch addresses are clamped instead of branched, so the compiler's in-order vmcnt
// waits never drain the other buffer), and the remainder and tail are loaded at once.  BASELINE
// config 1 (n = 10,240): 8.7 us per launch against 15-16 with flat loads and one 8-step batch
// (~18 GB/s: one wave's loads in flight); a third buffer measured the same, and staging tiles
// through LDS with every wave loading (one barrier per 16-step tile) measured slower (~19 us).
constexpr int kObU = 16;   // steps per register buffer, single-workgroup kernel (8 waves: <= 256 VGPRs)
constexpr int kObU1 = 32;  // the split kernel's one-wave workgroups hold twice as many steps in flight

template <int U>
__device__ __forceinline__ void ob_load(const double* __restrict__ x, const double* __restrict__ y, int64_t i,
                                        double (&xv)[U], double (&yv)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    xv[u] = x[i + 32 * u];
    yv[u] = y[i + 32 * u];
  }
}

template <int U>
__device__ __forceinline__ double ob_fma(const double (&xv)[U], const double (&yv)[U], double acc) {
#pragma unroll
  for (int u = 0; u < U; ++u) acc = __builtin_fma(xv[u], yv[u], acc);
  return acc;
}

// the 32 accumulators over the 32-aligned prefix (lanes 0..31; one wave reads everything)
template <int U = kObU>
__device__ __forceinline__ double ob_chains(const double* __restrict__ x, const double* __restrict__ y, int64_t w) {
  const int lane = threadIdx.x & 63;
  const int64_t n32 = (w & -int64_t(16)) & ~int64_t(31);
  double acc = 0.0;
  if (lane < 32) {
    constexpr int64_t GW = 32 * U;  // elements per group
    const int64_t G = n32 / GW;
    double ax[U], ay[U], bx[U], by[U];
    int64_t g = 0;
    if (G > 0) ob_load<U>(x, y, lane, ax, ay);
    for (; g + 1 < G; g += 2) {
      ob_load<U>(x, y, (g + 1) * GW + lane, bx, by);
      acc = ob_fma<U>(ax, ay, acc);
      ob_load<U>(x, y, (g + 2 < G ? g + 2 : g + 1) * GW + lane, ax, ay);
      acc = ob_fma<U>(bx, by, acc);
    }
    if (g < G) acc = ob_fma<U>(ax, ay, acc);
    // the remaining < U steps, loaded at once and added in order
    const int64_t base = G * GW;
    const int rem = int((n32 - base) >> 5);
    if (rem > 0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + (u < rem ? 32 * u : 0) + lane;
        bx[u] = x[i];
        by[u] = y[i];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (u < rem) acc = __builtin_fma(bx[u], by[u], acc);
    }
  }
  return acc;
}

// fold, 16-element step, lane tree and sequential tail of one chunk from its accumulators
__device__ __forceinline__ double ob_finish(const double* __restrict__ x, const double* __restrict__ y, int64_t w,
                                            double acc) {
  const int lane = threadIdx.x & 63;
  const int64_t n1 = w & -int64_t(16);
  const int64_t n32 = n1 & ~int64_t(31);
  // fold the 512-bit accumulators: lane 8v + j (j < 4) <- acc[8v + j] + acc[8v + 4 + j]
  double a = acc + __shfl_down(acc, 4, 64);
  if (n1 > n32 && lane < 32 && (lane & 7) < 4) {
    const int64_t e = n32 + 4 * (lane >> 3) + (lane & 3);
    a = __builtin_fma(x[e], y[e], a);
  }
  const int j = lane & 3;
  const double s = ((__shfl(a, j, 64) + __shfl(a, 8 + j, 64)) + __shfl(a, 16 + j, 64)) + __shfl(a, 24 + j, 64);
  double dot = (__shfl(s, 0, 64) + __shfl(s, 2, 64)) + (__shfl(s, 1, 64) + __shfl(s, 3, 64));
  // sequential tail of < 16 elements, loaded at once
  const int nt = int(w - n1);
  double tx = 0.0, ty = 0.0;
  if (lane < nt) {
    tx = x[n1 + lane];
    ty = y[n1 + lane];
  }
  for (int t = 0; t < nt; ++t) dot = __builtin_fma(__shfl(ty, t, 64), __shfl(tx, t, 64), dot);
  return dot;
}

template <int U = kObU>
__device__ __forceinline__ double ob_chunk_dot(const double* __restrict__ x, const double* __restrict__ y, int64_t w) {
  return ob_finish(x, y, w, ob_chains<U>(x, y, w));
}

enum ObWhich { kObInit = 0, kObZ = 1, kObQ = 2, kObR = 3, kObRho = 4, kObRR = 5 };

// up to 3 dots (xs[j] · ys[j]); thread 0 then writes the scalars of phase WHICH:
//   kObInit  rr = r·r, bb = b·b, atol, rho = (DIAG ? r·z : rr), done (‖b‖ = 0), hist[0]
//   kObZ     rho = r·z ; rr = r·r and hist[k] for k > 0           (after KB's EpiZ)
//   kObQ     pq = p·q ; alpha = rho / pq ; the recorded (rho, pq)  (after KC's EpiQ, whose pair it rewrites)
//   kObR     rr = r·r ; rho = (DIAG ? r·z : rr) ; hist[k]           (after CG / Jacobi k_update_r)
//   kObRho   rho = r·z                                             (after IC's k_dot_rho)
//   kObRR    rr = r·r ; hist[k]                                    (after IC's k_update_r)
// thread 0's scalar update of phase WHICH from the dot values v[0..nd)
// COUNTED (kObQ only): KC's EpiQ has already counted the iteration (ext_spai), so the pair recorded
// here is iteration S->iter - 1's
template <int WHICH, bool DIAG, bool COUNTED = false>
__device__ __forceinline__ void ob_epilogue(PcgState* S, const double (&v)[3]) {
  const int64_t k = S->iter;
  if constexpr (WHICH == kObInit) {
    S->rr = v[0];
    S->bb = v[1];
    const double bn = sqrt(v[1]);
    S->atol = fmax(0.0, S->rtol * bn);
    S->rho = DIAG ? v[2] : v[0];
    S->done = (bn == 0.0) ? 1 : 0;
    if (S->hist) S->hist[0] = sqrt(v[0]);
  } else if constexpr (WHICH == kObZ) {
    S->rho = v[0];
    if (k > 0) {
      S->rr = v[1];
      if (S->hist) S->hist[k] = sqrt(v[1]);
    }
  } else if constexpr (WHICH == kObQ) {
    const double rho = S->rho;
    double* const coef = S->coef;
    S->pq = v[0];
    S->alpha = rho / v[0];
    keep_coef(coef, COUNTED ? k - 1 : k, rho, v[0]);
  } else if constexpr (WHICH == kObR) {
    S->rr = v[0];
    S->rho = DIAG ? v[1] : v[0];
    if (S->hist) S->hist[k] = sqrt(v[0]);
  } else if constexpr (WHICH == kObRho) {
    S->rho = v[0];
  } else {
    S->rr = v[0];
    if (S->hist) S->hist[k] = sqrt(v[0]);
  }
}

// the chunk totals of dot j summed in chunk order (numpy's threads joined in order)
__device__ __forceinline__ void ob_join(const double* part, int nd, int ch, double (&v)[3]) {
  for (int j = 0; j < 3; ++j) v[j] = 0.0;
  for (int j = 0; j < nd; ++j) {
    double d = 0.0;
    for (int c = 0; c < ch; ++c) d = d + part[j * kObMaxThreads + c];
    v[j] = ch > 1 ? d : part[j * kObMaxThreads];
  }
}

template <int WHICH, bool DIAG, bool COUNTED = false>
__global__ void __launch_bounds__(kObBlock) k_dot_openblas(int64_t n, int nch, int nd, PcgState* S, const double* x0,
                                                           const double* y0, const double* x1, const double* y1,
                                                           const double* x2, const double* y2) {
  __shared__ double part[3 * kObMaxThreads];
  if (WHICH != kObInit && S->done) return;
  const int ch = (n > 10000 && nch > 1) ? nch : 1;
  const int nw = blockDim.x >> 6;
  for (int item = threadIdx.x >> 6; item < nd * ch; item += nw) {
    const int j = item / ch, c = item % ch;
    int64_t s = 0, w = n;
    if (ch > 1) ob_chunk(n, ch, c, &s, &w);
    // selects, not an array of pointers: the loads stay global_load (a flat load's lgkmcnt forces
    // waits on ALL outstanding loads, which would serialise the two register buffers)
    const double* xj = j == 0 ? x0 : j == 1 ? x1 : x2;
    const double* yj = j == 0 ? y0 : j == 1 ? y1 : y2;
    const double v = ob_chunk_dot(xj + s, yj + s, w);
    if ((threadIdx.x & 63) == 0) part[j * kObMaxThreads + c] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double v[3];
  ob_join(part, nd, ch, v);
  ob_epilogue<WHICH, DIAG, COUNTED>(S, v);
}

// Large n (>= kObSplitN): one single-wave workgroup per (dot, chunk) item -- every chunk of every
// dot on its own CU, with twice the steps in flight per register buffer (kObU1) -- writing its
// chunk total to a scratch slot; k_dot_openblas_fin then joins them in order and updates the
// scalars (one more launch; the same bits).  (Feeding the chains from an LDS ring filled by 7
// producer waves measured slower: kuhn101 parity solve 591 vs 272 ms at 1 thread, 91 vs 50 ms at 8
// -- the LDS hand-off per 64-step tile costs more than the loads it hides)
template <int WHICH>
__global__ void __launch_bounds__(64) k_dot_openblas_item(int64_t n, int nch, const PcgState* S, double* part,
                                                          const double* x0, const double* y0, const double* x1,
                                                          const double* y1, const double* x2, const double* y2) {
  if (WHICH != kObInit && S->done) return;
  const int ch = (n > 10000 && nch > 1) ? nch : 1;
  const int j = int(blockIdx.x) / ch, c = int(blockIdx.x) % ch;
  int64_t s = 0, w = n;
  if (ch > 1) ob_chunk(n, ch, c, &s, &w);
  const double* xj = j == 0 ? x0 : j == 1 ? x1 : x2;
  const double* yj = j == 0 ? y0 : j == 1 ? y1 : y2;
  const double v = ob_chunk_dot<kObU1>(xj + s, yj + s, w);
  if (threadIdx.x == 0) part[j * kObMaxThreads + c] = v;
}

template <int WHICH, bool DIAG, bool COUNTED = false>
__global__ void k_dot_openblas_fin(int64_t n, int nch, int nd, PcgState* S, const double* part) {
  if (threadIdx.x != 0 || (WHICH != kObInit && S->done)) return;
  const int ch = (n > 10000 && nch > 1) ? nch : 1;
  double v[3];
  ob_join(part, nd, ch, v);
  ob_epilogue<WHICH, DIAG, COUNTED>(S, v);
}

// parity mode: every reducing launch is followed by k_dot_openblas, which rewrites its scalars
template <int WHICH, bool DIAG = false, bool COUNTED = false>
static void enqueue_ob(lspcg_solver* s, hipStream_t st, int nd, const void* x0, const void* y0,
                       const void* x1 = nullptr, const void* y1 = nullptr, const void* x2 = nullptr,
                       const void* y2 = nullptr) {
  if (s->dot_order != LSPCG_DOT_OPENBLAS) return;
  const int ch = (s->n > 10000 && s->dot_threads > 1) ? s->dot_threads : 1;
  const auto* X0 = static_cast<const double*>(x0);
  const auto* Y0 = static_cast<const double*>(y0);
  const auto* X1 = static_cast<const double*>(x1);
  const auto* Y1 = static_cast<const double*>(y1);
  const auto* X2 = static_cast<const double*>(x2);
  const auto* Y2 = static_cast<const double*>(y2);
  if (s->n >= kObSplitN) {  // large n: one CU per (dot, chunk), then the ordered join
    hipLaunchKernelGGL(k_dot_openblas_item<WHICH>, dim3(nd * ch), dim3(64), 0, st, s->n, s->dot_threads, s->S,
                       s->ob_part, X0, Y0, X1, Y1, X2, Y2);
    hipLaunchKernelGGL((k_dot_openblas_fin<WHICH, DIAG, COUNTED>), dim3(1), dim3(64), 0, st, s->n, s->dot_threads, nd, s->S,
                       static_cast<const double*>(s->ob_part));
    return;
  }
  const int waves = std::min(kObBlock / 64, std::max(1, nd * ch));
  hipLaunchKernelGGL((k_dot_openblas<WHICH, DIAG, COUNTED>), dim3(1), dim3(64 * waves), 0, st, s->n, s->dot_threads, nd, s->S,
                     X0, Y0, X1, Y1, X2, Y2);
}

}  // namespace lspcg
