// Baseline preconditioners of the reference's comparison rows (infer.py:310-321, pymathprim
// "ic" / "ainv") on the GPU:
//
//   IC(0)   A ≈ L Lᵀ, L with the pattern of tril(A)          -> lspcg_ic0, applied by two
//           level-scheduled triangular solves (lspcg_solver_set_ic / LSPCG_PRECOND_IC)
//   AINV(0) A⁻¹ ≈ Z D⁻¹ Zᵀ, Z unit upper with the pattern of triu(A) (Benzi & Tůma incomplete
//           A-biconjugation)                                  -> lspcg_ainv0 returns L = Z D^{-1/2},
//           applied as the ext_spai operator L Lᵀ (+ 0·r) by the SpMV path
//
// Arithmetic (operation order per entry) is fixed by oracle/precond.py; pymathprim's own
// versions are unvendored (parity unpinned).  All factorizations are level scheduled: a row
// (column) depends only on rows of earlier levels, so one launch per level computes every row
// of that level in parallel, one thread per row, with the sequential operation order of the
// oracle.  Levels come from relaxation sweeps (lev[i] = 1 + max lev over dependencies) and a
// stable radix sort of (level, row).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "lspcg_factor.hpp"
#include "lspcg_internal.hpp"

namespace lspcg {

static int fgrid(int64_t n) {
  const int64_t g = (n + kThreads - 1) / kThreads;
  return int(std::max<int64_t>(1, std::min<int64_t>(g, 8192)));
}

// ---------------------------------------------------------------------------
// tril pattern (scalar CSR, sorted rows): count / fill; flag 1 = a row without its diagonal
// ---------------------------------------------------------------------------
__global__ void k_tril_count(int64_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                             int32_t* __restrict__ cnt, int* flag) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int c = 0;
    bool diag = false;
    for (int p = rp[i]; p < rp[i + 1]; ++p) {
      const int j = ci[p];
      c += j <= i;
      diag |= j == i;
    }
    cnt[i] = c;
    if (!diag) atomicOr(flag, 1);
  }
}

template <typename T>
__global__ void k_tril_fill(int64_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                            const T* __restrict__ v, const int32_t* __restrict__ orp, int32_t* __restrict__ oci,
                            T* __restrict__ ov) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int o = orp[i];
    for (int p = rp[i]; p < rp[i + 1]; ++p) {
      const int j = ci[p];
      if (j <= i) {
        oci[o] = j;
        if (ov) ov[o] = v[p];
        ++o;
      }
    }
  }
}

// an owned matrix under construction: destroyed on scope exit unless handed out
using MatGuard = std::unique_ptr<lspcg_mat, int (*)(lspcg_mat*)>;

// L <- tril(A) (values copied when with_vals)
static int tril_of(const lspcg_mat* A, bool with_vals, lspcg_mat** out) {
  LSPCG_CHECK(A->block_size == 1, LSPCG_ERR_UNSUPPORTED, "tril: scalar CSR required (expand BSR first)");
  hipStream_t st = A->ctx->stream;
  const int64_t n = A->n;
  DevBuf B;
  int32_t *cnt = nullptr, *tmp_rp = nullptr;
  int* flag = nullptr;
  if (int rc = B.get(&cnt, n) | B.get(&flag, 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  launch(k_tril_count, dim3(fgrid(n)), dim3(kThreads), st, n, A->rowptr, A->colind, cnt, flag);
  int f = 0;
  if (int rc = flag_value(flag, st, &f)) return rc;
  LSPCG_CHECK(!f, LSPCG_ERR_FORMAT, "factor: a row of A has no stored diagonal entry");
  // count first, then allocate with the exact entry count
  int64_t total = 0;
  if (int rc = B.get(&tmp_rp, n + 1)) return rc;
  if (int rc = scan_to_rowptr(cnt, n, tmp_rp, &total, st)) return rc;
  lspcg_mat* L = nullptr;
  if (int rc = mat_alloc(A->ctx, n, total, 1, A->dtype, &L)) return rc;
  MatGuard guard(L, lspcg_mat_destroy);
  LSPCG_HIP(hipMemcpyAsync(L->rowptr, tmp_rp, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToDevice, st));
  by_dtype(A->dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_tril_fill<T>, dim3(fgrid(n)), dim3(kThreads), st, n, A->rowptr, A->colind, as<T>(A->vals), L->rowptr,
           L->colind, with_vals ? as<T>(L->vals) : nullptr);
  });
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipStreamSynchronize(st));
  *out = guard.release();
  return LSPCG_OK;
}

// ---------------------------------------------------------------------------
// level sets
// ---------------------------------------------------------------------------
template <bool LOWER>
__global__ void k_level_sweep(int64_t n, const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                              int32_t* lev, int* changed) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    int m = 0;
    for (int p = rp[i]; p < rp[i + 1]; ++p) {
      const int64_t j = ci[p];
      if (LOWER ? j < i : j > i) {
        const int l = __hip_atomic_load(lev + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        m = l > m ? l : m;
      }
    }
    if (m > lev[i]) {
      __hip_atomic_store(lev + i, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *changed = 1;
    }
  }
}

__global__ void k_iota(int64_t n, int32_t* v) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    v[i] = int32_t(i);
}

// sorted levels -> ptr[l] = first position of level l (levels are contiguous 0..max)
__global__ void k_level_bounds(int64_t n, const int32_t* __restrict__ ls, int32_t* __restrict__ ptr) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int l = ls[i];
    const int prev = i == 0 ? -1 : ls[i - 1];
    for (int q = prev + 1; q <= l; ++q) ptr[q] = int32_t(i);
    if (i == n - 1) ptr[l + 1] = int32_t(n);
  }
}

void Levels::release() {
  (void)hipFree(order);
  order = nullptr;
  hptr.clear();
  nlev = 0;
}

void TrsvPlan::release() {
  for (void* p : {(void*)pad, (void*)head, sv, inv, c}) (void)hipFree(p);
  *this = TrsvPlan{};
}

// position t of the level-sorted order -> its place in the wave-padded order
__global__ void k_pad_order(int64_t n, const int32_t* __restrict__ lev_s, const int32_t* __restrict__ ptr,
                            const int32_t* __restrict__ pptr, const int32_t* __restrict__ order, int32_t* __restrict__ pad) {
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < n; t += int64_t(gridDim.x) * blockDim.x) {
    const int l = lev_s[t];
    pad[pptr[l] + (t - ptr[l])] = order[t];
  }
}

// The level sort of n > 0 rows, in B's scratch: lev_s = the sorted levels, order = the rows by
// (level, row), ptr (device) / hptr (host) = each level's first position
struct LevelSort {
  int32_t *lev_s = nullptr, *order = nullptr, *ptr = nullptr;
  std::vector<int32_t> hptr;
};

static int sort_levels(lspcg_ctx* ctx, int64_t n, const int32_t* rp, const int32_t* ci, bool lower, DevBuf& B,
                       LevelSort* S) {
  hipStream_t st = ctx->stream;
  int32_t *lev = nullptr, *lev_s = nullptr, *iota = nullptr, *order = nullptr, *ptr = nullptr;
  int* changed = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  if (int rc = B.get(&lev, n) | B.get(&lev_s, n) | B.get(&iota, n) | B.get(&order, n) | B.get(&changed, 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(lev, 0, sizeof(int32_t) * n, st));
  // relaxation sweeps until a round of sweeps changes nothing (<= longest dependency chain + 1
  // sweeps); kSweepRound sweeps per host check of the flag (extra sweeps change nothing)
  constexpr int kSweepRound = 8;
  int h = 1;
  for (int64_t sweep = 0; h && sweep <= n; sweep += kSweepRound) {
    LSPCG_HIP(hipMemsetAsync(changed, 0, sizeof(int), st));
    for (int r = 0; r < kSweepRound; ++r)
      by_flag(lower, [&](auto lo) {
        launch(k_level_sweep<decltype(lo)::value>, dim3(fgrid(n)), dim3(kThreads), st, n, rp, ci, lev, changed);
      });
    if (int rc = flag_value(changed, st, &h)) return rc;
  }
  launch(k_iota, dim3(fgrid(n)), dim3(kThreads), st, n, iota);
  LSPCG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, lev, lev_s, iota, order, int(n), 0, 32, st));
  if (int rc = B.get(&tmp, tmp_bytes)) return rc;
  LSPCG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, lev, lev_s, iota, order, int(n), 0, 32, st));
  int32_t maxl = 0;
  if (int rc = flag_value(lev_s + n - 1, st, &maxl)) return rc;
  if (int rc = B.get(&ptr, maxl + 2)) return rc;
  launch(k_level_bounds, dim3(fgrid(n)), dim3(kThreads), st, n, lev_s, ptr);
  S->hptr.resize(maxl + 2);
  LSPCG_HIP(hipMemcpyAsync(S->hptr.data(), ptr, sizeof(int32_t) * (maxl + 2), hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  S->lev_s = lev_s;
  S->order = order;
  S->ptr = ptr;
  return LSPCG_OK;
}

int build_levels(lspcg_ctx* ctx, int64_t n, const int32_t* rp, const int32_t* ci, bool lower, Levels* out) {
  out->release();
  if (n == 0) {
    out->hptr = {0};
    return LSPCG_OK;
  }
  DevBuf B;
  LevelSort S;
  if (int rc = sort_levels(ctx, n, rp, ci, lower, B, &S)) return rc;
  out->nlev = int(S.hptr.size()) - 1;
  out->hptr = std::move(S.hptr);
  out->order = B.keep(S.order);
  return LSPCG_OK;
}

// Two-pointer merge of the sorted column lists ca[a..ae) and cb[b..be): on(a, b) at every common
// column, in increasing column order (the oracle's order of operations)
template <class F>
__device__ __forceinline__ void merge_sorted(int a, int ae, const int32_t* ca, int b, int be, const int32_t* cb,
                                             F on) {
  while (a < ae && b < be) {
    const int x = ca[a], y = cb[b];
    if (x == y) {
      on(a, b);
      ++a;
      ++b;
    } else if (x < y) {
      ++a;
    } else {
      ++b;
    }
  }
}

// ---------------------------------------------------------------------------
// IC(0): one thread per row of the level; oracle/precond.py ic0 operation order
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_ic0_level(const int32_t* __restrict__ order, int32_t beg, int32_t cnt,
                            const int32_t* __restrict__ rp, const int32_t* __restrict__ ci, T* __restrict__ L,
                            int* flag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cnt) return;
  const int i = order[beg + t];
  const int pb = rp[i], pd = rp[i + 1] - 1;  // diagonal is the last entry of a tril row
  for (int p = pb; p < pd; ++p) {
    const int k = ci[p];
    T s = L[p];
    // merge the already computed part of row i (columns < k) with row k (off-diagonal part)
    const int be = rp[k + 1] - 1;
    merge_sorted(pb, p, ci, rp[k], be, ci, [&](int a, int b) { s = s - L[a] * L[b]; });
    L[p] = s / L[be];
  }
  T s = L[pd];
  for (int a = pb; a < pd; ++a) s = s - L[a] * L[a];
  if (!(s > T(0))) {
    atomicOr(flag, 1);
    s = T(1);
  }
  L[pd] = sqrt(s);
}

// ---------------------------------------------------------------------------
// triangular solves (LOWER: diagonal stored last in each row, UPPER: first)
// ---------------------------------------------------------------------------
// Sync-free solve: ONE launch for the whole triangular solve instead of one per level.  A
// resident grid (1 workgroup per CU: few polling waves per CU, short hand-offs) takes 256-position
// blocks of the wave-padded level order from a dequeue counter, in order, so a block only ever
// waits for blocks that running workgroups hold; thread t of block B owns position B*256 + t,
// waits for its dependencies' values (all still-missing ones re-read together per poll round,
// the row's values loaded beforehand) and runs scipy spsolve_triangular's arithmetic (the
// reference's IC apply, validate.py:359-365; oracle/precond.py restates it): a unit solve on the
// column-scaled factor, the row's updates in SuperLU's column order, then k_trsv_post.  The
// hand-off is the value itself: x is first filled with a NaN pattern no arithmetic produces, each
// row publishes its result with one 4- / 8-byte sc1 store (a self-validating granule,
// MI355X_MICROARCH.md R2) and waiters poll with sc1 loads.  A wave never holds rows of two
// levels, so no lane waits for a lane of its own wave.  Forward progress: a block waits only for
// blocks dequeued before it, which resident workgroups hold.  Every wave still has an exit: a row
// whose wait exceeds 2 s (a finished solve's chain is ~2 us per level) raises the levels' error
// word (head[1]) and takes NaN; lspcg_solver_solve / lspcg_trsv then fail with LSPCG_ERR_HIP
// instead of returning a result.
template <typename T>
struct TrsvBits;
template <>
struct TrsvBits<double> {
  using U = unsigned long long;
  static constexpr U kWait = 0x7FF4C0DEDEADBEEFull;  // signalling-NaN payload: never an arithmetic result
};
template <>
struct TrsvBits<float> {
  using U = unsigned;
  static constexpr U kWait = 0x7FA5C0DEu;
};

constexpr int kTrsvBatch = 8;

// read of a dependency's value: an sc1 load (an atomic RMW poll measured the same)
template <typename U>
__device__ __forceinline__ U trsv_poll(const U* p) {
  return __hip_atomic_load(const_cast<U*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (also resets the block dequeue counter head[0] for the launch that follows.  Observed with the reset
// as a hipMemsetAsync node between the kernel nodes of the iteration graph: once other work with a
// host read had run on the context's stream between two solves, replays gave NaN from the second
// triangular solve on, until a device-wide synchronize or a re-capture; with the reset here they do
// not.  Supposed, not shown: the node was no longer ordered before the launch, so the counter still
// held the previous solve's value, every workgroup left at once and x kept the wait pattern.)
template <typename T>
__global__ void k_trsv_wait_fill(int64_t n, T* __restrict__ x, const int32_t* done, unsigned* head) {
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(head, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (done && *done) return;
  using U = typename TrsvBits<T>::U;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    reinterpret_cast<U*>(x)[i] = TrsvBits<T>::kWait;
}

template <typename T, bool LOWER>
__global__ void __launch_bounds__(256) k_trsv_syncfree(int64_t npad, const int32_t* __restrict__ pad,
                                                       const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                       const T* __restrict__ sv, const T* __restrict__ b, T* x,
                                                       const int32_t* done, unsigned* head) {
  using U = typename TrsvBits<T>::U;
  __shared__ unsigned s_blk;
  if (done && *done) return;
  U* xu = reinterpret_cast<U*>(x);
  const unsigned nblk = unsigned((npad + 255) / 256);
  for (;;) {
    // the workgroup takes the next 256-position block (per-wave 64-position blocks measured slower:
    // 4x the dequeues on one counter)
    if (threadIdx.x == 0) s_blk = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const unsigned blk = s_blk;
    __syncthreads();
    if (blk >= nblk) return;  // every workgroup leaves through here once the blocks are taken
    const uint64_t t0 = wall_clock64();  // the block's waits are bounded from here
    const int64_t t = int64_t(blk) * 256 + threadIdx.x;
    const int i = t < npad ? pad[t] : -1;
    if (i >= 0) {
      T s = b[i];
      // the off-diagonal entries of row i, visited in spsolve_triangular's update order:
      // increasing column (lower, diagonal last) / decreasing column (upper, diagonal first)
      const int cnt = rp[i + 1] - rp[i] - 1;
      auto entry = [&](int k) { return LOWER ? rp[i] + k : rp[i + 1] - 1 - k; };
      // the dependencies' values are loaded kTrsvBatch at a time, and every poll round re-reads ALL
      // still-waiting ones together: one memory latency per round, not one per entry; the sum
      // then runs in update order
      for (int kb = 0; kb < cnt; kb += kTrsvBatch) {
        U u[kTrsvBatch];
        T w[kTrsvBatch];  // the row's scaled values, loaded before the wait (not after the last hand-off)
        const U* src[kTrsvBatch];
#pragma unroll
        for (int k = 0; k < kTrsvBatch; ++k) {
          const int q = entry(kb + k < cnt ? kb + k : 0);
          src[k] = xu + ci[q];
          w[k] = sv[q];
        }
#pragma unroll
        for (int k = 0; k < kTrsvBatch; ++k) u[k] = trsv_poll(src[k]);
        for (;;) {
          bool wait = false;
#pragma unroll
          for (int k = 0; k < kTrsvBatch; ++k) wait |= (kb + k < cnt) && u[k] == TrsvBits<T>::kWait;
          if (!wait) break;
          if (wall_clock64() - t0 > 200000000ull) {  // 2 s at the 100 MHz constant clock
            __hip_atomic_store(head + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < kTrsvBatch; ++k)
              if (u[k] == TrsvBits<T>::kWait) u[k] = __builtin_bit_cast(U, T(NAN));
            break;
          }
          __builtin_amdgcn_s_sleep(2);
#pragma unroll
          for (int k = 0; k < kTrsvBatch; ++k)
            if (u[k] == TrsvBits<T>::kWait) u[k] = trsv_poll(src[k]);
        }
#pragma unroll
        for (int k = 0; k < kTrsvBatch; ++k)
          if (kb + k < cnt) s = s - __builtin_bit_cast(T, u[k]) * w[k];
      }
      // unit triangular solve: the published value is y_i itself (k_trsv_post scales it)
      __hip_atomic_store(xu + i, __builtin_bit_cast(U, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// spsolve_triangular's column scaling: inv_i = 1 / d_i, c_i = d_i inv_i (the scaled diagonal the
// lower solve's U phase divides by), then sv_p = v_p inv_{col p}
template <typename T, bool LOWER>
__global__ void k_trsv_inv(int64_t n, const int32_t* __restrict__ rp, const T* __restrict__ v, T* __restrict__ inv,
                           T* __restrict__ c) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const T d = v[LOWER ? rp[i + 1] - 1 : rp[i]];
    const T iv = T(1) / d;
    inv[i] = iv;
    c[i] = d * iv;
  }
}

template <typename T>
__global__ void k_trsv_scale(int64_t nnz, const int32_t* __restrict__ ci, const T* __restrict__ v,
                             const T* __restrict__ inv, T* __restrict__ sv) {
  for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < nnz; p += int64_t(gridDim.x) * blockDim.x)
    sv[p] = v[p] * inv[ci[p]];
}

// x_i = (y_i / c_i) inv_i (lower: SuperLU's U phase divides by the scaled diagonal) or y_i inv_i
// (upper: its L phase divides by the identity's 1)
template <typename T, bool LOWER>
__global__ void k_trsv_post(int64_t n, T* __restrict__ x, const T* __restrict__ c, const T* __restrict__ inv,
                            const int32_t* done) {
  if (done && *done) return;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    if constexpr (LOWER) x[i] = (x[i] / c[i]) * inv[i];
    else x[i] = x[i] * inv[i];
  }
}

int trsv_plan_build(const lspcg_mat* T_, bool lower, TrsvPlan* out) {
  LSPCG_CHECK(T_->block_size == 1 && T_->storage_dtype() == T_->dtype, LSPCG_ERR_UNSUPPORTED,
              "trsv: scalar CSR with plain storage required");
  out->release();
  hipStream_t st = T_->ctx->stream;
  const int64_t n = T_->n, nnz = T_->nnzb;
  if (n == 0) return LSPCG_OK;
  DevBuf B;
  LevelSort S;
  if (int rc = sort_levels(T_->ctx, n, T_->rowptr, T_->colind, lower, B, &S)) return rc;
  // every level padded to whole wave64s
  const int nlev = int(S.hptr.size()) - 1;
  std::vector<int32_t> pptr(nlev + 1, 0);
  for (int l = 0; l < nlev; ++l) pptr[l + 1] = pptr[l] + (S.hptr[l + 1] - S.hptr[l] + 63) / 64 * 64;
  const int64_t npad = pptr[nlev];
  int32_t *dpptr = nullptr, *pad = nullptr;
  unsigned* head = nullptr;  // [dequeue counter | timeout flag]
  if (int rc = B.get(&dpptr, nlev + 1) | B.get(&pad, npad) | B.get(&head, 2)) return rc;
  LSPCG_HIP(hipMemcpy(dpptr, pptr.data(), sizeof(int32_t) * (nlev + 1), hipMemcpyHostToDevice));
  LSPCG_HIP(hipMemsetAsync(pad, 0xFF, sizeof(int32_t) * npad, st));
  launch(k_pad_order, dim3(fgrid(n)), dim3(kThreads), st, n, S.lev_s, S.ptr, dpptr, S.order, pad);
  LSPCG_HIP(hipMemsetAsync(head, 0, 2 * sizeof(unsigned), st));
  LSPCG_HIP(hipStreamSynchronize(st));
  out->pad = B.keep(pad);
  out->npad = npad;
  out->head = B.keep(head);
  B.release();  // the sort's scratch, while nothing is enqueued
  if (hipDeviceGetAttribute(&out->cus, hipDeviceAttributeMultiprocessorCount, T_->ctx->device) != hipSuccess ||
      out->cus <= 0)
    out->cus = 256;
  // the scaled values: enqueued, not waited for
  const int rc = by_dtype(T_->dtype, [&](auto t) -> int {
    using T = decltype(t);
    T *sv = nullptr, *inv = nullptr, *c = nullptr;
    if (int rc = B.get(&sv, nnz) | B.get(&inv, n) | B.get(&c, n)) return rc;
    out->sv = B.keep(sv);
    out->inv = B.keep(inv);
    out->c = B.keep(c);
    return trsv_plan_refill(T_, lower, *out);
  });
  if (rc) out->release();
  return rc;
}

int trsv_plan_refill(const lspcg_mat* T_, bool lower, const TrsvPlan& plan) {
  hipStream_t st = T_->ctx->stream;
  const int64_t n = T_->n, nnz = T_->nnzb;
  if (n == 0) return LSPCG_OK;
  LSPCG_CHECK(plan.sv && plan.inv && plan.c, LSPCG_ERR_ARG, "trsv: no plan to refill");
  return by_dtype(T_->dtype, [&](auto t) -> int {
    using T = decltype(t);
    T *sv = as<T>(plan.sv), *inv = as<T>(plan.inv), *c = as<T>(plan.c);
    by_flag(lower, [&](auto lo) {
      launch(k_trsv_inv<T, decltype(lo)::value>, dim3(fgrid(n)), dim3(kThreads), st, n, T_->rowptr, as<T>(T_->vals),
             inv, c);
    });
    if (nnz) launch(k_trsv_scale<T>, dim3(fgrid(nnz)), dim3(kThreads), st, nnz, T_->colind, as<T>(T_->vals), inv, sv);
    LSPCG_HIP(hipGetLastError());
    return LSPCG_OK;
  });
}

int enqueue_trsv(const lspcg_mat* T_, const TrsvPlan& plan, bool lower, const void* b, void* x, const int32_t* done,
                 hipStream_t st) {
  if (plan.npad <= 0) return LSPCG_OK;
  const int64_t n = T_->n;
  // 1 workgroup per CU (2 or 4 measured slower: more polling waves)
  const dim3 g(unsigned(std::min<int64_t>((plan.npad + 255) / 256, int64_t(plan.cus)))), blk(256);
  by_dtype(T_->dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_trsv_wait_fill<T>, dim3(fgrid(n)), dim3(kThreads), st, n, as<T>(x), done, plan.head);
    by_flag(lower, [&](auto lo) {
      constexpr bool LOWER = decltype(lo)::value;
      launch(k_trsv_syncfree<T, LOWER>, g, blk, st, plan.npad, plan.pad, T_->rowptr, T_->colind, as<T>(plan.sv),
             as<T>(b), as<T>(x), done, plan.head);
      launch(k_trsv_post<T, LOWER>, dim3(fgrid(n)), dim3(kThreads), st, n, as<T>(x), as<T>(plan.c), as<T>(plan.inv),
             done);
    });
  });
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

int trsv_check_timeout(const TrsvPlan& plan, hipStream_t st) {
  if (!plan.head) return LSPCG_OK;
  int h = 0;
  if (int rc = flag_value(reinterpret_cast<const int*>(plan.head + 1), st, &h)) return rc;
  if (h) {
    LSPCG_HIP(hipMemsetAsync(plan.head + 1, 0, sizeof(unsigned), st));
    LSPCG_HIP(hipStreamSynchronize(st));
    set_error("triangular solve: a row waited more than 2 s for a dependency (sync-free hand-off timed out); "
              "the result is invalid");
    return LSPCG_ERR_HIP;
  }
  return LSPCG_OK;
}

// the level launches of IC(0) on L = tril(A)'s values; LSPCG_ERR_BREAKDOWN on a non-positive pivot
static int ic0_levels(lspcg_mat* L, const Levels& lv) {
  hipStream_t st = L->ctx->stream;
  DevBuf B;
  int* flag = nullptr;
  if (int rc = B.get(&flag, 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  by_dtype(L->dtype, [&](auto t) {
    using T = decltype(t);
    for (int l = 0; l < lv.nlev; ++l) {
      const int beg = lv.hptr[l], cnt = lv.hptr[l + 1] - lv.hptr[l];
      launch(k_ic0_level<T>, dim3((cnt + 127) / 128), dim3(128), st, lv.order, beg, cnt, L->rowptr, L->colind,
             as<T>(L->vals), flag);
    }
  });
  LSPCG_HIP(hipGetLastError());
  int f = 0;
  if (int rc = flag_value(flag, st, &f)) return rc;
  LSPCG_CHECK(!f, LSPCG_ERR_BREAKDOWN,
              "IC(0) breakdown: a non-positive pivot (the matrix is not an M-matrix / not SPD)");
  return LSPCG_OK;
}

int ic0_factor(const lspcg_mat* A, lspcg_mat** out, Levels* levels) {
  LSPCG_CHECK(A && out, LSPCG_ERR_ARG, "ic0: NULL");
  lspcg_mat* L = nullptr;
  if (int rc = tril_of(A, true, &L)) return rc;
  MatGuard guard(L, lspcg_mat_destroy);
  Levels own;
  Levels& lv = levels ? *levels : own;
  if (int rc = build_levels(A->ctx, L->n, L->rowptr, L->colind, true, &lv)) return rc;
  if (int rc = ic0_levels(L, lv)) return rc;
  *out = guard.release();
  return LSPCG_OK;
}

int ic0_numeric(const lspcg_mat* A, lspcg_mat* L, const Levels& lv) {
  LSPCG_CHECK(A && L, LSPCG_ERR_ARG, "ic0: NULL");
  LSPCG_CHECK(A->block_size == 1 && L->block_size == 1 && A->n == L->n && A->dtype == L->dtype &&
                  int64_t(lv.hptr.size()) == int64_t(lv.nlev) + 1 && (L->n == 0 || lv.hptr.back() == L->n),
              LSPCG_ERR_ARG, "ic0_numeric: L and its levels do not belong to A");
  hipStream_t st = A->ctx->stream;
  // L <- tril(A)'s values at L's row pointers (the columns it rewrites are the ones L has)
  by_dtype(A->dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_tril_fill<T>, dim3(fgrid(A->n)), dim3(kThreads), st, A->n, A->rowptr, A->colind, as<T>(A->vals), L->rowptr,
           L->colind, as<T>(L->vals));
  });
  LSPCG_HIP(hipGetLastError());
  return ic0_levels(L, lv);
}

// ---------------------------------------------------------------------------
// AINV(0)
// ---------------------------------------------------------------------------
constexpr int kAinvMaxP = 64;  // |P_j| = entries of tril row j supported by the k-way merge

// candidates C_j = sorted unique {i < j : row i of A meets P_j} = U_{k in P_j} {i in row k of A, i < j}
// (symmetric pattern).  COUNT pass writes cnt[j]; FILL pass writes the list at cp[j].
template <bool FILL>
__global__ void k_ainv_cand(int64_t n, const int32_t* __restrict__ arp, const int32_t* __restrict__ aci,
                            const int32_t* __restrict__ trp, const int32_t* __restrict__ tci, int32_t* cnt,
                            const int32_t* __restrict__ cp, int32_t* __restrict__ cidx, int* flag) {
  for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += int64_t(gridDim.x) * blockDim.x) {
    const int pb = trp[j], pe = trp[j + 1];
    const int np = pe - pb;
    if (np > kAinvMaxP) {
      atomicOr(flag, 2);
      if (!FILL) cnt[j] = 0;
      continue;
    }
    int cur[kAinvMaxP], end[kAinvMaxP];
    for (int u = 0; u < np; ++u) {
      const int k = tci[pb + u];
      cur[u] = arp[k];
      end[u] = arp[k + 1];
    }
    int c = 0;
    int last = -1;
    int o = FILL ? cp[j] : 0;
    for (;;) {
      int mn = 0x7fffffff;
      for (int u = 0; u < np; ++u)
        if (cur[u] < end[u]) {
          const int v = aci[cur[u]];
          mn = v < mn ? v : mn;
        }
      if (mn >= j) break;  // every remaining head is >= j (rows are sorted)
      for (int u = 0; u < np; ++u)
        if (cur[u] < end[u] && aci[cur[u]] == mn) ++cur[u];
      if (mn != last) {
        if (FILL) cidx[o++] = mn;
        ++c;
        last = mn;
      }
    }
    if (!FILL) cnt[j] = c;
  }
}

// column j of Z (values z[trp[j]..trp[j+1]), pattern tci) and d_j; oracle/precond.py ainv0 order
template <typename T>
__global__ void k_ainv_level(const int32_t* __restrict__ order, int32_t beg, int32_t cnt,
                             const int32_t* __restrict__ arp, const int32_t* __restrict__ aci,
                             const T* __restrict__ av, const int32_t* __restrict__ trp,
                             const int32_t* __restrict__ tci, const int32_t* __restrict__ cp,
                             const int32_t* __restrict__ cidx, T* __restrict__ z, T* __restrict__ d, int* flag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cnt) return;
  const int j = order[beg + t];
  const int pb = trp[j], pe = trp[j + 1];
  for (int c = cp[j]; c < cp[j + 1]; ++c) {
    const int i = cidx[c];
    // p = a_i . z_j over P_j (increasing k)
    T p = T(0);
    merge_sorted(arp[i], arp[i + 1], aci, pb, pe, tci, [&](int a, int q) { p = p + av[a] * z[q]; });
    if (p != T(0)) {
      const T f = p / d[i];
      merge_sorted(trp[i], trp[i + 1], tci, pb, pe, tci, [&](int a, int q) { z[q] = z[q] - f * z[a]; });
    }
  }
  T dj = T(0);
  merge_sorted(arp[j], arp[j + 1], aci, pb, pe, tci, [&](int a, int q) { dj = dj + av[a] * z[q]; });
  if (!(dj > T(0))) {
    atomicOr(flag, 1);
    dj = T(1);
  }
  d[j] = dj;
}

template <typename T>
__global__ void k_ainv_init(int64_t n, const int32_t* __restrict__ trp, T* __restrict__ z) {
  for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += int64_t(gridDim.x) * blockDim.x) {
    for (int p = trp[j]; p < trp[j + 1] - 1; ++p) z[p] = T(0);
    z[trp[j + 1] - 1] = T(1);  // diagonal (last entry of the tril row)
  }
}

template <typename T>
__global__ void k_ainv_scale(int64_t n, const int32_t* __restrict__ trp, const T* __restrict__ d, T* __restrict__ z) {
  for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += int64_t(gridDim.x) * blockDim.x) {
    const T s = sqrt(d[j]);
    for (int p = trp[j]; p < trp[j + 1]; ++p) z[p] = z[p] / s;
  }
}

int ainv0_factor(const lspcg_mat* A, lspcg_mat** out) {
  LSPCG_CHECK(A && out, LSPCG_ERR_ARG, "ainv0: NULL");
  LSPCG_CHECK(A->storage_dtype() == A->dtype, LSPCG_ERR_ARG, "ainv0: compact-storage views are not accepted");
  hipStream_t st = A->ctx->stream;
  const int64_t n = A->n;
  lspcg_mat* Zt = nullptr;  // rows = columns of Z (pattern tril(A)), scaled by d^{-1/2} at the end
  if (int rc = tril_of(A, false, &Zt)) return rc;
  MatGuard guard(Zt, lspcg_mat_destroy);
  DevBuf B;
  Levels lv;
  int32_t *cnt = nullptr, *cp = nullptr, *cidx = nullptr;
  int* flag = nullptr;
  int64_t total = 0;
  if (int rc = B.get(&cnt, n) | B.get(&cp, n + 1) | B.get(&flag, 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  const dim3 g(fgrid(n)), blk(kThreads);
  launch(k_ainv_cand<false>, g, blk, st, n, A->rowptr, A->colind, Zt->rowptr, Zt->colind, cnt, nullptr, nullptr, flag);
  if (int rc = scan_to_rowptr(cnt, n, cp, &total, st)) return rc;
  if (int rc = B.get(&cidx, total)) return rc;
  launch(k_ainv_cand<true>, g, blk, st, n, A->rowptr, A->colind, Zt->rowptr, Zt->colind, cnt, cp, cidx, flag);
  int f = 0;
  if (int rc = flag_value(flag, st, &f)) return rc;
  LSPCG_CHECK(!(f & 2), LSPCG_ERR_UNSUPPORTED, "ainv0: a row of tril(A) has more than 64 entries (unsupported)");
  if (int rc = build_levels(A->ctx, n, cp, cidx, true, &lv)) return rc;
  const int rc = by_dtype(A->dtype, [&](auto t) -> int {
    using T = decltype(t);
    T *d = nullptr, *z = as<T>(Zt->vals);
    if (int rc = B.get(&d, n)) return rc;
    launch(k_ainv_init<T>, g, blk, st, n, Zt->rowptr, z);
    for (int l = 0; l < lv.nlev; ++l) {
      const int beg = lv.hptr[l], cnt_l = lv.hptr[l + 1] - lv.hptr[l];
      launch(k_ainv_level<T>, dim3((cnt_l + 127) / 128), dim3(128), st, lv.order, beg, cnt_l, A->rowptr, A->colind,
             as<T>(A->vals), Zt->rowptr, Zt->colind, cp, cidx, z, d, flag);
    }
    launch(k_ainv_scale<T>, g, blk, st, n, Zt->rowptr, d, z);
    LSPCG_HIP(hipGetLastError());
    return LSPCG_OK;
  });
  if (rc) return rc;
  if (int rc2 = flag_value(flag, st, &f)) return rc2;
  LSPCG_CHECK(!(f & 1), LSPCG_ERR_BREAKDOWN, "AINV(0) breakdown: a non-positive pivot");
  return lspcg_mat_transpose(Zt, out);  // L = (D^{-1/2} Zᵀ)ᵀ = Z D^{-1/2}
}

}  // namespace lspcg

using namespace lspcg;

extern "C" {

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int lspcg_ic0(const lspcg_mat* A, lspcg_mat** L, double* t_ms) {
  LSPCG_CHECK(A && L, LSPCG_ERR_ARG, "ic0: NULL");
  LSPCG_HIP(hipSetDevice(A->ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = ic0_factor(A, L);
  if (t_ms) *t_ms = ms_since(t0);
  return rc;
}

int lspcg_ainv0(const lspcg_mat* A, lspcg_mat** L, double* t_ms) {
  LSPCG_CHECK(A && L, LSPCG_ERR_ARG, "ainv0: NULL");
  LSPCG_HIP(hipSetDevice(A->ctx->device));
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = ainv0_factor(A, L);
  if (t_ms) *t_ms = ms_since(t0);
  return rc;
}

int lspcg_trsv(const lspcg_mat* T, int lower, const void* b, void* x) {
  LSPCG_CHECK(T && (T->n == 0 || (b && x)), LSPCG_ERR_ARG, "trsv: NULL");
  LSPCG_CHECK(T->block_size == 1 && T->storage_dtype() == T->dtype, LSPCG_ERR_UNSUPPORTED,
              "trsv: scalar CSR with plain storage required");
  LSPCG_HIP(hipSetDevice(T->ctx->device));
  TrsvPlan plan;
  int rc = trsv_plan_build(T, lower != 0, &plan);
  if (!rc) rc = enqueue_trsv(T, plan, lower != 0, b, x, nullptr, T->ctx->stream);
  if (!rc && hipStreamSynchronize(T->ctx->stream) != hipSuccess) {
    set_error("trsv: stream synchronize failed");
    rc = LSPCG_ERR_HIP;
  }
  if (!rc) rc = trsv_check_timeout(plan, T->ctx->stream);
  plan.release();
  return rc;
}

}  // extern "C"
