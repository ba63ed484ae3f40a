// Context, sparse-matrix handles, transpose / diagonal / column scaling, SpMV and dot
// entry points of liblspcg_hip.so (C ABI: include/lspcg.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lspcg_internal.hpp"
#include "lspcg_sell.hpp"
#include "lspcg_spmv.hpp"

namespace lspcg {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

std::mutex& submit_mutex() {
  static std::mutex mu;
  return mu;
}

static size_t dtype_size(int dtype) { return dtype == LSPCG_F32 ? 4 : 8; }

int mat_alloc_entries(lspcg_mat* m, int64_t nnzb) {
  const int64_t ne = nnzb * m->block_size * m->block_size;
  const size_t es = dtype_size(m->dtype);
  hipStream_t st = m->ctx->stream;
  LSPCG_HIP(hipMalloc(&m->colind, sizeof(int32_t) * (nnzb + kEntryPad)));
  LSPCG_HIP(hipMalloc(&m->vals, es * (ne + kEntryPad)));
  LSPCG_HIP(hipMemsetAsync(m->colind + nnzb, 0, sizeof(int32_t) * kEntryPad, st));
  LSPCG_HIP(hipMemsetAsync(static_cast<char*>(m->vals) + es * ne, 0, es * kEntryPad, st));
  return LSPCG_OK;
}

// ---------------------------------------------------------------------------
// Transpose: counting sort by column with atomics, then a per-row insertion sort of
// the (original row, source position) pairs -> deterministic, sorted output.
// ---------------------------------------------------------------------------
__global__ void k_count_cols(int64_t nnzb, const int32_t* __restrict__ colind, int32_t* __restrict__ cnt) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < nnzb; k += int64_t(gridDim.x) * blockDim.x)
    atomicAdd(&cnt[colind[k]], 1);
}

__global__ void k_scatter_transpose(int64_t nb, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                    const int32_t* __restrict__ tptr, int32_t* __restrict__ fill,
                                    int32_t* __restrict__ trow, int64_t* __restrict__ tsrc) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nb; i += int64_t(gridDim.x) * blockDim.x) {
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int32_t c = colind[k];
      const int32_t pos = tptr[c] + atomicAdd(&fill[c], 1);
      trow[pos] = int32_t(i);
      tsrc[pos] = k;
    }
  }
}

template <typename T, int BS>
__global__ void k_sort_gather_transpose(int64_t nb, const int32_t* __restrict__ tptr, int32_t* __restrict__ trow,
                                        int64_t* __restrict__ tsrc, const T* __restrict__ vals, T* __restrict__ tvals) {
  for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < nb; j += int64_t(gridDim.x) * blockDim.x) {
    const int32_t b = tptr[j], e = tptr[j + 1];
    for (int32_t k = b + 1; k < e; ++k) {  // insertion sort by original row (unique keys)
      const int32_t r = trow[k];
      const int64_t s = tsrc[k];
      int32_t m = k - 1;
      while (m >= b && trow[m] > r) {
        trow[m + 1] = trow[m];
        tsrc[m + 1] = tsrc[m];
        --m;
      }
      trow[m + 1] = r;
      tsrc[m + 1] = s;
    }
    for (int32_t k = b; k < e; ++k) {
      const T* src = vals + tsrc[k] * BS * BS;
      T* dst = tvals + int64_t(k) * BS * BS;
#pragma unroll
      for (int p = 0; p < BS; ++p)
#pragma unroll
        for (int q = 0; q < BS; ++q) dst[p * BS + q] = src[q * BS + p];
    }
  }
}

// Symmetric-pattern transpose: Aᵀ has A's pattern, and the entry (r, j) of Aᵀ is A's entry
// (j, r), found by binary search in row j.  Deterministic, no atomics; flag <- 1 if some (j, r)
// is missing (pattern not symmetric: the general path runs instead).  A workgroup owns 256 rows
// and visits their entries entry-parallel, so the column reads and the output writes are
// coalesced; an entry's row comes from a search in the LDS copy of those rows' rowptr.
constexpr int kTrRows = 256;
template <typename T, int BS>
__global__ void __launch_bounds__(kTrRows) k_transpose_sym(int64_t nb, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ colind,
                                                          const T* __restrict__ vals, T* __restrict__ tvals,
                                                          int* __restrict__ flag) {
  __shared__ int32_t rp[kTrRows + 1];
  for (int64_t r0 = int64_t(blockIdx.x) * kTrRows; r0 < nb; r0 += int64_t(gridDim.x) * kTrRows) {
    const int cnt = int(nb - r0 < kTrRows ? nb - r0 : kTrRows);
    __syncthreads();
    for (int t = threadIdx.x; t <= cnt; t += blockDim.x) rp[t] = rowptr[r0 + t];
    __syncthreads();
    for (int32_t k = rp[0] + int32_t(threadIdx.x); k < rp[cnt]; k += int32_t(blockDim.x)) {
      int lo = 0, hi = cnt - 1;  // the row: largest t with rp[t] <= k (skips empty rows)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rp[mid] <= k) lo = mid;
        else hi = mid - 1;
      }
      const int32_t r = int32_t(r0 + lo);
      const int32_t j = colind[k];
      int32_t a = rowptr[j], e = rowptr[j + 1];
      const int32_t end = e;
      while (a < e) {
        const int32_t mid = (a + e) >> 1;
        if (colind[mid] < r) a = mid + 1;
        else e = mid;
      }
      if (a >= end || colind[a] != r) {
        atomicOr(flag, 1);
        continue;
      }
      const T* src = vals + int64_t(a) * BS * BS;
      T* dst = tvals + int64_t(k) * BS * BS;
#pragma unroll
      for (int p = 0; p < BS; ++p)
#pragma unroll
        for (int q = 0; q < BS; ++q) dst[p * BS + q] = src[q * BS + p];
    }
  }
}

template <typename T, int BS>
__global__ void k_diagonal(int64_t nb, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                           const T* __restrict__ vals, T* __restrict__ d) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nb; i += int64_t(gridDim.x) * blockDim.x) {
    int32_t lo = rowptr[i], hi = rowptr[i + 1];
    while (lo < hi) {  // binary search for column i (indices sorted)
      const int32_t mid = (lo + hi) >> 1;
      if (colind[mid] < i) lo = mid + 1; else hi = mid;
    }
    const bool found = lo < rowptr[i + 1] && colind[lo] == i;
#pragma unroll
    for (int a = 0; a < BS; ++a) d[i * BS + a] = found ? vals[int64_t(lo) * BS * BS + a * BS + a] : T(0);
  }
}

template <typename T, int BS>
__global__ void k_scale_columns(int64_t nnzb, const int32_t* __restrict__ colind, T* __restrict__ vals,
                                const T* __restrict__ d) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < nnzb * BS * BS;
       k += int64_t(gridDim.x) * blockDim.x) {
    const int64_t kb = k / (BS * BS);
    const int q = int(k % BS);
    vals[k] = vals[k] * d[int64_t(colind[kb]) * BS + q];
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) k_dot(int64_t n, const T* __restrict__ x, const T* __restrict__ y,
                                                  double* partials, unsigned* ticket, double* out) {
  DD d[1] = {dd_zero()};
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    dd_fma(d[0], double(x[i]), double(y[i]));
  grid_reduce_dd<1>(d, partials, ticket, [&](const double* v) { out[0] = v[0]; });
}

// Reads a large buffer (evicts the Infinity Cache with CLEAN lines; a memset would leave
// dirty lines whose write-back would be charged to the next kernel).
using u32x4 = unsigned __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(kThreads) k_flush_read(const u32x4* __restrict__ buf, int64_t n, unsigned* sink) {
  unsigned acc = 0;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const u32x4 v = buf[i];
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x9e3779b9u) sink[0] = acc;  // keeps the loads alive
}

static int grid_for(int64_t n) {
  int64_t g = (n + kThreads - 1) / kThreads;
  return int(std::max<int64_t>(1, std::min<int64_t>(g, kElemBlocksMax)));
}

// flag |= 2 when a[0..n) != b[0..n): streaming, coalesced, one atomic per wave that saw a difference
__global__ void __launch_bounds__(kThreads) k_pattern_neq(int64_t n, const int32_t* __restrict__ a,
                                                          const int32_t* __restrict__ b, int* __restrict__ flag) {
  bool bad = false;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    bad |= a[i] != b[i];
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 2);
}

void pattern_neq(const int32_t* rp_a, const int32_t* rp_b, int64_t nrp, const int32_t* ci_a, const int32_t* ci_b,
                 int64_t nci, int* flag, hipStream_t st) {
  if (nrp > 0) launch(k_pattern_neq, dim3(grid_for(nrp)), dim3(kThreads), st, nrp, rp_a, rp_b, flag);
  if (nci > 0) launch(k_pattern_neq, dim3(grid_for(nci)), dim3(kThreads), st, nci, ci_a, ci_b, flag);
}

// diagnostic gather: one 16-B load of an interleaved pair, a - alpha*b (the fused schedule's
// r - alpha q / p beta + z gathers with the two vectors interleaved)
struct GatherPairDiag {
  const double* xy;
  double alpha;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ double operator()(int64_t j) const {
    const f64x2 v = *(const __attribute__((address_space(1))) f64x2*)(xy + 2 * j);
    return v.x - alpha * v.y;
  }
};

// ---- diagnostic SpMV configurations (fp64, scalar CSR) for on-device A/B tuning
using SpmvLaunch = void (*)(const lspcg_mat*, const void*, void*, hipStream_t);
template <int TH, int GPT, bool NT, bool LANEC = false, bool XCD = false>
static void spmv_variant(const lspcg_mat* A, const void* x, void* y, hipStream_t st) {
  launch_spmv_cfg<double, double, 1, TH, GPT, NT, ProNone, GatherVec<double>, EpiStore<double>, LANEC, XCD>(
      A, GatherVec<double>{static_cast<const double*>(x)}, ProNone{},
                                          EpiStore<double>{static_cast<double*>(y)}, st);
}
static const SpmvLaunch kSpmvVariants[] = {
    spmv_variant<256, 4, false>, spmv_variant<256, 4, true>,  spmv_variant<256, 2, false>,
    spmv_variant<256, 2, true>,  spmv_variant<128, 4, false>, spmv_variant<128, 8, false>,
    spmv_variant<512, 2, false>, spmv_variant<512, 4, false>, spmv_variant<64, 8, false>,
    spmv_variant<128, 2, false>, spmv_variant<256, 8, false>, spmv_variant<128, 4, true>,
    spmv_variant<256, 4, false, true>, spmv_variant<256, 2, false, true>, spmv_variant<128, 4, false, true>,
    spmv_variant<512, 2, false, true>,  spmv_variant<256, 4, false, false, true>, spmv_variant<256, 4, false, true, true>,
    spmv_variant<128, 4, false, false, true>,
};
static constexpr int kNumSpmvVariants = int(sizeof(kSpmvVariants) / sizeof(kSpmvVariants[0]));

}  // namespace lspcg

using namespace lspcg;

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

const char* lspcg_last_error(void) { return g_last_error.c_str(); }
int lspcg_version(void) { return 10000; }

// hash of the sources, headers, flags and arch (_build.tree_hash(), passed by the build); the
// marker string lets the build check a binary's provenance without loading it
#ifndef LSPCG_BUILD_ID
#define LSPCG_BUILD_ID "unknown"
#endif
__attribute__((used)) static const char kBuildMarker[] = "LSPCG_BUILD_ID=" LSPCG_BUILD_ID;
const char* lspcg_build_id(void) { return kBuildMarker + 15; }

int lspcg_ctx_create(int device, void* stream, lspcg_ctx** out) {
  LSPCG_CHECK(out != nullptr, LSPCG_ERR_ARG, "ctx_create: out is NULL");
  int ndev = 0;
  LSPCG_HIP(hipGetDeviceCount(&ndev));
  LSPCG_CHECK(device >= 0 && device < ndev, LSPCG_ERR_ARG, "ctx_create: invalid device " + std::to_string(device));
  LSPCG_HIP(hipSetDevice(device));
  std::unique_ptr<lspcg_ctx> c(new lspcg_ctx());
  c->device = device;
  // NULL selects the device's default (null) stream, which PyTorch also uses by default,
  // so library work is ordered with the caller's tensor producers/consumers.
  c->stream = static_cast<hipStream_t>(stream);
  *out = c.release();
  return LSPCG_OK;
}

int lspcg_ctx_destroy(lspcg_ctx* ctx) {
  if (!ctx) return LSPCG_OK;
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return LSPCG_OK;
}

int lspcg_ctx_synchronize(lspcg_ctx* ctx) {
  LSPCG_CHECK(ctx, LSPCG_ERR_ARG, "ctx is NULL");
  LSPCG_HIP(hipStreamSynchronize(ctx->stream));
  return LSPCG_OK;
}

}  // extern "C"

namespace lspcg {
int mat_alloc(lspcg_ctx* ctx, int64_t nb, int64_t nnzb, int bs, int dtype, lspcg_mat** out) {
  LSPCG_CHECK(ctx && out, LSPCG_ERR_ARG, "mat: NULL ctx/out");
  LSPCG_CHECK(bs == 1 || bs == 3, LSPCG_ERR_UNSUPPORTED, "mat: block size must be 1 or 3");
  LSPCG_CHECK(dtype == LSPCG_F32 || dtype == LSPCG_F64, LSPCG_ERR_ARG, "mat: bad dtype");
  LSPCG_CHECK(nb >= 0 && nnzb >= 0 && nnzb < (int64_t(1) << 31) && nb < (int64_t(1) << 31) / bs, LSPCG_ERR_ARG,
              "mat: sizes out of int32 range");
  LSPCG_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<lspcg_mat> m(new lspcg_mat());
  m->ctx = ctx;
  m->block_size = bs;
  m->dtype = dtype;
  m->nb = nb;
  m->n = nb * bs;
  m->nnzb = nnzb;
  LSPCG_HIP(hipMalloc(&m->rowptr, sizeof(int32_t) * (nb + 1)));
  int rc = mat_alloc_entries(m.get(), nnzb);
  if (rc) return rc;
  *out = m.release();
  return LSPCG_OK;
}

int scan_to_rowptr(const int32_t* cnt, int64_t n, int32_t* rowptr, int64_t* total, hipStream_t st) {
  std::vector<int32_t> h(n + 1);
  if (n) LSPCG_HIP(hipMemcpyAsync(h.data(), cnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  int64_t acc = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t c = h[i];
    h[i] = int32_t(acc);
    acc += c;
  }
  LSPCG_CHECK(acc < (int64_t(1) << 31), LSPCG_ERR_ARG, "pattern too large for int32 indices");
  h[n] = int32_t(acc);
  LSPCG_HIP(hipMemcpyAsync(rowptr, h.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  *total = acc;
  return LSPCG_OK;
}

int flag_value(const int* dflag, hipStream_t st, int* out) {
  LSPCG_HIP(hipMemcpyAsync(out, dflag, sizeof(int), hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  return LSPCG_OK;
}
}  // namespace lspcg

extern "C" {

int lspcg_mat_create_bsr(lspcg_ctx* ctx, int64_t nb, int64_t nnzb, int bs, const int32_t* indptr,
                         const int32_t* indices, const void* vals, int dtype, lspcg_mat** out) {
  LSPCG_CHECK(indptr && (nnzb == 0 || (indices && vals)), LSPCG_ERR_ARG, "mat_create: NULL arrays");
  lspcg_mat* m = nullptr;
  int rc = mat_alloc(ctx, nb, nnzb, bs, dtype, &m);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(m->rowptr, indptr, sizeof(int32_t) * (nb + 1), hipMemcpyDefault, st);
  if (e == hipSuccess && nnzb)
    e = hipMemcpyAsync(m->colind, indices, sizeof(int32_t) * nnzb, hipMemcpyDefault, st);
  if (e == hipSuccess && nnzb)
    e = hipMemcpyAsync(m->vals, vals, dtype_size(dtype) * nnzb * bs * bs, hipMemcpyDefault, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // host sources may be released by the caller
  if (e != hipSuccess) {
    set_error(std::string("mat_create copy failed: ") + hipGetErrorString(e));
    lspcg_mat_destroy(m);
    return LSPCG_ERR_HIP;
  }
  *out = m;
  return LSPCG_OK;
}

int lspcg_mat_create_csr(lspcg_ctx* ctx, int64_t n, int64_t nnz, const int32_t* indptr, const int32_t* indices,
                         const void* vals, int dtype, lspcg_mat** out) {
  return lspcg_mat_create_bsr(ctx, n, nnz, 1, indptr, indices, vals, dtype, out);
}

static void drop_sell(lspcg_mat* A) {
  if (!A->sell) return;
  (void)hipStreamSynchronize(A->ctx->stream);
  A->sell->release();
  delete A->sell;
  A->sell = nullptr;
}

int lspcg_mat_destroy(lspcg_mat* A) {
  if (!A) return LSPCG_OK;
  (void)hipSetDevice(A->ctx->device);
  drop_sell(A);
  mat_drop_sample_aux(A);
  (void)hipFree(A->rowptr);
  (void)hipFree(A->colind);
  (void)hipFree(A->vals);
  delete A;
  return LSPCG_OK;
}

int lspcg_mat_info(const lspcg_mat* A, int64_t* n, int64_t* nnzb, int* bs, int* dtype) {
  LSPCG_CHECK(A, LSPCG_ERR_ARG, "mat_info: NULL");
  if (n) *n = A->n;
  if (nnzb) *nnzb = A->nnzb;
  if (bs) *bs = A->block_size;
  if (dtype) *dtype = A->dtype;
  return LSPCG_OK;
}

int lspcg_mat_copy_out(const lspcg_mat* A, int32_t* indptr, int32_t* indices, void* vals) {
  LSPCG_CHECK(A, LSPCG_ERR_ARG, "copy_out: NULL");
  hipStream_t st = A->ctx->stream;
  if (indptr) LSPCG_HIP(hipMemcpyAsync(indptr, A->rowptr, sizeof(int32_t) * (A->nb + 1), hipMemcpyDefault, st));
  if (indices && A->nnzb) LSPCG_HIP(hipMemcpyAsync(indices, A->colind, sizeof(int32_t) * A->nnzb, hipMemcpyDefault, st));
  if (vals && A->nnzb)
    LSPCG_HIP(hipMemcpyAsync(vals, A->vals, dtype_size(A->dtype) * A->nnzb * A->block_size * A->block_size,
                             hipMemcpyDefault, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  return LSPCG_OK;
}

int lspcg_mat_transpose(const lspcg_mat* A, lspcg_mat** out) {
  return lspcg::mat_transpose(A, out, nullptr, nullptr);
}

}  // extern "C"

bool lspcg::mat_reusable(const lspcg_mat* old, const lspcg_mat* like) {
  return old && like && old != like && old->ctx == like->ctx && old->nb == like->nb && old->nnzb == like->nnzb &&
         old->block_size == like->block_size && old->dtype == like->dtype &&
         old->storage_dtype() == like->storage_dtype() && !old->sell;
}

int lspcg::mat_transpose(const lspcg_mat* A, lspcg_mat** out, bool* same_pattern, lspcg_mat* reuse) {
  LSPCG_CHECK(A && out, LSPCG_ERR_ARG, "transpose: NULL");
  if (same_pattern) *same_pattern = false;
  lspcg_ctx* ctx = A->ctx;
  hipStream_t st = ctx->stream;
  lspcg_mat* Tm = nullptr;
  // a previous transpose of a matrix of the same shape is overwritten in place (a new ext_spai factor
  // on the same solver: no free / allocate of the entry arrays, and its addresses stay valid)
  if (A->storage_dtype() == A->dtype && mat_reusable(reuse, A)) Tm = reuse;
  else if (int rc = mat_alloc(ctx, A->nb, A->nnzb, A->block_size, A->dtype, &Tm)) return rc;
  // an early return destroys Tm unless it is the caller's `reuse`; handed out through release()
  std::unique_ptr<lspcg_mat, int (*)(lspcg_mat*)> guard(Tm == reuse ? nullptr : Tm, lspcg_mat_destroy);
  DevBuf B;
  // symmetric pattern (the ext_spai factor always has A's pattern): value permutation only
  int* flag = nullptr;
  if (int rc = B.get(&flag, 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  LSPCG_HIP(hipMemcpyAsync(Tm->rowptr, A->rowptr, sizeof(int32_t) * (A->nb + 1), hipMemcpyDeviceToDevice, st));
  if (A->nnzb) LSPCG_HIP(hipMemcpyAsync(Tm->colind, A->colind, sizeof(int32_t) * A->nnzb, hipMemcpyDeviceToDevice, st));
  if (A->nb) {
    const dim3 g(unsigned(std::min<int64_t>((A->nb + kTrRows - 1) / kTrRows, 65535))), b(kTrRows);
    by_dtype_bs(A->dtype, A->block_size, [&](auto t, auto bs) {
      using T = decltype(t);
      launch(k_transpose_sym<T, decltype(bs)::value>, g, b, st, A->nb, A->rowptr, A->colind, as<T>(A->vals),
             as<T>(Tm->vals), flag);
    });
    LSPCG_HIP(hipGetLastError());
  }
  int missing = 1;
  if (int rc = flag_value(flag, st, &missing)) return rc;
  B.release();
  if (!missing) {
    if (same_pattern) *same_pattern = true;
    guard.release();
    *out = Tm;
    return LSPCG_OK;
  }
  // general pattern: counts -> host exclusive scan (setup path, not the solve loop) -> fill
  int32_t* cnt = nullptr;
  int64_t* tsrc = nullptr;
  int64_t total = 0;
  if (int rc = B.get(&cnt, A->nb + 1) | B.get(&tsrc, A->nnzb)) return rc;
  LSPCG_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (A->nb + 1), st));
  launch(k_count_cols, dim3(grid_for(A->nnzb)), dim3(kThreads), st, A->nnzb, A->colind, cnt);
  if (int rc = scan_to_rowptr(cnt, A->nb, Tm->rowptr, &total, st)) return rc;
  LSPCG_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (A->nb + 1), st));
  const dim3 g(grid_for(A->nb)), b(kThreads);
  launch(k_scatter_transpose, g, b, st, A->nb, A->rowptr, A->colind, Tm->rowptr, cnt, Tm->colind, tsrc);
  by_dtype_bs(A->dtype, A->block_size, [&](auto t, auto bs) {
    using T = decltype(t);
    launch(k_sort_gather_transpose<T, decltype(bs)::value>, g, b, st, A->nb, Tm->rowptr, Tm->colind, tsrc,
           as<T>(A->vals), as<T>(Tm->vals));
  });
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipStreamSynchronize(st));
  guard.release();
  *out = Tm;
  return LSPCG_OK;
}

int lspcg::mat_refresh_spmv(lspcg_mat* A) {
  SellCopy* c = A->sell;
  if (!c) return LSPCG_OK;
  hipStream_t st = A->ctx->stream;
  const lspcg_mat* M = A;
  if (c->ro.perm) {  // the kept permutation: P A Pᵀ overwritten in place (the pattern reads its rowptr)
    lspcg_mat* out = nullptr;
    if (int rc = mat_permute(A, c->ro, &out, c->Ap)) return rc;
    if (out != c->Ap) {
      lspcg_mat_destroy(out);
      set_error("set_values: the permuted copy of the SpMV analysis does not fit the matrix");
      return LSPCG_ERR_ARG;
    }
    M = c->Ap;
  }
  const int vd = M->storage_dtype();
  return c->P.bs == 3 ? bsell_fill_values(c->P, M->vals, vd, vd, st, &c->vals)
                      : sell_fill_values(c->P, M->colind, M->vals, vd, vd, st, &c->vals);
}

// a pointer the device can read as it is (hipMalloc'd); anything else is staged by a copy
static bool is_device_pointer(const void* p) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // an unregistered host pointer: not an error of ours
    return false;
  }
  return at.type == hipMemoryTypeDevice;
}

extern "C" int lspcg_mat_set_values(lspcg_mat* A, const int32_t* indptr, const int32_t* indices, const void* vals,
                                    int dtype) {
  LSPCG_CHECK(A && (vals || A->nnzb == 0), LSPCG_ERR_ARG, "set_values: NULL argument");
  LSPCG_CHECK(dtype == A->dtype && A->storage_dtype() == A->dtype, LSPCG_ERR_ARG,
              "set_values: the values' dtype differs from the matrix dtype");
  LSPCG_HIP(hipSetDevice(A->ctx->device));
  hipStream_t st = A->ctx->stream;
  if (indptr || indices) {  // the pattern the values belong to: compared on the device before any write
    DevBuf B;
    int* flag = nullptr;
    if (int rc = B.get(&flag, 1)) return rc;
    LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    auto on_device = [&](const int32_t* p, int64_t n, const int32_t** out) -> int {
      *out = p;
      if (!p || n == 0 || is_device_pointer(p)) return LSPCG_OK;
      int32_t* d = nullptr;
      if (int rc = B.get(&d, n)) return rc;
      LSPCG_HIP(hipMemcpyAsync(d, p, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
      *out = d;
      return LSPCG_OK;
    };
    const int32_t *rp = nullptr, *ci = nullptr;
    if (int rc = on_device(indptr, A->nb + 1, &rp) | on_device(indices, A->nnzb, &ci)) return rc;
    pattern_neq(rp, A->rowptr, rp ? A->nb + 1 : 0, ci, A->colind, ci ? A->nnzb : 0, flag, st);
    LSPCG_HIP(hipGetLastError());
    int f = 0;
    if (int rc = flag_value(flag, st, &f)) return rc;
    LSPCG_CHECK(!f, LSPCG_ERR_FORMAT, "set_values: indptr / indices differ from the matrix's pattern (nothing written)");
  }
  const int64_t ne = A->nnzb * A->block_size * A->block_size;
  if (ne) LSPCG_HIP(hipMemcpyAsync(A->vals, vals, dtype_size(dtype) * ne, hipMemcpyDefault, st));
  if (int rc = mat_refresh_spmv(A)) return rc;
  LSPCG_HIP(hipStreamSynchronize(st));  // host sources may be released by the caller
  return LSPCG_OK;
}

extern "C" {

int lspcg_mat_diagonal(const lspcg_mat* A, void* d) {
  LSPCG_CHECK(A && d, LSPCG_ERR_ARG, "diagonal: NULL");
  hipStream_t st = A->ctx->stream;
  by_dtype_bs(A->dtype, A->block_size, [&](auto t, auto bs) {
    using T = decltype(t);
    launch(k_diagonal<T, decltype(bs)::value>, dim3(grid_for(A->nb)), dim3(kThreads), st, A->nb, A->rowptr, A->colind,
           as<T>(A->vals), as<T>(d));
  });
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

int lspcg_mat_prepare_spmv(lspcg_mat* A, int* kind) {
  LSPCG_CHECK(A, LSPCG_ERR_ARG, "prepare_spmv: NULL");
  LSPCG_HIP(hipSetDevice(A->ctx->device));
  drop_sell(A);
  if (kind) *kind = 0;
  if (A->n == 0 || A->nnzb == 0) return LSPCG_OK;
  hipStream_t st = A->ctx->stream;
  std::unique_ptr<SellCopy, void (*)(SellCopy*)> c(new SellCopy(), [](SellCopy* p) {
    p->release();
    delete p;
  });
  const bool blk = A->block_size == 3;  // BSR 3x3: the BSELL-64 block layout
  // a numbering far from banded: analyse P A Pᵀ (the solver's rule and permutation, rcm_reorder)
  int mode = -1;
  if (const char* e = std::getenv("LSPCG_REORDER")) mode = e[0] == 'a' ? -1 : std::atoi(e) ? 1 : 0;
  bool applied = false;
  if (int rc = rcm_reorder(A, mode, &c->ro, &applied)) return rc;
  const lspcg_mat* M = A;
  if (applied) {
    if (int rc = mat_permute(A, c->ro, &c->Ap)) return rc;
    M = c->Ap;
    const size_t vb = size_t(A->dtype == LSPCG_F32 ? 4 : 8) * size_t(std::max<int64_t>(A->n, 1));
    LSPCG_HIP(hipMalloc(&c->xs, vb));
  }
  int rc = blk ? bsell_build_pattern(M->nb, M->nnzb, M->rowptr, M->colind, sell_max_pad(), true, bsdia_allowed(), st,
                                     &c->P)
               : sell_build_pattern(M->n, M->nnzb, M->rowptr, M->colind, sell_max_pad(),
                                    kSellCol16 | kSellColDia | kSellColJag | kSellColXs, st,
                                    &c->P);
  if (rc == LSPCG_ERR_UNSUPPORTED) return LSPCG_OK;  // irregular rows: the CSR / BSR kernel stays
  if (rc) return rc;
  const int vd = M->storage_dtype();
  rc = blk ? bsell_fill_values(c->P, M->vals, vd, vd, st, &c->vals)
           : sell_fill_values(c->P, M->colind, M->vals, vd, vd, st, &c->vals);
  if (rc) {
    c->release();
    return rc;
  }
  LSPCG_HIP(hipStreamSynchronize(st));
  if (kind) *kind = c->P.col_bits;
  A->sell = c.release();
  return LSPCG_OK;
}

int lspcg_mat_spmv_reorder_info(const lspcg_mat* A, int* applied, double* mean_offset_before,
                                double* mean_offset_after) {
  LSPCG_CHECK(A && applied, LSPCG_ERR_ARG, "spmv_reorder_info: NULL argument");
  const SellCopy* c = A->sell;
  *applied = c && c->ro.perm ? 1 : 0;
  if (mean_offset_before) *mean_offset_before = c ? c->ro.off_before : 0.0;
  if (mean_offset_after) *mean_offset_after = c ? c->ro.off_after : 0.0;
  return LSPCG_OK;
}

int lspcg_mat_scale_columns(lspcg_mat* A, const void* d) {
  LSPCG_CHECK(A && d, LSPCG_ERR_ARG, "scale_columns: NULL");
  drop_sell(A);  // values change: the SELL copy would be stale
  hipStream_t st = A->ctx->stream;
  const int g = grid_for(A->nnzb * A->block_size * A->block_size);
  by_dtype_bs(A->dtype, A->block_size, [&](auto t, auto bs) {
    using T = decltype(t);
    launch(k_scale_columns<T, decltype(bs)::value>, dim3(g), dim3(kThreads), st, A->nnzb, A->colind, as<T>(A->vals),
           as<T>(d));
  });
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

int lspcg_spmv(lspcg_ctx* ctx, const lspcg_mat* A, const void* x, void* y) {
  LSPCG_CHECK(ctx && A && x && y, LSPCG_ERR_ARG, "spmv: NULL argument");
  if (const SellCopy* c = A->sell; c && c->ro.perm) {
    // reordered analysis: x -> P x, then (P A Pᵀ)(P x) with each row stored at its original place
    // (EpiStorePerm).  Two launches, so a kernel timer is left unconsumed (lspcg_spmv_timed then
    // times the whole call, x's gather included)
    KernelTimer* kt = kernel_timer();
    kernel_timer() = nullptr;
    const int64_t nb = A->nb;
    const int32_t* pm = c->ro.perm;
    int rc = vec_permute(A->dtype, nb, A->block_size, pm, x, c->xs, false, ctx->stream);
    if (!rc)
      rc = by_dtype_bs(A->dtype, A->block_size, [&](auto t, auto bs) {
        using T = decltype(t);
        return launch_sell<T, T>(c->P, c->vals, GatherVec<T>{as<T>(c->xs)}, ProNone{},
                                 EpiStorePerm<T, decltype(bs)::value>{as<T>(y), pm}, ctx->stream);
      });
    kernel_timer() = kt;
    if (rc) return rc;
    LSPCG_HIP(hipGetLastError());
    return LSPCG_OK;
  }
  const int rc = by_dtype(A->dtype, [&](auto t) -> int {
    using T = decltype(t);
    const EpiStore<T> epi{as<T>(y)};
    if (const SellCopy* c = A->sell)
      return launch_sell<T, T>(c->P, c->vals, GatherVec<T>{as<T>(x)}, ProNone{}, epi, ctx->stream);
    return launch_spmv_any<T>(A, as<T>(x), ProNone{}, epi, ctx->stream);
  });
  if (rc) return rc;
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

}  // extern "C"

__global__ void k_noop() {}

// the two timing events of a measurement, destroyed on every return
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int create() {
    LSPCG_HIP(hipEventCreate(&e0));
    LSPCG_HIP(hipEventCreate(&e1));
    return LSPCG_OK;
  }
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

template <class Launch>
static int spmv_timed_impl(lspcg_ctx* ctx, const lspcg_mat* A, int reps, int64_t flush_bytes, double* avg_ms,
                           Launch launch) {
  LSPCG_CHECK(ctx && reps > 0 && avg_ms && flush_bytes >= 0, LSPCG_ERR_ARG, "spmv_timed: bad argument");
  EventPair ev;
  if (int rc = ev.create()) return rc;
  const hipEvent_t e0 = ev.e0, e1 = ev.e1;
  DevBuf B;
  char* flush = nullptr;
  if (flush_bytes > 0) {
    if (int rc = B.get(&flush, size_t(flush_bytes) + 64)) return rc;
    LSPCG_HIP(hipMemsetAsync(flush, 1, size_t(flush_bytes) + 64, ctx->stream));
  }
  double total = 0.0;
  if (!flush) {
    if (int rc = launch()) return rc;  // untimed first launch
    LSPCG_HIP(hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < reps; ++i)
      if (int rc = launch()) return rc;
    LSPCG_HIP(hipEventRecord(e1, ctx->stream));
    LSPCG_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    LSPCG_HIP(hipEventElapsedTime(&ms, e0, e1));
    total = ms;
  } else {
    // cold: an Infinity-Cache-sized read before every launch.  The SpMV launch is timed by its own
    // start / end stamps (KernelTimer: hipExtLaunchKernelGGL events, the durations rocprofv3's
    // kernel trace reports); an event pair around the launch would add the in-stream kernel
    // boundaries.  Launch paths without the hook (lspcg_read_timed's read kernel) fall back to
    // R x (flush + launch) - R x (flush + an empty one-workgroup kernel), which has the same number
    // of boundaries on both sides.
    auto flush_k = [&]() {
      hipLaunchKernelGGL(k_flush_read, dim3(4096), dim3(kThreads), 0, ctx->stream,
                         reinterpret_cast<const u32x4*>(flush), flush_bytes / 16,
                         reinterpret_cast<unsigned*>(flush + flush_bytes));
    };
    flush_k();
    if (int rc = launch()) return rc;  // untimed first pair
    bool stamped = true;
    double sum = 0.0;
    for (int i = 0; i < reps && stamped; ++i) {
      flush_k();
      KernelTimer kt{e0, e1};
      kernel_timer() = &kt;
      const int rc = launch();
      stamped = kernel_timer() == nullptr;  // consumed by the launch
      kernel_timer() = nullptr;
      if (rc) return rc;
      if (stamped) {
        LSPCG_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        LSPCG_HIP(hipEventElapsedTime(&ms, e0, e1));
        sum += ms;
      }
    }
    float t_pair = 0.f, t_flush = 0.f;
    if (!stamped) {
      LSPCG_HIP(hipEventRecord(e0, ctx->stream));
      for (int i = 0; i < reps; ++i) {
        flush_k();
        if (int rc = launch()) return rc;
      }
      LSPCG_HIP(hipEventRecord(e1, ctx->stream));
      LSPCG_HIP(hipEventSynchronize(e1));
      LSPCG_HIP(hipEventElapsedTime(&t_pair, e0, e1));
      LSPCG_HIP(hipEventRecord(e0, ctx->stream));
      for (int i = 0; i < reps; ++i) {
        flush_k();
        hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, ctx->stream);
      }
      LSPCG_HIP(hipEventRecord(e1, ctx->stream));
      LSPCG_HIP(hipEventSynchronize(e1));
      LSPCG_HIP(hipEventElapsedTime(&t_flush, e0, e1));
    }
    LSPCG_HIP(hipGetLastError());
    total = stamped ? sum : double(t_pair) - double(t_flush);
  }
  *avg_ms = total / reps;
  return LSPCG_OK;
}

extern "C" {

int lspcg_spmv_timed(lspcg_ctx* ctx, const lspcg_mat* A, const void* x, void* y, int reps, int64_t flush_bytes,
                     double* avg_ms) {
  return spmv_timed_impl(ctx, A, reps, flush_bytes, avg_ms, [&]() -> int { return lspcg_spmv(ctx, A, x, y); });
}

int lspcg_spmv_variant_timed(lspcg_ctx* ctx, const lspcg_mat* A, int variant, const void* x, void* y, int reps,
                             int64_t flush_bytes, double* avg_ms) {
  if (variant < 0) return kNumSpmvVariants;
  LSPCG_CHECK(A && variant < kNumSpmvVariants && A->dtype == LSPCG_F64 && A->block_size == 1, LSPCG_ERR_ARG,
              "spmv_variant_timed: fp64 scalar CSR and a valid variant id required");
  return spmv_timed_impl(ctx, A, reps, flush_bytes, avg_ms, [&]() -> int {
    kSpmvVariants[variant](A, x, y, ctx->stream);
    LSPCG_HIP(hipGetLastError());
    return LSPCG_OK;
  });
}

int lspcg_spmv_sell_timed(lspcg_ctx* ctx, const lspcg_mat* A, int compact, const void* x, void* y, int reps,
                          int64_t flush_bytes, double* avg_ms) {
  LSPCG_CHECK(ctx && A && x && y && A->dtype == LSPCG_F64 && A->block_size == 1 && A->storage_dtype() == LSPCG_F64,
              LSPCG_ERR_ARG, "spmv_sell_timed: fp64 scalar CSR required");
  hipStream_t st = ctx->stream;
  SellPattern P;
  // any padding; compact bit 1: 16-bit offsets allowed, bit 3: SELL-DIA allowed, bit 4: SELL-64J allowed, bit 5: SELL-64X allowed
  const int cols = ((compact & 2) ? kSellCol16 : 0) | ((compact & 8) ? kSellColDia : 0) |
                   ((compact & 16) ? kSellColJag : 0) | ((compact & 32) && !(compact & 4) ? kSellColXs : 0);
  int rc = sell_build_pattern(A->n, A->nnzb, A->rowptr, A->colind, 1e30, cols, st, &P);
  if (rc) return rc;
  DevBuf B;
  void* v = nullptr;
  rc = sell_fill_values(P, A->colind, A->vals, LSPCG_F64, (compact & 1) ? LSPCG_F32 : LSPCG_F64, st, &v);
  B.p.push_back(v);  // the filled values are this function's from here
  double* x2 = nullptr;
  if (!rc && (compact & 4) && !(rc = B.get(&x2, 2 * A->n))) {  // experiment: 16-B gathers of interleaved (x, x) pairs
    (void)hipMemcpy2DAsync(x2, 16, x, 8, 8, A->n, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpy2DAsync(x2 + 1, 16, x, 8, 8, A->n, hipMemcpyDeviceToDevice, st);
  }
  if (!rc) {
    const GatherVec<double> gx{static_cast<const double*>(x)};
    const GatherPairDiag gp{x2, 0.0};
    const EpiStore<double> epi{static_cast<double*>(y)};
    rc = spmv_timed_impl(ctx, A, reps, flush_bytes, avg_ms, [&]() -> int {
      int lrc;
      if (compact & 4) {
        lrc = (compact & 1) ? launch_sell<double, float>(P, v, gp, ProNone{}, epi, st)
                            : launch_sell<double, double>(P, v, gp, ProNone{}, epi, st);
      } else {
        lrc = (compact & 1) ? launch_sell<double, float>(P, v, gx, ProNone{}, epi, st)
                            : launch_sell<double, double>(P, v, gx, ProNone{}, epi, st);
      }
      if (lrc) return lrc;
      LSPCG_HIP(hipGetLastError());
      return LSPCG_OK;
    });
  }
  (void)hipStreamSynchronize(st);
  B.release();
  P.release();
  return rc;
}

int lspcg_read_timed(lspcg_ctx* ctx, int64_t bytes, int reps, int64_t flush_bytes, double* avg_ms) {
  LSPCG_CHECK(ctx && bytes >= 16 && reps > 0 && avg_ms, LSPCG_ERR_ARG, "read_timed: bad argument");
  DevBuf B;
  char* buf = nullptr;
  if (int rc = B.get(&buf, size_t(bytes) + 64)) return rc;
  LSPCG_HIP(hipMemsetAsync(buf, 2, size_t(bytes) + 64, ctx->stream));
  int g = 0;
  LSPCG_HIP(hipDeviceGetAttribute(&g, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int rc = spmv_timed_impl(ctx, nullptr, reps, flush_bytes, avg_ms, [&]() -> int {
    hipLaunchKernelGGL(k_flush_read, dim3(unsigned(g * 8)), dim3(kThreads), 0, ctx->stream,
                       reinterpret_cast<const u32x4*>(buf), bytes / 16, reinterpret_cast<unsigned*>(buf + bytes));
    LSPCG_HIP(hipGetLastError());
    return LSPCG_OK;
  });
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

int lspcg_dot(lspcg_ctx* ctx, int64_t n, int dtype, const void* x, const void* y, double* out) {
  LSPCG_CHECK(ctx && out && n >= 0 && (n == 0 || (x && y)), LSPCG_ERR_ARG, "dot: bad argument");
  hipStream_t st = ctx->stream;
  const int g = grid_for(n);
  DevBuf B;
  double* buf = nullptr;  // [partials(2*g) | result]
  unsigned* ticket = nullptr;
  if (int rc = B.get(&buf, 2 * g + 1) | B.get(&ticket, kTicketWords)) return rc;
  LSPCG_HIP(hipMemsetAsync(ticket, 0, sizeof(unsigned) * kTicketWords, st));
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    launch(k_dot<T>, dim3(g), dim3(kThreads), st, n, as<T>(x), as<T>(y), buf, ticket, buf + 2 * g);
  });
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipMemcpyAsync(out, buf + 2 * g, sizeof(double), hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  return LSPCG_OK;
}

}  // extern "C"
