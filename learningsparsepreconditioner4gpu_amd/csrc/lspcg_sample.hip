// The GNN's input sample of a matrix that already lives on the device -- the GPU form of
// neural_cg/data.py:218-336 (make_data) as dataset.make_data restates it: edge_index from the CSR
// pattern, the matrix scale (normalize_matrix none / mean / frob / l1), edge_attr = the scaled
// values in fp32, the three diagonal vectors and x = [node_features | mask | scatter(edge_attr)].
//
// Numerics: every output value is computed in double with the host path's expression and rounded
// once, so it equals the host sample's for the same scale.  The mean / frob sums are compensated
// (DD) over chunks of kSumChunk values: a chunk's partial depends only on the chunk, and the
// partials are summed by one workgroup in a fixed shape, so the scale depends on neither the grid
// nor the device and no floating-point atomic is used.  The l1 row sums and the edge -> node
// reduce are plain sequential sums in stored / ascending edge order (scipy's and torch's orders).
//
// Streaming kernels: grid-stride, 16-B loads and stores where both ends are 16-B aligned (the flat
// value array, edge_attr and the two edge_index rows are contiguous), scalar tails.  In steady state
// one sample reads the values twice (sum, scaled copy) and writes edge_attr once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>

#include "lspcg_internal.hpp"

namespace lspcg {

// What a sample keeps on its matrix: the edges grouped by destination (pattern only, so
// lspcg_mat_set_values keeps it) and the chunk partials of the scale's sum.
struct SampleAux {
  int32_t* cptr = nullptr;  // [nb+1] column pointer
  int32_t* perm = nullptr;  // [nnzb] edges of column j at perm[cptr[j] .. cptr[j+1]), ascending
  double* part = nullptr;   // [2 * chunks | row-max partials]
  int64_t part_len = 0;
};

void mat_drop_sample_aux(lspcg_mat* A) {
  SampleAux* s = A->sample_aux;
  if (!s) return;
  (void)hipStreamSynchronize(A->ctx->stream);
  (void)hipFree(s->cptr);
  (void)hipFree(s->perm);
  (void)hipFree(s->part);
  delete s;
  A->sample_aux = nullptr;
}

namespace {

using d2 = double __attribute__((ext_vector_type(2)));
using f4 = float __attribute__((ext_vector_type(4)));
using l2 = long long __attribute__((ext_vector_type(2)));
using i4 = int __attribute__((ext_vector_type(4)));

constexpr int kSumChunk = 16 * kThreads;  // values per compensated partial (fixed: the sum's order)
constexpr double kDiagEps = 1e-7;         // data.py:318-320 / :264

int grid_for(int64_t items) {
  return int(std::max<int64_t>(1, std::min<int64_t>((items + kThreads - 1) / kThreads, kElemBlocksMax)));
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// four consecutive values as double: one 16-B load (fp32) or two (fp64); i + 4 <= n, vals + i 16-B aligned
__device__ __forceinline__ void load4(const float* __restrict__ vals, int64_t i, double (&v)[4]) {
  const f4 a = *reinterpret_cast<const f4*>(vals + i);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
}
__device__ __forceinline__ void load4(const double* __restrict__ vals, int64_t i, double (&v)[4]) {
  const d2 a = *reinterpret_cast<const d2*>(vals + i), b = *reinterpret_cast<const d2*>(vals + i + 2);
  v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
}

// ---------------------------------------------------------------------------
// edge_index
// ---------------------------------------------------------------------------
// Row 1 is colind widened (streamed, four entries per thread); row 0 comes from rowptr with no
// search: eight lanes walk one row's segment, so a wave covers eight consecutive rows, whose
// segments are adjacent in memory.
template <bool VEC>
__global__ void __launch_bounds__(kThreads) k_edge_index(int64_t nb, int64_t E, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ colind,
                                                         int64_t* __restrict__ ei) {
  const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, nt = int64_t(gridDim.x) * blockDim.x;
  int64_t* __restrict__ col = ei + E;
  if (VEC) {
    for (int64_t k = 4 * tid; k < E; k += 4 * nt) {
      if (k + 4 <= E) {
        const i4 c = *reinterpret_cast<const i4*>(colind + k);
        *reinterpret_cast<l2*>(col + k) = l2{c.x, c.y};
        *reinterpret_cast<l2*>(col + k + 2) = l2{c.z, c.w};
      } else {
        for (int64_t u = k; u < E; ++u) col[u] = colind[u];
      }
    }
  } else {
    for (int64_t k = tid; k < E; k += nt) col[k] = colind[k];
  }
  const int sub = int(tid & 7);
  for (int64_t i = tid >> 3; i < nb; i += nt >> 3) {
    const int32_t e = rowptr[i + 1];
    for (int32_t k = rowptr[i] + sub; k < e; k += 8) ei[k] = i;
  }
}

// ---------------------------------------------------------------------------
// scale
// ---------------------------------------------------------------------------
// part[2c], part[2c+1] <- the compensated sum of |v| (ABS) or v^2 over chunk c.  Thread t adds the
// chunk's values 4 (it * kThreads + t) + 0..3, it = 0..3, in that order, then the workgroup tree:
// the same for every grid.
template <typename T, bool ABS>
__global__ void __launch_bounds__(kThreads) k_sample_sum(int64_t ne, const T* __restrict__ vals,
                                                         double* __restrict__ part) {
  __shared__ DD lds[kThreads / 64];
  const int64_t nch = (ne + kSumChunk - 1) / kSumChunk;
  for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {
    DD a[1] = {dd_zero()};
#pragma unroll
    for (int it = 0; it < kSumChunk / (4 * kThreads); ++it) {
      const int64_t i = c * kSumChunk + 4 * (int64_t(it) * kThreads + threadIdx.x);
      double v[4];
      if (i + 4 <= ne) {
        load4(vals, i, v);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + u < ne ? double(vals[i + u]) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ABS) a[0] = dd_add(a[0], DD{__builtin_fabs(v[u]), 0.0});
        else dd_fma(a[0], v[u], v[u]);
      }
    }
    __syncthreads();  // thread 0 is done with the previous chunk's lds
    block_reduce_dd<1>(a, lds);
    if (threadIdx.x == 0) {
      part[2 * c + 0] = a[0].s;
      part[2 * c + 1] = a[0].c;
    }
  }
}

// one workgroup: thread t adds partials t, t + kThreads, ... in that order, then the workgroup tree
__global__ void __launch_bounds__(kThreads) k_sample_scale(int64_t nch, const double* __restrict__ part, int normalize,
                                                           double count, double* __restrict__ scale) {
  __shared__ DD lds[kThreads / 64];
  DD a[1] = {dd_zero()};
  for (int64_t c = threadIdx.x; c < nch; c += kThreads) a[0] = dd_add(a[0], DD{part[2 * c], part[2 * c + 1]});
  block_reduce_dd<1>(a, lds);
  if (threadIdx.x == 0) {
    const double s = dd_value(a[0]);
    scale[0] = normalize == LSPCG_NORM_MEAN ? 1.0 / (s / count) : 1.0 / sqrt(s);
  }
}

// l1: part[block] <- the largest row sum of |v| among the block's rows, each row a sequential sum
// in stored order starting from 0 (scipy's csr_matvec with a vector of ones).  max is exact, so the
// grid does not matter.
template <typename T>
__global__ void __launch_bounds__(kThreads) k_sample_rowmax(int64_t nb, const int32_t* __restrict__ rowptr,
                                                            const T* __restrict__ vals, double* __restrict__ part) {
  __shared__ double lds[kThreads / 64];
  double m = 0.0;  // an empty row sums to 0, and no sum is negative
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nb; i += int64_t(gridDim.x) * blockDim.x) {
    double s = 0.0;
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) s += __builtin_fabs(double(vals[k]));
    m = s > m ? s : m;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) m = lds[w] > m ? lds[w] : m;
    part[blockIdx.x] = m;
  }
}
__global__ void __launch_bounds__(64) k_sample_scale_l1(int np, const double* __restrict__ part,
                                                        double* __restrict__ scale) {
  double m = 0.0;
  for (int c = threadIdx.x; c < np; c += 64) m = part[c] > m ? part[c] : m;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  if (threadIdx.x == 0) scale[0] = 1.0 / (m + kDiagEps);
}
__global__ void k_sample_scale_one(double* __restrict__ scale) { scale[0] = 1.0; }

// ---------------------------------------------------------------------------
// value outputs
// ---------------------------------------------------------------------------
// edge_attr[k] = float(s * v[k]) over the flat value array, four values per thread and step
template <typename T, bool VEC>
__global__ void __launch_bounds__(kThreads) k_sample_edge_attr(int64_t ne, const T* __restrict__ vals,
                                                               const double* __restrict__ scale,
                                                               float* __restrict__ ea) {
  const double s = scale[0];
  const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, nt = int64_t(gridDim.x) * blockDim.x;
  if (VEC) {
    for (int64_t k = 4 * tid; k < ne; k += 4 * nt) {
      if (k + 4 <= ne) {
        double v[4];
        load4(vals, k, v);
        *reinterpret_cast<f4*>(ea + k) = f4{float(s * v[0]), float(s * v[1]), float(s * v[2]), float(s * v[3])};
      } else {
        for (int64_t u = k; u < ne; ++u) ea[u] = float(s * double(vals[u]));
      }
    }
  } else {
    for (int64_t k = tid; k < ne; k += nt) ea[k] = float(s * double(vals[k]));
  }
}

// diagonal / inv_diag / rsqrt_diag of block row i (binary search of column i, as lspcg_mat_diagonal)
template <typename T, int BS>
__global__ void __launch_bounds__(kThreads) k_sample_diag(int64_t nb, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ colind,
                                                          const T* __restrict__ vals, const double* __restrict__ scale,
                                                          float* __restrict__ diag, float* __restrict__ inv,
                                                          float* __restrict__ rsq) {
  const double s = scale[0];
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nb; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t end = rowptr[i + 1];
    int32_t lo = rowptr[i], hi = end;
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (colind[mid] < i) lo = mid + 1; else hi = mid;
    }
    const bool found = lo < end && colind[lo] == i;
#pragma unroll
    for (int a = 0; a < BS; ++a) {
      const double d = (found ? double(vals[int64_t(lo) * BS * BS + a * BS + a]) : 0.0) * s;
      diag[i * BS + a] = float(d);
      inv[i * BS + a] = float(1.0 / (d + kDiagEps));
      rsq[i * BS + a] = float(1.0 / sqrt(d + kDiagEps));
    }
  }
}

// ---------------------------------------------------------------------------
// x = [node_features | mask | reduce of edge_attr by destination]
// ---------------------------------------------------------------------------
struct XDesc {
  int64_t nb;
  int F, node_in, mask_cols, bs, BB, reduce;
  const float* nf;
  const void* mask;
  int mask_f64;
  const int32_t *cptr, *perm;
  const float* ea;
};

// One thread per element of x.  A reduce column c of node j folds edge_attr[e][c] over the edges
// into j in ascending edge order (torch's index_add_ / scatter_reduce_ order on the host): fp32
// adds from 0.0f, the mean's division by max(count, 1) in fp32, max / min as std::max / std::min
// fold them; no incoming edge gives 0.
__global__ void __launch_bounds__(kThreads) k_sample_x(XDesc d, float* __restrict__ x) {
  const int64_t total = d.nb * d.F;
  for (int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += int64_t(gridDim.x) * blockDim.x) {
    const int64_t j = idx / d.F;
    int col = int(idx - j * d.F);
    float out;
    if (col < d.node_in) {
      out = d.nf[j * d.node_in + col];
    } else if ((col -= d.node_in) < d.mask_cols) {
      const int64_t m = j * d.bs + col;
      out = !d.mask ? 1.0f : d.mask_f64 ? float(static_cast<const double*>(d.mask)[m])
                                        : static_cast<const float*>(d.mask)[m];
    } else {
      col -= d.mask_cols;
      const int32_t b = d.cptr[j], e = d.cptr[j + 1];
      const float* __restrict__ src = d.ea + col;
      out = 0.0f;
      if (d.reduce == LSPCG_REDUCE_SUM || d.reduce == LSPCG_REDUCE_MEAN) {
        for (int32_t k = b; k < e; ++k) out += src[int64_t(d.perm[k]) * d.BB];
        if (d.reduce == LSPCG_REDUCE_MEAN) out = out / float(e - b > 1 ? e - b : 1);
      } else if (e > b) {
        out = src[int64_t(d.perm[b]) * d.BB];
        for (int32_t k = b + 1; k < e; ++k) {
          const float v = src[int64_t(d.perm[k]) * d.BB];
          if (d.reduce == LSPCG_REDUCE_MAX) out = out < v ? v : out;
          else out = v < out ? v : out;
        }
      }
    }
    x[idx] = out;
  }
}

// ---------------------------------------------------------------------------
// destination grouping
// ---------------------------------------------------------------------------
__global__ void k_iota_f64(int64_t n, double* __restrict__ v) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += int64_t(gridDim.x) * blockDim.x)
    v[k] = double(k);
}
__global__ void k_f64_to_i32(int64_t n, const double* __restrict__ v, int32_t* __restrict__ out) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += int64_t(gridDim.x) * blockDim.x)
    out[k] = int32_t(v[k]);
}

SampleAux* aux_of(lspcg_mat* A) {
  if (!A->sample_aux) A->sample_aux = new SampleAux();
  return A->sample_aux;
}

// The column pointer and the stable edge permutation are the transpose of the block pattern with
// each entry's own index as its value: mat_transpose (the symmetric-pattern search, else the
// counting fill and per-row sort) returns them as the rowptr and the values of the result.
int build_col_groups(lspcg_mat* A) {
  SampleAux* s = aux_of(A);
  if (s->cptr) return LSPCG_OK;
  hipStream_t st = A->ctx->stream;
  using MatPtr = std::unique_ptr<lspcg_mat, int (*)(lspcg_mat*)>;
  lspcg_mat* raw = nullptr;
  if (int rc = mat_alloc(A->ctx, A->nb, A->nnzb, 1, LSPCG_F64, &raw)) return rc;
  MatPtr ids(raw, lspcg_mat_destroy);
  LSPCG_HIP(hipMemcpyAsync(ids->rowptr, A->rowptr, sizeof(int32_t) * (A->nb + 1), hipMemcpyDeviceToDevice, st));
  LSPCG_HIP(hipMemcpyAsync(ids->colind, A->colind, sizeof(int32_t) * A->nnzb, hipMemcpyDeviceToDevice, st));
  launch(k_iota_f64, dim3(grid_for(A->nnzb)), dim3(kThreads), st, A->nnzb, as<double>(ids->vals));
  LSPCG_HIP(hipGetLastError());
  raw = nullptr;
  if (int rc = mat_transpose(ids.get(), &raw, nullptr, nullptr)) return rc;
  MatPtr T(raw, lspcg_mat_destroy);
  int32_t* perm = nullptr;
  LSPCG_HIP(hipMalloc(&perm, sizeof(int32_t) * A->nnzb));
  launch(k_f64_to_i32, dim3(grid_for(A->nnzb)), dim3(kThreads), st, A->nnzb, as<double>(T->vals), perm);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {  // T is freed below
    (void)hipFree(perm);
    set_error("mat_sample: building the destination grouping failed");
    return LSPCG_ERR_HIP;
  }
  s->perm = perm;
  s->cptr = T->rowptr;  // taken over from the transpose
  T->rowptr = nullptr;
  return LSPCG_OK;
}

int reserve_part(lspcg_mat* A, int64_t len) {
  SampleAux* s = aux_of(A);
  if (s->part_len >= len) return LSPCG_OK;
  if (s->part) {
    LSPCG_HIP(hipStreamSynchronize(A->ctx->stream));
    (void)hipFree(s->part);
    s->part = nullptr;
    s->part_len = 0;
  }
  LSPCG_HIP(hipMalloc(&s->part, sizeof(double) * len));
  s->part_len = len;
  return LSPCG_OK;
}

}  // namespace
}  // namespace lspcg

using namespace lspcg;

extern "C" {

int lspcg_mat_edge_index(const lspcg_mat* A, int64_t* edge_index) {
  LSPCG_CHECK(A && edge_index, LSPCG_ERR_ARG, "mat_edge_index: NULL argument");
  if (A->nnzb == 0) return LSPCG_OK;
  LSPCG_HIP(hipSetDevice(A->ctx->device));
  hipStream_t st = A->ctx->stream;
  const dim3 g(grid_for(std::max((A->nnzb + 3) / 4, A->nb * 8))), b(kThreads);
  // 16-B stores need both rows aligned: row 1 starts E entries of 8 bytes after row 0
  by_flag(aligned16(edge_index) && A->nnzb % 2 == 0 && aligned16(A->colind), [&](auto vec) {
    launch(k_edge_index<decltype(vec)::value>, g, b, st, A->nb, A->nnzb, A->rowptr, A->colind, edge_index);
  });
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

int lspcg_mat_sample(lspcg_ctx* ctx, lspcg_mat* A, const lspcg_sample_desc* desc, const void* mask, int mask_dtype,
                     const float* node_features, float* x, float* edge_attr, float* diagonal, float* inv_diag,
                     float* rsqrt_diag, double* scale) {
  LSPCG_CHECK(ctx && A && desc && x && edge_attr && scale, LSPCG_ERR_ARG, "mat_sample: NULL argument");
  LSPCG_CHECK(ctx->device == A->ctx->device, LSPCG_ERR_ARG, "mat_sample: the matrix lives on another device");
  LSPCG_CHECK(A->nnzb > 0 && A->nb > 0, LSPCG_ERR_ARG, "mat_sample: empty matrix");
  LSPCG_CHECK(desc->normalize >= LSPCG_NORM_NONE && desc->normalize <= LSPCG_NORM_L1, LSPCG_ERR_ARG,
              "mat_sample: unknown normalize code");
  LSPCG_CHECK(desc->edge_reduce >= LSPCG_REDUCE_DISABLE && desc->edge_reduce <= LSPCG_REDUCE_MIN, LSPCG_ERR_ARG,
              "mat_sample: unknown edge_reduce code");
  LSPCG_CHECK(desc->mask_as_node_feature == 0 || desc->mask_as_node_feature == 1, LSPCG_ERR_ARG,
              "mat_sample: mask_as_node_feature must be 0 or 1");
  LSPCG_CHECK(desc->node_in >= 0 && (desc->node_in == 0 || node_features), LSPCG_ERR_ARG,
              "mat_sample: node_in > 0 needs node_features");
  LSPCG_CHECK(!mask || mask_dtype == LSPCG_F32 || mask_dtype == LSPCG_F64, LSPCG_ERR_ARG, "mat_sample: bad mask dtype");
  const bool diag = diagonal || inv_diag || rsqrt_diag;
  LSPCG_CHECK(!diag || (diagonal && inv_diag && rsqrt_diag), LSPCG_ERR_ARG,
              "mat_sample: diagonal, inv_diag and rsqrt_diag are given together or not at all");
  const int bs = A->block_size, BB = bs * bs;
  const int mask_cols = desc->mask_as_node_feature ? bs : 0;
  const int F = desc->node_in + mask_cols + (desc->edge_reduce != LSPCG_REDUCE_DISABLE ? BB : 0);
  LSPCG_CHECK(F > 0, LSPCG_ERR_ARG, "mat_sample: no node feature selected (F_in = 0)");
  LSPCG_CHECK(desc->normalize != LSPCG_NORM_L1 || bs == 1, LSPCG_ERR_UNSUPPORTED,
              "mat_sample: normalize l1 is defined for block size 1 only");
  LSPCG_CHECK(A->storage_dtype() == A->dtype, LSPCG_ERR_UNSUPPORTED, "mat_sample: compact value storage");
  LSPCG_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t ne = A->nnzb * BB;
  const int64_t nch = (ne + kSumChunk - 1) / kSumChunk;
  const int gsum = int(std::min<int64_t>(nch, kReduceBlocksMax)), grow = grid_for(A->nb);
  // first use only (allocates and synchronises): the edges grouped by destination for the reduce
  if (desc->edge_reduce != LSPCG_REDUCE_DISABLE)
    if (int rc = build_col_groups(A)) return rc;

  // ---- scale
  if (desc->normalize == LSPCG_NORM_NONE) {
    launch(k_sample_scale_one, dim3(1), dim3(1), st, scale);
  } else if (desc->normalize == LSPCG_NORM_L1) {
    if (int rc = reserve_part(A, std::max<int64_t>(2 * nch, grow))) return rc;
    double* part = A->sample_aux->part;
    by_dtype(A->dtype, [&](auto t) {
      using T = decltype(t);
      launch(k_sample_rowmax<T>, dim3(grow), dim3(kThreads), st, A->nb, A->rowptr, as<T>(A->vals), part);
    });
    launch(k_sample_scale_l1, dim3(1), dim3(64), st, grow, part, scale);
  } else {
    if (int rc = reserve_part(A, std::max<int64_t>(2 * nch, grow))) return rc;
    double* part = A->sample_aux->part;
    by_dtype(A->dtype, [&](auto t) {
      using T = decltype(t);
      by_flag(desc->normalize == LSPCG_NORM_MEAN, [&](auto ab) {
        launch(k_sample_sum<T, decltype(ab)::value>, dim3(gsum), dim3(kThreads), st, ne, as<T>(A->vals), part);
      });
    });
    launch(k_sample_scale, dim3(1), dim3(kThreads), st, nch, part, desc->normalize, double(ne), scale);
  }
  LSPCG_HIP(hipGetLastError());

  // ---- scaled values, diagonal vectors
  by_dtype(A->dtype, [&](auto t) {
    using T = decltype(t);
    by_flag(aligned16(A->vals) && aligned16(edge_attr), [&](auto vec) {
      launch(k_sample_edge_attr<T, decltype(vec)::value>, dim3(grid_for((ne + 3) / 4)), dim3(kThreads), st, ne,
             as<T>(A->vals), scale, edge_attr);
    });
  });
  if (diag)
    by_dtype_bs(A->dtype, bs, [&](auto t, auto b) {
      using T = decltype(t);
      launch(k_sample_diag<T, decltype(b)::value>, dim3(grow), dim3(kThreads), st, A->nb, A->rowptr, A->colind,
             as<T>(A->vals), scale, diagonal, inv_diag, rsqrt_diag);
    });
  LSPCG_HIP(hipGetLastError());

  // ---- x
  XDesc d{};
  d.nb = A->nb;
  d.F = F;
  d.node_in = desc->node_in;
  d.mask_cols = mask_cols;
  d.bs = bs;
  d.BB = BB;
  d.reduce = desc->edge_reduce;
  d.nf = node_features;
  d.mask = mask;
  d.mask_f64 = mask_dtype == LSPCG_F64;
  d.ea = edge_attr;
  if (desc->edge_reduce != LSPCG_REDUCE_DISABLE) {
    d.cptr = A->sample_aux->cptr;
    d.perm = A->sample_aux->perm;
  }
  launch(k_sample_x, dim3(grid_for(A->nb * F)), dim3(kThreads), st, d, x);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

}  // extern "C"
