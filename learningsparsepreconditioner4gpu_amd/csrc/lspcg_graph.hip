// Block SpMV as message passing over an edge list -- the GPU form of the reference's
// GraphSpmv (neural_cg/nn/basic_layers.py:112-142) and AATPE (:228-261), the torch twin of
// the ext_spai apply used by training and by neural_pcg.py:649-654.
//
// PyG semantics restated (basic_layers.py:126-142):
//   GraphSpmv(use_transpose=False): flow "target_to_source": x_j = x[edge_index[1]], the
//     message A_e x_j is summed at edge_index[0]        ->  y = A x   (A_e = block (row, col))
//   GraphSpmv(use_transpose=True):  flow "source_to_target": x_j = x[edge_index[0]], the
//     message A_eᵀ x_j is summed at edge_index[1]       ->  y = Aᵀ x
//   forward(..., mask): out * mask after the sum.
//   AATPE.forward(x, ei, A, mask, diag): t = mask ⊙ Aᵀx ; t *= diag ; y = mask ⊙ (A t) + (εx)·diag
// Any edge order, duplicates summed (PyG's scatter-add); the list is sorted once per graph
// (lspcg_graph_create: two radix sorts of 64-bit (row, col) / (col, row) keys) so each output
// row is a deterministic sequential sum over its edges in (row, col) order -- PyG's atomic
// scatter order is arbitrary, so parity is the fp32 tolerance (1e-5), not bits.
//
// The training objective on the same handle (lspcg_graph_spai_loss, lspcg_graph_spmv_grad_vals):
// the reference's _shared_step (workspace.py:96-112, scaled_workspace.py:98-104) applies AATPE to
// the residual and feeds RelativeL2Loss_ANorm / L2Loss_ANorm (loss.py:168-203); here the chain
//   t = m ⊙ (Lᵀ r) [⊙ δ] ; d = m ⊙ (L t) + (ε r) [⊙ δ] ; q = m ⊙ (A d) ; loss(q, r)
// and its gradient with respect to the values of L run as five row-sum SpMVs (k_graph_spmv, no
// scatter), a chunked fixed-order reduction in double and one per-edge outer-product kernel:
//   gq = 2 (q − r) w_g ; gy = m ⊙ (Aᵀ (m ⊙ gq)) ; gtm = m ⊙ (Lᵀ gy) [⊙ δ]
//   dL_e = gy_I ⊗ t_J + r_I ⊗ gtm_J
// No floating-point atomics: two calls on the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "lspcg_internal.hpp"

struct lspcg_graph {
  lspcg_ctx* ctx = nullptr;
  int64_t N = 0, E = 0;
  int bs = 1;
  // row-major (by edge_index[0]) and column-major (by edge_index[1]) orders of the edges:
  // ptr[N+1] into perm[E] (edge ids) and other[E] (the edge's column, resp. row)
  int32_t *rp = nullptr, *rperm = nullptr, *rother = nullptr;
  int32_t *cp = nullptr, *cperm = nullptr, *cother = nullptr;
  // ---- gradient / loss state, allocated on first use (calls on one graph run on one stream at a time)
  int32_t *erow = nullptr, *ecol = nullptr;  // the two ends of every edge in the CALLER's edge order
  void* vec[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // t, d, q, gq, gy, gtm: N*bs of 8 bytes
  // the graphs of the last lspcg_graph_spai_loss call: node boundaries, and the fixed chunks of
  // kLossChunk scalar rows, split at graph boundaries, that the per-graph sums are reduced over
  std::vector<int64_t> hptr;
  int64_t nchunks = 0;
  int64_t* dptr = nullptr;      // [B+1] node boundaries
  int32_t* cbeg = nullptr;      // [nchunks] first scalar row of each chunk
  int32_t* cend = nullptr;      // [nchunks] one past its last
  int32_t* gchunk = nullptr;    // [B+1] chunks of graph g: gchunk[g] .. gchunk[g+1]
  double* cpart = nullptr;      // [nchunks][2] (‖q − r‖², ‖r‖²) of each chunk
  double* gw = nullptr;         // [B][2] per graph: its loss term, and w_g
  int64_t cap_graphs = -1, cap_chunks = -1;
};

namespace lspcg {

__global__ void k_graph_keys(int64_t E, int64_t N, const int64_t* __restrict__ ei, uint64_t* __restrict__ krow,
                             uint64_t* __restrict__ kcol, int32_t* __restrict__ ids, int* __restrict__ flag) {
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < E; e += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = ei[e], c = ei[E + e];
    if (r < 0 || r >= N || c < 0 || c >= N) {
      atomicOr(flag, 1);
      krow[e] = kcol[e] = 0;
    } else {
      krow[e] = uint64_t(r) * uint64_t(N) + uint64_t(c);
      kcol[e] = uint64_t(c) * uint64_t(N) + uint64_t(r);
    }
    ids[e] = int32_t(e);
  }
}

// ptr[i] = first sorted position whose key >= i*N; other[k] = key % N
__global__ void k_graph_ptr(int64_t E, int64_t N, const uint64_t* __restrict__ keys, int32_t* __restrict__ ptr,
                            int32_t* __restrict__ other) {
  const int64_t ts = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i <= N; i += ts) {
    const uint64_t key = uint64_t(i) * uint64_t(N);
    int64_t lo = 0, hi = E;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    ptr[i] = int32_t(lo);
  }
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < E; k += ts) other[k] = int32_t(keys[k] % uint64_t(N));
}

// One thread per scalar output row i = BS*I + a: the sum over the row's edges (sorted order),
// each edge's block row a (TRANS: block column a) against x at the other end.
//   PASS 0 (GraphSpmv / AATPE first half): y = s ; y *= mask ; y *= scale (AATPE's diag)
//   PASS 1 (AATPE second half): y = (s * mask) + (eps * x0) * scale
template <typename T, int BS, bool TRANS, int PASS>
__global__ void __launch_bounds__(256) k_graph_spmv(int64_t N, const int32_t* __restrict__ ptr,
                                                    const int32_t* __restrict__ perm, const int32_t* __restrict__ other,
                                                    const T* __restrict__ vals, const T* __restrict__ x,
                                                    const T* __restrict__ mask, const T* __restrict__ scale,
                                                    const T* __restrict__ x0, T eps, T* __restrict__ y) {
  const int64_t n = N * BS;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t I = i / BS;
    const int a = int(i - I * BS);
    T s = T(0);
    for (int32_t k = ptr[I]; k < ptr[I + 1]; ++k) {
      const int64_t e = perm[k];
      const int64_t J = other[k];
      const T* blk = vals + e * BS * BS;
      T m = T(0);  // the message component: (A_e x_J)[a] or (A_eᵀ x_J)[a]
#pragma unroll
      for (int c = 0; c < BS; ++c) m = m + (TRANS ? blk[c * BS + a] : blk[a * BS + c]) * x[J * BS + c];
      s = s + m;
    }
    if (mask) s = s * mask[i];
    if constexpr (PASS == 0) {
      if (scale) s = s * scale[i];
    } else {
      T ex = eps * x0[i];
      if (scale) ex = ex * scale[i];
      s = s + ex;
    }
    y[i] = s;
  }
}

constexpr int kLossChunk = 2048;  // scalar rows per reduction chunk: 256 threads x 8, independent of the grid

// (erow, ecol)[e] = the two ends of edge e, recovered from the two sorted orders (one-off per graph)
__global__ void k_graph_ends(int64_t E, const int32_t* __restrict__ rperm, const int32_t* __restrict__ rother,
                             const int32_t* __restrict__ cperm, const int32_t* __restrict__ cother,
                             int32_t* __restrict__ erow, int32_t* __restrict__ ecol) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < E; k += int64_t(gridDim.x) * blockDim.x) {
    ecol[rperm[k]] = rother[k];
    erow[cperm[k]] = cother[k];
  }
}

// One thread per edge, caller's edge order: out_e = u_I ⊗ v_J (+ u2_I ⊗ v2_J), rows by the I-end
// vector and columns by the J-end vector; the bs*bs values leave from registers.
template <typename T, int BS, bool TWO>
__global__ void __launch_bounds__(256) k_graph_outer(int64_t E, const int32_t* __restrict__ erow,
                                                     const int32_t* __restrict__ ecol, const T* __restrict__ u,
                                                     const T* __restrict__ v, const T* __restrict__ u2,
                                                     const T* __restrict__ v2, T* __restrict__ out) {
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < E; e += int64_t(gridDim.x) * blockDim.x) {
    const int64_t I = erow[e], J = ecol[e];
    T a[BS], b[BS], a2[BS], b2[BS];
#pragma unroll
    for (int k = 0; k < BS; ++k) {
      a[k] = u[I * BS + k];
      b[k] = v[J * BS + k];
      if constexpr (TWO) {
        a2[k] = u2[I * BS + k];
        b2[k] = v2[J * BS + k];
      }
    }
    T o[BS * BS];
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        T w = a[i] * b[j];
        if constexpr (TWO) w = w + a2[i] * b2[j];
        o[i * BS + j] = w;
      }
    T* dst = out + e * (BS * BS);
#pragma unroll
    for (int k = 0; k < BS * BS; ++k) dst[k] = o[k];
  }
}

// fixed-order sum of 2 doubles over a 256-thread workgroup; the result is valid in thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds /* 8 */) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    a = a + __shfl_xor(a, m, 64);
    b = b + __shfl_xor(b, m, 64);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();  // lds may still be read by the previous round
  if (lane == 0) {
    lds[wid * 2 + 0] = a;
    lds[wid * 2 + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = lds[0];
    b = lds[1];
    for (int w = 1; w < int(blockDim.x >> 6); ++w) {
      a = a + lds[w * 2 + 0];
      b = b + lds[w * 2 + 1];
    }
  }
}

// cpart[c] = (Σ (q − r)², Σ r²) over chunk c, in double; one workgroup per chunk, every thread
// a fixed strided subset of the chunk -> the sum's order does not depend on the grid
template <typename T>
__global__ void __launch_bounds__(256) k_loss_chunks(int64_t nchunks, const int32_t* __restrict__ cbeg,
                                                     const int32_t* __restrict__ cend, const T* __restrict__ q,
                                                     const T* __restrict__ r, double* __restrict__ cpart) {
  __shared__ double lds[8];
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int32_t i1 = cend[c];
    double se = 0.0, sr = 0.0;
    for (int64_t i = int64_t(cbeg[c]) + threadIdx.x; i < i1; i += 256) {
      const double rr = double(r[i]);
      const double e = double(q[i]) - rr;
      se = se + e * e;
      sr = sr + rr * rr;
    }
    block_sum2(se, sr, lds);
    if (threadIdx.x == 0) {
      cpart[c * 2 + 0] = se;
      cpart[c * 2 + 1] = sr;
    }
  }
}

// One workgroup per graph: its chunk partials summed in a fixed strided order.
// kind 0 (RelativeL2Loss_ANorm, sqr_out): term = ‖q_g − r_g‖² / (‖r_g‖² + eps) / B, w_g = 1 / (B (‖r_g‖² + eps))
// kind 1 (L2Loss_ANorm):                  term = ‖q_g − r_g‖² / n,                   w_g = 1 / n
__global__ void __launch_bounds__(256) k_loss_graphs(int64_t B, const int32_t* __restrict__ gchunk,
                                                     const double* __restrict__ cpart, int kind, double eps, double n,
                                                     double* __restrict__ gw) {
  __shared__ double lds[8];
  for (int64_t g = blockIdx.x; g < B; g += gridDim.x) {
    double se = 0.0, sr = 0.0;
    for (int32_t c = gchunk[g] + int32_t(threadIdx.x); c < gchunk[g + 1]; c += 256) {
      se = se + cpart[int64_t(c) * 2 + 0];
      sr = sr + cpart[int64_t(c) * 2 + 1];
    }
    block_sum2(se, sr, lds);
    if (threadIdx.x == 0) {
      const double w = kind == 0 ? 1.0 / (double(B) * (sr + eps)) : 1.0 / n;
      gw[g * 2 + 0] = se * w;
      gw[g * 2 + 1] = w;
    }
  }
}

// loss = Σ_g term_g, one workgroup, fixed order
__global__ void __launch_bounds__(256) k_loss_total(int64_t B, const double* __restrict__ gw, double* __restrict__ loss) {
  __shared__ double lds[8];
  double s = 0.0, z = 0.0;
  for (int64_t g = threadIdx.x; g < B; g += 256) s = s + gw[g * 2];
  block_sum2(s, z, lds);
  if (threadIdx.x == 0) *loss = s;
}

// gq = m ⊙ (2 (q − r) w_g), the graph of a row found by a search in ptr
template <typename T, int BS>
__global__ void __launch_bounds__(256) k_loss_gq(int64_t N, int64_t B, const int64_t* __restrict__ ptr,
                                                 const double* __restrict__ gw, const T* __restrict__ q,
                                                 const T* __restrict__ r, const T* __restrict__ mask,
                                                 T* __restrict__ gq) {
  const int64_t n = N * BS;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t I = i / BS;
    int64_t lo = 0, hi = B;  // the last g with ptr[g] <= I (empty graphs share a boundary: the search skips them)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (ptr[mid] <= I) lo = mid;
      else hi = mid;
    }
    double v = 2.0 * (double(q[i]) - double(r[i])) * gw[lo * 2 + 1];
    if (mask) v = v * double(mask[i]);
    gq[i] = T(v);
  }
}

static int grid_of(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return int(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

template <typename T, int BS>
static void launch(const lspcg_graph* g, bool trans, int pass, const T* vals, const T* x, const T* mask, const T* scale,
                   const T* x0, T eps, T* y) {
  hipStream_t st = g->ctx->stream;
  const dim3 grid(grid_of(g->N * BS)), blk(256);
  const int32_t* ptr = trans ? g->cp : g->rp;
  const int32_t* perm = trans ? g->cperm : g->rperm;
  const int32_t* oth = trans ? g->cother : g->rother;
  if (trans) {
    if (pass == 0)
      hipLaunchKernelGGL((k_graph_spmv<T, BS, true, 0>), grid, blk, 0, st, g->N, ptr, perm, oth, vals, x, mask, scale, x0, eps, y);
    else
      hipLaunchKernelGGL((k_graph_spmv<T, BS, true, 1>), grid, blk, 0, st, g->N, ptr, perm, oth, vals, x, mask, scale, x0, eps, y);
  } else {
    if (pass == 0)
      hipLaunchKernelGGL((k_graph_spmv<T, BS, false, 0>), grid, blk, 0, st, g->N, ptr, perm, oth, vals, x, mask, scale, x0, eps, y);
    else
      hipLaunchKernelGGL((k_graph_spmv<T, BS, false, 1>), grid, blk, 0, st, g->N, ptr, perm, oth, vals, x, mask, scale, x0, eps, y);
  }
}

template <typename T>
static int dispatch(const lspcg_graph* g, bool trans, int pass, const void* vals, const void* x, const void* mask,
                    const void* scale, const void* x0, double eps, void* y) {
  auto v = static_cast<const T*>(vals);
  auto xx = static_cast<const T*>(x);
  auto m = static_cast<const T*>(mask);
  auto sc = static_cast<const T*>(scale);
  auto z = static_cast<const T*>(x0);
  auto yy = static_cast<T*>(y);
  if (g->bs == 1) launch<T, 1>(g, trans, pass, v, xx, m, sc, z, T(eps), yy);
  else launch<T, 3>(g, trans, pass, v, xx, m, sc, z, T(eps), yy);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

static int run(const lspcg_graph* g, int dtype, bool trans, int pass, const void* vals, const void* x,
               const void* mask, const void* scale, const void* x0, double eps, void* y) {
  if (g->N == 0) return LSPCG_OK;
  return dtype == LSPCG_F32 ? dispatch<float>(g, trans, pass, vals, x, mask, scale, x0, eps, y)
                            : dispatch<double>(g, trans, pass, vals, x, mask, scale, x0, eps, y);
}

// ---- gradient / loss host side --------------------------------------------------------------

// the ends of every edge in the caller's order, built from the sorted orders on first use
static int ensure_ends(lspcg_graph* g) {
  if (g->erow || g->E == 0) return LSPCG_OK;
  const size_t eb = sizeof(int32_t) * size_t(g->E);
  if (!g->ecol) LSPCG_HIP(hipMalloc(&g->ecol, eb));
  int32_t* er = nullptr;
  LSPCG_HIP(hipMalloc(&er, eb));
  hipLaunchKernelGGL(k_graph_ends, dim3(grid_of(g->E)), dim3(256), 0, g->ctx->stream, g->E, g->rperm, g->rother,
                     g->cperm, g->cother, er, g->ecol);
  g->erow = er;  // set last: a call that failed above starts over
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

template <typename T>
static int outer(const lspcg_graph* g, const void* u, const void* v, const void* u2, const void* v2, void* out) {
  if (g->E == 0) return LSPCG_OK;
  hipStream_t st = g->ctx->stream;
  const dim3 grid(grid_of(g->E)), blk(256);
  auto a = static_cast<const T*>(u), b = static_cast<const T*>(v);
  auto a2 = static_cast<const T*>(u2), b2 = static_cast<const T*>(v2);
  auto o = static_cast<T*>(out);
  if (g->bs == 1) {
    if (u2) hipLaunchKernelGGL((k_graph_outer<T, 1, true>), grid, blk, 0, st, g->E, g->erow, g->ecol, a, b, a2, b2, o);
    else hipLaunchKernelGGL((k_graph_outer<T, 1, false>), grid, blk, 0, st, g->E, g->erow, g->ecol, a, b, a2, b2, o);
  } else {
    if (u2) hipLaunchKernelGGL((k_graph_outer<T, 3, true>), grid, blk, 0, st, g->E, g->erow, g->ecol, a, b, a2, b2, o);
    else hipLaunchKernelGGL((k_graph_outer<T, 3, false>), grid, blk, 0, st, g->E, g->erow, g->ecol, a, b, a2, b2, o);
  }
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

static int ensure_vecs(lspcg_graph* g) {
  if (g->vec[0]) return LSPCG_OK;
  const size_t nb = sizeof(double) * size_t(std::max<int64_t>(g->N * g->bs, 1));  // either dtype fits
  for (void*& p : g->vec) LSPCG_HIP(hipMalloc(&p, nb));
  return LSPCG_OK;
}

// Node boundaries of the B graphs (host or device pointer): validated, cut into the reduction
// chunks and uploaded; a call with the boundaries of the previous one reuses what is there.
static int set_graphs(lspcg_graph* g, const int64_t* ptr, int64_t B) {
  std::vector<int64_t> h(size_t(B) + 1);
  hipPointerAttribute_t attr;
  const bool on_device = hipPointerGetAttributes(&attr, ptr) == hipSuccess && attr.type == hipMemoryTypeDevice;
  (void)hipGetLastError();  // a plain host pointer is no error here
  if (on_device) LSPCG_HIP(hipMemcpy(h.data(), ptr, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost));
  else std::copy(ptr, ptr + B + 1, h.begin());
  bool ok = h[0] == 0 && h[size_t(B)] == g->N;
  for (int64_t k = 0; ok && k < B; ++k) ok = h[size_t(k)] <= h[size_t(k) + 1];
  LSPCG_CHECK(ok, LSPCG_ERR_FORMAT, "graph_spai_loss: ptr must be non-decreasing from 0 to N");
  if (g->cap_graphs >= 0 && h == g->hptr) return LSPCG_OK;
  std::vector<int32_t> cb, ce, gc(size_t(B) + 1);
  for (int64_t k = 0; k < B; ++k) {
    gc[size_t(k)] = int32_t(cb.size());
    const int64_t i1 = h[size_t(k) + 1] * g->bs;
    for (int64_t i = h[size_t(k)] * g->bs; i < i1; i += kLossChunk) {
      cb.push_back(int32_t(i));
      ce.push_back(int32_t(std::min<int64_t>(i + kLossChunk, i1)));
    }
  }
  gc[size_t(B)] = int32_t(cb.size());
  const int64_t nc = int64_t(cb.size());
  hipStream_t st = g->ctx->stream;
  LSPCG_HIP(hipStreamSynchronize(st));  // the arrays below may still be read by the previous call
  if (B > g->cap_graphs) {
    (void)hipFree(g->dptr);
    (void)hipFree(g->gchunk);
    (void)hipFree(g->gw);
    g->dptr = nullptr, g->gchunk = nullptr, g->gw = nullptr, g->cap_graphs = -1;
    LSPCG_HIP(hipMalloc(&g->dptr, sizeof(int64_t) * (B + 1)));
    LSPCG_HIP(hipMalloc(&g->gchunk, sizeof(int32_t) * (B + 1)));
    LSPCG_HIP(hipMalloc(&g->gw, sizeof(double) * 2 * std::max<int64_t>(B, 1)));
    g->cap_graphs = B;
  }
  if (nc > g->cap_chunks) {
    (void)hipFree(g->cbeg);
    (void)hipFree(g->cend);
    (void)hipFree(g->cpart);
    g->cbeg = nullptr, g->cend = nullptr, g->cpart = nullptr, g->cap_chunks = -1;
    const size_t m = size_t(std::max<int64_t>(nc, 1));
    LSPCG_HIP(hipMalloc(&g->cbeg, sizeof(int32_t) * m));
    LSPCG_HIP(hipMalloc(&g->cend, sizeof(int32_t) * m));
    LSPCG_HIP(hipMalloc(&g->cpart, sizeof(double) * 2 * m));
    g->cap_chunks = nc;
  }
  g->hptr.clear();  // not valid until every copy below is done
  LSPCG_HIP(hipMemcpyAsync(g->dptr, h.data(), sizeof(int64_t) * (B + 1), hipMemcpyHostToDevice, st));
  LSPCG_HIP(hipMemcpyAsync(g->gchunk, gc.data(), sizeof(int32_t) * (B + 1), hipMemcpyHostToDevice, st));
  if (nc) {
    LSPCG_HIP(hipMemcpyAsync(g->cbeg, cb.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice, st));
    LSPCG_HIP(hipMemcpyAsync(g->cend, ce.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice, st));
  }
  LSPCG_HIP(hipStreamSynchronize(st));  // the host vectors go out of scope
  g->hptr = std::move(h);
  g->nchunks = nc;
  return LSPCG_OK;
}

template <typename T>
static int loss_chain(lspcg_graph* g, int dtype, const void* Lv, const void* Av, double epsilon, const void* r,
                      const void* mask, const void* diag, int64_t B, int kind, double loss_eps, double* loss_out,
                      void* dL) {
  hipStream_t st = g->ctx->stream;
  T *t = static_cast<T*>(g->vec[0]), *d = static_cast<T*>(g->vec[1]), *q = static_cast<T*>(g->vec[2]);
  T *gq = static_cast<T*>(g->vec[3]), *gy = static_cast<T*>(g->vec[4]), *gtm = static_cast<T*>(g->vec[5]);
  auto rr = static_cast<const T*>(r);
  auto m = static_cast<const T*>(mask);
  if (int rc = run(g, dtype, true, 0, Lv, r, mask, diag, nullptr, 0.0, t)) return rc;
  if (int rc = run(g, dtype, false, 1, Lv, t, mask, diag, r, epsilon, d)) return rc;
  if (int rc = run(g, dtype, false, 0, Av, d, mask, nullptr, nullptr, 0.0, q)) return rc;
  const int cgrid = int(std::min<int64_t>(std::max<int64_t>(g->nchunks, 1), 65536));
  hipLaunchKernelGGL((k_loss_chunks<T>), dim3(cgrid), dim3(256), 0, st, g->nchunks, g->cbeg, g->cend, q, rr, g->cpart);
  const int ggrid = int(std::min<int64_t>(B, 8192));
  hipLaunchKernelGGL(k_loss_graphs, dim3(ggrid), dim3(256), 0, st, B, g->gchunk, g->cpart, kind, loss_eps,
                     double(g->N * g->bs), g->gw);
  hipLaunchKernelGGL(k_loss_total, dim3(1), dim3(256), 0, st, B, g->gw, loss_out);
  LSPCG_HIP(hipGetLastError());
  if (!dL || g->E == 0) return LSPCG_OK;
  const dim3 grid(grid_of(g->N * g->bs)), blk(256);
  if (g->bs == 1) hipLaunchKernelGGL((k_loss_gq<T, 1>), grid, blk, 0, st, g->N, B, g->dptr, g->gw, q, rr, m, gq);
  else hipLaunchKernelGGL((k_loss_gq<T, 3>), grid, blk, 0, st, g->N, B, g->dptr, g->gw, q, rr, m, gq);
  LSPCG_HIP(hipGetLastError());
  if (int rc = run(g, dtype, true, 0, Av, gq, mask, nullptr, nullptr, 0.0, gy)) return rc;
  if (int rc = run(g, dtype, true, 0, Lv, gy, mask, diag, nullptr, 0.0, gtm)) return rc;
  return outer<T>(g, gy, t, r, gtm, dL);
}

}  // namespace lspcg

using namespace lspcg;

extern "C" {

int lspcg_graph_create(lspcg_ctx* ctx, int64_t N, int64_t E, int bs, const int64_t* edge_index, lspcg_graph** out) {
  LSPCG_CHECK(ctx && out && (E == 0 || edge_index), LSPCG_ERR_ARG, "graph_create: NULL argument");
  LSPCG_CHECK(bs == 1 || bs == 3, LSPCG_ERR_UNSUPPORTED, "graph_create: block size must be 1 or 3");
  LSPCG_CHECK(N >= 0 && E >= 0 && E < (int64_t(1) << 31) && N * bs < (int64_t(1) << 31), LSPCG_ERR_ARG,
              "graph_create: sizes out of int32 range");
  LSPCG_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::unique_ptr<lspcg_graph> g(new lspcg_graph());
  g->ctx = ctx;
  g->N = N;
  g->E = E;
  g->bs = bs;
  const size_t eb = sizeof(int32_t) * size_t(std::max<int64_t>(E, 1));
  for (int32_t** p : {&g->rp, &g->cp}) LSPCG_HIP(hipMalloc(p, sizeof(int32_t) * (N + 1)));
  for (int32_t** p : {&g->rperm, &g->rother, &g->cperm, &g->cother}) LSPCG_HIP(hipMalloc(p, eb));
  if (E == 0) {
    LSPCG_HIP(hipMemsetAsync(g->rp, 0, sizeof(int32_t) * (N + 1), st));
    LSPCG_HIP(hipMemsetAsync(g->cp, 0, sizeof(int32_t) * (N + 1), st));
    LSPCG_HIP(hipStreamSynchronize(st));
    *out = g.release();
    return LSPCG_OK;
  }
  uint64_t *kr = nullptr, *kc = nullptr, *ks = nullptr;
  int32_t* ids = nullptr;
  int* flag = nullptr;
  void* tmp = nullptr;
  DevBuf B;
  if (int rc = B.get(&kr, E) | B.get(&kc, E) | B.get(&ks, E) | B.get(&ids, E) | B.get(&flag, 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_graph_keys, dim3(grid_of(E)), dim3(256), 0, st, E, N, edge_index, kr, kc, ids, flag);
  int bits = 1;
  while (bits < 64 && (uint64_t(1) << bits) < uint64_t(N) * uint64_t(N)) ++bits;
  size_t tb = 0;
  LSPCG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, kr, ks, ids, g->rperm, int(E), 0, bits, st));
  if (int rc = B.get(&tmp, tb)) return rc;
  LSPCG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, kr, ks, ids, g->rperm, int(E), 0, bits, st));
  hipLaunchKernelGGL(k_graph_ptr, dim3(grid_of(std::max<int64_t>(N + 1, E))), dim3(256), 0, st, E, N, ks, g->rp,
                     g->rother);
  LSPCG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, kc, ks, ids, g->cperm, int(E), 0, bits, st));
  hipLaunchKernelGGL(k_graph_ptr, dim3(grid_of(std::max<int64_t>(N + 1, E))), dim3(256), 0, st, E, N, ks, g->cp,
                     g->cother);
  int h = 0;
  if (int rc = flag_value(flag, st, &h)) return rc;
  if (h) {
    lspcg_graph_destroy(g.release());
    set_error("graph_create: edge_index out of range [0, N)");
    return LSPCG_ERR_FORMAT;
  }
  *out = g.release();
  return LSPCG_OK;
}

int lspcg_graph_destroy(lspcg_graph* g) {
  if (!g) return LSPCG_OK;
  (void)hipSetDevice(g->ctx->device);
  for (int32_t* p : {g->rp, g->rperm, g->rother, g->cp, g->cperm, g->cother}) (void)hipFree(p);
  for (void* p : {(void*)g->erow, (void*)g->ecol, (void*)g->dptr, (void*)g->cbeg, (void*)g->cend, (void*)g->gchunk,
                  (void*)g->cpart, (void*)g->gw})
    (void)hipFree(p);
  for (void* p : g->vec) (void)hipFree(p);
  delete g;
  return LSPCG_OK;
}

int lspcg_graph_spmv(lspcg_graph* g, const void* vals, int dtype, int transpose, const void* x, const void* mask,
                     void* y) {
  LSPCG_CHECK(g && (g->E == 0 || vals) && x && y, LSPCG_ERR_ARG, "graph_spmv: NULL argument");
  LSPCG_CHECK(dtype == LSPCG_F32 || dtype == LSPCG_F64, LSPCG_ERR_ARG, "graph_spmv: bad dtype");
  LSPCG_CHECK(x != y, LSPCG_ERR_ARG, "graph_spmv: x and y must not alias");
  LSPCG_HIP(hipSetDevice(g->ctx->device));
  return run(g, dtype, transpose != 0, 0, vals, x, mask, nullptr, nullptr, 0.0, y);
}

int lspcg_graph_aatpe(lspcg_graph* g, const void* vals, int dtype, double epsilon, const void* x, const void* mask,
                      const void* diag, void* t, void* y) {
  LSPCG_CHECK(g && (g->E == 0 || vals) && x && t && y, LSPCG_ERR_ARG, "graph_aatpe: NULL argument");
  LSPCG_CHECK(dtype == LSPCG_F32 || dtype == LSPCG_F64, LSPCG_ERR_ARG, "graph_aatpe: bad dtype");
  LSPCG_CHECK(x != y && x != t && t != y, LSPCG_ERR_ARG, "graph_aatpe: x, t and y must not alias");
  LSPCG_HIP(hipSetDevice(g->ctx->device));
  if (int rc = run(g, dtype, true, 0, vals, x, mask, diag, nullptr, 0.0, t)) return rc;
  return run(g, dtype, false, 1, vals, t, mask, diag, x, epsilon, y);
}

int lspcg_graph_spmv_grad_vals(lspcg_graph* g, int dtype, int transpose, const void* gy, const void* x, void* dvals) {
  LSPCG_CHECK(g && gy && x && (g->E == 0 || dvals), LSPCG_ERR_ARG, "graph_spmv_grad_vals: NULL argument");
  LSPCG_CHECK(dtype == LSPCG_F32 || dtype == LSPCG_F64, LSPCG_ERR_ARG, "graph_spmv_grad_vals: bad dtype");
  LSPCG_CHECK(dvals != gy && dvals != x, LSPCG_ERR_ARG, "graph_spmv_grad_vals: dvals must not alias an input");
  LSPCG_HIP(hipSetDevice(g->ctx->device));
  if (int rc = ensure_ends(g)) return rc;
  // y = m ⊙ (A x): dA_e = gy_I ⊗ x_J ; y = m ⊙ (Aᵀ x): dA_e = x_I ⊗ gy_J
  const void* u = transpose ? x : gy;
  const void* v = transpose ? gy : x;
  return dtype == LSPCG_F32 ? outer<float>(g, u, v, nullptr, nullptr, dvals)
                            : outer<double>(g, u, v, nullptr, nullptr, dvals);
}

int lspcg_graph_spai_loss(lspcg_graph* g, const void* Lvals, const void* Avals, int dtype, double epsilon,
                          const void* r, const void* mask, const void* diag, const int64_t* ptr, int64_t B, int kind,
                          double loss_eps, double* loss_out, void* dLvals) {
  LSPCG_CHECK(g && r && ptr && loss_out && (g->E == 0 || (Lvals && Avals)), LSPCG_ERR_ARG,
              "graph_spai_loss: NULL argument");
  LSPCG_CHECK(dtype == LSPCG_F32 || dtype == LSPCG_F64, LSPCG_ERR_ARG, "graph_spai_loss: bad dtype");
  LSPCG_CHECK(kind == 0 || kind == 1, LSPCG_ERR_ARG, "graph_spai_loss: kind must be 0 (relative) or 1 (mse)");
  LSPCG_CHECK(B >= 0 && B < (int64_t(1) << 31), LSPCG_ERR_ARG, "graph_spai_loss: bad graph count");
  const void* lo = loss_out;
  LSPCG_CHECK(lo != dLvals && lo != Lvals && lo != Avals && lo != r && lo != mask && lo != diag && lo != (const void*)ptr,
              LSPCG_ERR_ARG, "graph_spai_loss: loss_out must not alias another argument");
  LSPCG_CHECK(!dLvals || (dLvals != Lvals && dLvals != Avals && dLvals != r && dLvals != mask && dLvals != diag &&
                          dLvals != (const void*)ptr),
              LSPCG_ERR_ARG, "graph_spai_loss: dLvals must not alias an input");
  LSPCG_HIP(hipSetDevice(g->ctx->device));
  if (int rc = set_graphs(g, ptr, B)) return rc;
  if (g->N == 0) {  // no rows: every graph's term is 0 / (0 + eps); nothing that indexes is launched
    LSPCG_HIP(hipMemsetAsync(loss_out, 0, sizeof(double), g->ctx->stream));
    return LSPCG_OK;
  }
  if (int rc = ensure_vecs(g)) return rc;
  if (dLvals)
    if (int rc = ensure_ends(g)) return rc;
  return dtype == LSPCG_F32
             ? loss_chain<float>(g, dtype, Lvals, Avals, epsilon, r, mask, diag, B, kind, loss_eps, loss_out, dLvals)
             : loss_chain<double>(g, dtype, Lvals, Avals, epsilon, r, mask, diag, B, kind, loss_eps, loss_out, dLvals);
}

}  // extern "C"
