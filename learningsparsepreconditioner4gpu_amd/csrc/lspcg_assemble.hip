// Device CSR / BSR assembly with Dirichlet masking -- the GPU form of
// neural_cg/utils/validate.py:22-51 (to_csr_cpu) with neural_cg/data.py:134-156
// (make_bsr_from_coo_inds) and :159-170 (apply_dbc_masking).
//
// Reference semantics reproduced exactly for row-major sorted, duplicate-free edges (the
// only layout make_bsr_from_coo_inds handles correctly, data.py:150-156; checked here):
//   v      = blocks cast to the output dtype
//   v      = 0                     where mask[row] == 0 or mask[col] == 0
//   v_ii  += (1 - mask[i])          (scipy COO + diags(1 - mask))
//   scalar CSR output drops every entry that ends up exactly 0 (scipy csr_plus_csr) and
//   inserts (i,i) when the pattern lacks it and 1 - mask[i] != 0.
// The BSR output keeps the block pattern (zeros inside blocks are harmless for SpMV).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>
#include <string>

#include "lspcg_internal.hpp"

namespace lspcg {

__global__ void k_check_edges(int64_t E, int64_t nb, const int64_t* __restrict__ ei, int* __restrict__ flag) {
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < E; e += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = ei[e], c = ei[E + e];
    int f = 0;
    if (r < 0 || r >= nb || c < 0 || c >= nb) f |= 1;
    if (e > 0) {
      const int64_t rp = ei[e - 1], cp = ei[E + e - 1];
      if (rp > r || (rp == r && cp >= c)) f |= 2;
    }
    if (f) atomicOr(flag, f);
  }
}

// bptr[i] = first edge with row >= i (edges sorted by row)
__global__ void k_block_rowptr(int64_t E, int64_t nb, const int64_t* __restrict__ ei, int32_t* __restrict__ bptr) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i <= nb; i += int64_t(gridDim.x) * blockDim.x) {
    int64_t lo = 0, hi = E;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (ei[mid] < i) lo = mid + 1; else hi = mid;
    }
    bptr[i] = int32_t(lo);
  }
}

template <typename TO, typename TI, typename TM>
struct AsmIn {
  int64_t nb, E;
  const int64_t* ei;
  const TI* blocks;
  const TM* mask;  // nullable
  const int32_t* bptr;
};

template <typename TO, typename TM>
__device__ __forceinline__ TO mask_val(const TM* mask, int64_t i) {
  return mask ? TO(mask[i]) : TO(1);
}

// Scalar CSR output, one 16-lane segment per scalar row (4 rows per wave): the segment walks the
// row's entries 16 at a time (coalesced edge / block reads), ballots give each kept entry its
// output slot.  Same result as scalar_row (above): an entry is kept when its masked value (plus
// 1 - mask on the diagonal) is nonzero; a missing diagonal with 1 - mask != 0 goes right after
// the kept entries left of it.  COUNT writes the per-row count, FILL the entries at rowptr[i].
template <typename TO, typename TI, typename TM, int BS, bool FILL>
__global__ void __launch_bounds__(256) k_asm_rows(AsmIn<TO, TI, TM> in, const int32_t* __restrict__ rowptr,
                                                  int32_t* __restrict__ cnt_out, int32_t* __restrict__ cols,
                                                  TO* __restrict__ vals) {
  const int lane = threadIdx.x & 63, sl = lane & 15;
  const uint64_t segmask = 0xFFFFull << (lane & 48);
  const uint64_t below_me = (1ull << lane) - 1;
  const int64_t nrows = in.nb * BS;
  const int64_t nseg = (int64_t(gridDim.x) * blockDim.x) >> 4;
  for (int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 4; i < nrows; i += nseg) {
    const int64_t I = i / BS;
    const int a = int(i - I * BS);
    const TO mi = mask_val<TO>(in.mask, i);
    const TO ident = TO(1) - mi;
    const bool row_masked = mi == TO(0);
    const int32_t b = in.bptr[I];
    const int32_t ne = (in.bptr[I + 1] - b) * BS;
    auto entry = [&](int32_t t, int64_t& j, TO& v) {  // t-th scalar entry of row i (t < ne)
      const int32_t k = b + t / BS;
      const int c = t % BS;
      j = in.ei[in.E + k] * BS + c;
      v = TO(in.blocks[(int64_t(k) * BS + a) * BS + c]);
      if (row_masked || mask_val<TO>(in.mask, j) == TO(0)) v = TO(0);
      if (j == i) v = v + ident;
    };
    int32_t kept = 0, below = 0;
    bool has_diag = false;
    for (int32_t t0 = 0; t0 < ne; t0 += 16) {
      const int32_t t = t0 + sl;
      bool keep = false, low = false, dg = false;
      if (t < ne) {
        int64_t j;
        TO v;
        entry(t, j, v);
        keep = v != TO(0);
        low = keep && j < i;
        dg = j == i;
      }
      kept += __popcll(__ballot(keep) & segmask);
      below += __popcll(__ballot(low) & segmask);
      has_diag = has_diag || (__ballot(dg) & segmask) != 0;
    }
    const bool ins = !has_diag && ident != TO(0);
    if constexpr (!FILL) {
      if (sl == 0) cnt_out[i] = kept + (ins ? 1 : 0);
    } else {
      const int32_t pos0 = rowptr[i];
      if (ins && sl == 0) {
        cols[pos0 + below] = int32_t(i);
        vals[pos0 + below] = ident;
      }
      int32_t run = 0;
      for (int32_t t0 = 0; t0 < ne; t0 += 16) {
        const int32_t t = t0 + sl;
        bool keep = false;
        int64_t j = 0;
        TO v = TO(0);
        if (t < ne) {
          entry(t, j, v);
          keep = v != TO(0);
        }
        const uint64_t bk = __ballot(keep) & segmask;
        if (keep) {
          const int32_t p = pos0 + run + __popcll(bk & below_me) + ((ins && j > i) ? 1 : 0);
          cols[p] = int32_t(j);
          vals[p] = v;
        }
        run += __popcll(bk);
      }
    }
  }
}

// BSR output: same block pattern; masking applied in place; requires the diagonal block
// wherever 1 - mask != 0 (flag bit 4 otherwise).
template <typename TO, typename TI, typename TM, int BS>
__global__ void k_asm_bsr(AsmIn<TO, TI, TM> in, int32_t* __restrict__ rowptr, int32_t* __restrict__ cols,
                          TO* __restrict__ vals, int* __restrict__ flag) {
  for (int64_t I = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; I < in.nb; I += int64_t(gridDim.x) * blockDim.x) {
    bool has_diag = false;
    for (int32_t k = in.bptr[I]; k < in.bptr[I + 1]; ++k) {
      const int64_t J = in.ei[in.E + k];
      cols[k] = int32_t(J);
      for (int a = 0; a < BS; ++a) {
        const int64_t i = I * BS + a;
        const TO mi = mask_val<TO>(in.mask, i);
        for (int c = 0; c < BS; ++c) {
          const int64_t j = J * BS + c;
          TO v = TO(in.blocks[(k * BS + a) * BS + c]);
          if (mi == TO(0) || mask_val<TO>(in.mask, j) == TO(0)) v = TO(0);
          if (j == i) v = v + (TO(1) - mi);
          vals[(k * BS + a) * BS + c] = v;
        }
      }
      if (J == I) has_diag = true;
    }
    rowptr[I] = in.bptr[I];
    if (I == in.nb - 1) rowptr[in.nb] = in.bptr[in.nb];
    if (!has_diag) {
      for (int a = 0; a < BS; ++a)
        if (TO(1) - mask_val<TO>(in.mask, I * BS + a) != TO(0)) atomicOr(flag, 4);
    }
  }
}

static int seg_grid(int64_t rows) {  // 16 threads per row, grid-stride beyond 16384 workgroups
  int64_t g = (rows * 16 + 255) / 256;
  return int(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

static int grid_of(int64_t n) {
  int64_t g = (n + kThreads - 1) / kThreads;
  return int(g < 1 ? 1 : (g > kElemBlocksMax ? kElemBlocksMax : g));
}

// lspcg_assemble_into: the same count / fill passes into scratch arrays, the resulting pattern compared with
// `into`'s on the device (one flag read), the values copied over only when it is the same.  The
// scratch holds the largest pattern the passes can write (every edge entry kept plus one inserted
// diagonal per row), so the fill is in bounds whatever the mask and the values turned out to be.
template <typename TO, typename TI, typename TM, int BS>
static int assemble_into_t(lspcg_ctx* ctx, const AsmIn<TO, TI, TM>& in, int out_block, lspcg_mat* A, int* flag) {
  hipStream_t st = ctx->stream;
  const int64_t nb = in.nb, E = in.E, n = nb * BS;
  LSPCG_CHECK(A->ctx == ctx && A->storage_dtype() == A->dtype, LSPCG_ERR_ARG, "assemble_into: a matrix of another context");
  LSPCG_CHECK(A->block_size == (out_block ? BS : 1) && A->n == n, LSPCG_ERR_FORMAT,
              "assemble_into: the matrix has another size or block size (nothing written)");
  DevBuf B;
  int32_t *rp = nullptr, *ci = nullptr;
  TO* v = nullptr;
  int hflag = 0;
  if (out_block) {
    if (int rc = B.get(&rp, nb + 1) | B.get(&ci, E) | B.get(&v, E * BS * BS)) return rc;
    hipLaunchKernelGGL((k_asm_bsr<TO, TI, TM, BS>), dim3(grid_of(nb)), dim3(kThreads), 0, st, in, rp, ci, v, flag);
    if (nb == 0) LSPCG_HIP(hipMemsetAsync(rp, 0, sizeof(int32_t), st));
    pattern_neq(rp, A->rowptr, nb + 1, ci, A->colind, std::min(E, A->nnzb), flag, st);
    LSPCG_HIP(hipGetLastError());
    if (int rc = flag_value(flag, st, &hflag)) return rc;
    LSPCG_CHECK(!(hflag & 4), LSPCG_ERR_FORMAT,
                "assemble: BSR output needs the diagonal block of every Dirichlet-masked block row");
    LSPCG_CHECK(!(hflag & 2) && E == A->nnzb, LSPCG_ERR_FORMAT,
                "assemble_into: the assembled pattern differs from the matrix's (nothing written)");
    if (E) LSPCG_HIP(hipMemcpyAsync(A->vals, v, sizeof(TO) * E * BS * BS, hipMemcpyDeviceToDevice, st));
  } else {
    const int64_t cap = E * BS * BS + n;
    int32_t* cnt = nullptr;
    if (int rc = B.get(&cnt, n + 1) | B.get(&rp, n + 1) | B.get(&ci, cap) | B.get(&v, cap)) return rc;
    hipLaunchKernelGGL((k_asm_rows<TO, TI, TM, BS, false>), dim3(seg_grid(n)), dim3(256), 0, st, in,
                       static_cast<const int32_t*>(nullptr), cnt, static_cast<int32_t*>(nullptr), static_cast<TO*>(nullptr));
    LSPCG_HIP(hipMemsetAsync(cnt + n, 0, sizeof(int32_t), st));
    size_t tmp_bytes = 0;
    LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, rp, int(n + 1), st));
    void* tmp = nullptr;
    if (int rc = B.get(&tmp, tmp_bytes)) return rc;
    LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, rp, int(n + 1), st));
    hipLaunchKernelGGL((k_asm_rows<TO, TI, TM, BS, true>), dim3(seg_grid(n)), dim3(256), 0, st, in,
                       static_cast<const int32_t*>(rp), static_cast<int32_t*>(nullptr), ci, v);
    // equal row pointers give equal entry counts, so the columns are compared over A's (a differing
    // row pointer raises the flag whatever the columns say)
    pattern_neq(rp, A->rowptr, n + 1, ci, A->colind, std::min(cap, A->nnzb), flag, st);
    LSPCG_HIP(hipGetLastError());
    if (int rc = flag_value(flag, st, &hflag)) return rc;
    LSPCG_CHECK(!(hflag & 2), LSPCG_ERR_FORMAT,
                "assemble_into: the assembled pattern differs from the matrix's (nothing written)");
    if (A->nnzb) LSPCG_HIP(hipMemcpyAsync(A->vals, v, sizeof(TO) * A->nnzb, hipMemcpyDeviceToDevice, st));
  }
  if (int rc = mat_refresh_spmv(A)) return rc;
  LSPCG_HIP(hipStreamSynchronize(st));  // the scratch is freed on return
  return LSPCG_OK;
}

// `into` (nullable): lspcg_assemble_into's existing handle, *out unused
template <typename TO, typename TI, typename TM, int BS>
static int assemble_t(lspcg_ctx* ctx, int64_t nb, int64_t E, const int64_t* ei, const void* blocks, const void* mask,
                      int out_dtype, int out_block, lspcg_mat** out, lspcg_mat* into) {
  hipStream_t st = ctx->stream;
  DevBuf B;
  int32_t* bptr = nullptr;
  int* flag = nullptr;
  if (int rc = B.get(&bptr, nb + 1) | B.get(&flag, 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  if (E > 0) hipLaunchKernelGGL(k_check_edges, dim3(grid_of(E)), dim3(kThreads), 0, st, E, nb, ei, flag);
  hipLaunchKernelGGL(k_block_rowptr, dim3(grid_of(nb + 1)), dim3(kThreads), 0, st, E, nb, ei, bptr);
  int hflag = 0;
  if (int rc = flag_value(flag, st, &hflag)) return rc;
  LSPCG_CHECK(!(hflag & 1), LSPCG_ERR_FORMAT, "assemble: edge_index out of range");
  LSPCG_CHECK(!(hflag & 2), LSPCG_ERR_FORMAT,
              "assemble: edge_index must be row-major sorted without duplicates (make_bsr_from_coo_inds contract)");
  AsmIn<TO, TI, TM> in{nb, E, ei, static_cast<const TI*>(blocks), static_cast<const TM*>(mask), bptr};
  const int64_t n = nb * BS;
  if (into) return assemble_into_t<TO, TI, TM, BS>(ctx, in, out_block, into, flag);

  std::unique_ptr<lspcg_mat, int (*)(lspcg_mat*)> m(new lspcg_mat(), lspcg_mat_destroy);
  m->ctx = ctx;
  m->dtype = out_dtype;
  if (out_block) {
    m->block_size = BS;
    m->nb = nb;
    m->n = n;
    m->nnzb = E;
    LSPCG_HIP(hipMalloc(&m->rowptr, sizeof(int32_t) * (nb + 1)));
    if (int rc = mat_alloc_entries(m.get(), E)) return rc;
    hipLaunchKernelGGL((k_asm_bsr<TO, TI, TM, BS>), dim3(grid_of(nb)), dim3(kThreads), 0, st, in, m->rowptr,
                       m->colind, static_cast<TO*>(m->vals), flag);
    if (int rc = flag_value(flag, st, &hflag)) return rc;
    LSPCG_CHECK(!(hflag & 4), LSPCG_ERR_FORMAT,
                "assemble: BSR output needs the diagonal block of every Dirichlet-masked block row");
    *out = m.release();
    return LSPCG_OK;
  }
  // scalar CSR: count -> exclusive scan (hipcub) -> fill
  m->block_size = 1;
  m->nb = n;
  m->n = n;
  LSPCG_HIP(hipMalloc(&m->rowptr, sizeof(int32_t) * (n + 1)));
  int32_t* cnt = nullptr;  // counts in [0,n) (+ a zero at n), scanned into rowptr[0..n]
  if (int rc = B.get(&cnt, n + 1)) return rc;
  hipLaunchKernelGGL((k_asm_rows<TO, TI, TM, BS, false>), dim3(seg_grid(n)), dim3(256), 0, st, in,
                     static_cast<const int32_t*>(nullptr), cnt, static_cast<int32_t*>(nullptr), static_cast<TO*>(nullptr));
  LSPCG_HIP(hipMemsetAsync(cnt + n, 0, sizeof(int32_t), st));
  size_t tmp_bytes = 0;
  LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, m->rowptr, int(n + 1), st));
  DevBuf scan;
  void* tmp = nullptr;
  if (int rc = scan.get(&tmp, tmp_bytes)) return rc;
  LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, m->rowptr, int(n + 1), st));
  int32_t nnz = 0;
  if (int rc = flag_value(m->rowptr + n, st, &nnz)) return rc;
  scan.release();
  m->nnzb = nnz;
  if (int rc = mat_alloc_entries(m.get(), nnz)) return rc;
  hipLaunchKernelGGL((k_asm_rows<TO, TI, TM, BS, true>), dim3(seg_grid(n)), dim3(256), 0, st, in, m->rowptr,
                     static_cast<int32_t*>(nullptr), m->colind, static_cast<TO*>(m->vals));
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipStreamSynchronize(st));
  *out = m.release();
  return LSPCG_OK;
}

template <typename TO, typename TI, typename TM>
static int assemble_bs(lspcg_ctx* ctx, int64_t nb, int64_t E, int bs, const int64_t* ei, const void* blocks,
                       const void* mask, int out_dtype, int out_block, lspcg_mat** out, lspcg_mat* into) {
  if (bs == 1) return assemble_t<TO, TI, TM, 1>(ctx, nb, E, ei, blocks, mask, out_dtype, out_block, out, into);
  if (bs == 3) return assemble_t<TO, TI, TM, 3>(ctx, nb, E, ei, blocks, mask, out_dtype, out_block, out, into);
  set_error("assemble: block size must be 1 or 3");
  return LSPCG_ERR_UNSUPPORTED;
}

template <typename TO, typename TI>
static int assemble_m(lspcg_ctx* ctx, int64_t nb, int64_t E, int bs, const int64_t* ei, const void* blocks,
                      const void* mask, int mask_dtype, int out_dtype, int out_block, lspcg_mat** out, lspcg_mat* into) {
  if (mask_dtype == LSPCG_F32)
    return assemble_bs<TO, TI, float>(ctx, nb, E, bs, ei, blocks, mask, out_dtype, out_block, out, into);
  return assemble_bs<TO, TI, double>(ctx, nb, E, bs, ei, blocks, mask, out_dtype, out_block, out, into);
}

}  // namespace lspcg

using namespace lspcg;

static int assemble_any(lspcg_ctx* ctx, int64_t nb, int64_t E, int bs, const int64_t* edge_index, const void* blocks,
                        int in_dtype, const void* mask, int mask_dtype, int out_dtype, int out_block, lspcg_mat** out,
                        lspcg_mat* into) {
  LSPCG_CHECK(ctx && (out || into) && (E == 0 || (edge_index && blocks)), LSPCG_ERR_ARG, "assemble: NULL argument");
  LSPCG_CHECK(nb >= 0 && E >= 0 && nb * bs < (int64_t(1) << 31) && E < (int64_t(1) << 31), LSPCG_ERR_ARG,
              "assemble: sizes out of range");
  LSPCG_HIP(hipSetDevice(ctx->device));
  if (out_dtype == LSPCG_F64) {
    if (in_dtype == LSPCG_F32)
      return assemble_m<double, float>(ctx, nb, E, bs, edge_index, blocks, mask, mask_dtype, out_dtype, out_block, out, into);
    return assemble_m<double, double>(ctx, nb, E, bs, edge_index, blocks, mask, mask_dtype, out_dtype, out_block, out, into);
  }
  if (in_dtype == LSPCG_F32)
    return assemble_m<float, float>(ctx, nb, E, bs, edge_index, blocks, mask, mask_dtype, out_dtype, out_block, out, into);
  return assemble_m<float, double>(ctx, nb, E, bs, edge_index, blocks, mask, mask_dtype, out_dtype, out_block, out, into);
}

extern "C" int lspcg_assemble(lspcg_ctx* ctx, int64_t nb, int64_t E, int bs, const int64_t* edge_index,
                              const void* blocks, int in_dtype, const void* mask, int mask_dtype, int out_dtype,
                              int out_block, lspcg_mat** out) {
  LSPCG_CHECK(out, LSPCG_ERR_ARG, "assemble: NULL argument");
  return assemble_any(ctx, nb, E, bs, edge_index, blocks, in_dtype, mask, mask_dtype, out_dtype, out_block, out, nullptr);
}

extern "C" int lspcg_assemble_into(lspcg_ctx* ctx, int64_t nb, int64_t E, int bs, const int64_t* edge_index,
                                   const void* blocks, int in_dtype, const void* mask, int mask_dtype, int out_block,
                                   lspcg_mat* A) {
  LSPCG_CHECK(A, LSPCG_ERR_ARG, "assemble_into: NULL matrix");
  return assemble_any(ctx, nb, E, bs, edge_index, blocks, in_dtype, mask, mask_dtype, A->dtype, out_block, nullptr, A);
}
