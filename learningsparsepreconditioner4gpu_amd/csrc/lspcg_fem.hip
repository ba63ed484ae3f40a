// P1 finite-element operators of a tetrahedral mesh, assembled on the device into a live lspcg_mat:
// the heat operator A = K(κ) + diag(ρ ⊙ m) (the reference's laplacian(nodes, elem) +
// diags(lumped_mass(...) * field), datagen/heat_tetmesh.py:17-56, datagen/heat.py) and the 3x3-block
// linear-elastic stiffness + mass of problems.elasticity_box (datagen/elast_twist.py).
//
// Analysis, once per connectivity (lspcg_fem_create): the 16 vertex pairs of every tet and one (i, i)
// per vertex become 64-bit keys row * N + col, in the order e = 16 t + 4 a + b, then 16 T + i.  One
// STABLE radix sort of (key, e) yields at once the canonical CSR pattern (the runs of equal keys) and
// the gather map: inside a run the contributions stand in ascending e, i.e. ascending tet, then
// ascending 4 a + b, and the diagonal's marker 16 T + i comes last.  The sorted e ARE the map
// (contrib), eptr[k] is the start of entry k's run.
//
// Assembly.  Every stored value is the left-to-right sum of its run's contributions, each computed
// from the expressions of problems.p1_laplacian_exact in double (-ffp-contract=off); a diagonal entry
// also sums vol / 4 (the lumped mass, same order) and adds the mass term last; the value is rounded
// once on the store.  Heat writes the 4x4 element matrices per tet first and gathers them per entry
// (16 doubles per tet: cheaper than recomputing nine fp64 divisions per contribution); elasticity
// recomputes each incident tet's gradients per stored block instead of moving 1152 B per tet twice
// (both measured).  No atomics on values: the bits depend on neither the grid nor
// earlier calls, and entry (i, j) and entry (j, i) run through the same products in the same order
// -> A is symmetric in bits.  The values land in scratch of the handle and reach the matrix through
// lspcg_mat_set_values with the handle's pattern, so another pattern is refused there and a
// prepare_spmv copy is refilled.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

#include "lspcg_internal.hpp"

struct lspcg_fem {
  lspcg_ctx* ctx = nullptr;
  int64_t N = 0, T = 0, nnz = 0;
  double* nodes = nullptr;     // [N,3]
  int32_t* tets = nullptr;     // [T,4]
  int32_t* indptr = nullptr;   // [N+1]
  int32_t* indices = nullptr;  // [nnz]
  int32_t* eptr = nullptr;     // [nnz+1] runs of contrib
  uint32_t* contrib = nullptr; // [16T+N]: 16 t + 4 a + b, or 16 T + i (the diagonal's marker, last in its run)
  void* scratch = nullptr;     // the values of the last assembly (either dtype, either block size)
  size_t scratch_bytes = 0;
  double* elem = nullptr;      // heat: the element matrices [T,16], then vol / 4 [T]; allocated on first use
  unsigned long long* flag = nullptr;  // first offending tet * 4 + kind
};

namespace lspcg {
namespace {

constexpr unsigned long long kNoTet = ~0ull;
enum { kBadIndex = 0, kBadRepeat = 1, kBadDet = 2 };

struct TetGeo {
  double g0[3], g1[3], g2[3], g3[3];
  double det;
};

// problems.p1_laplacian_exact, expression by expression
__device__ __forceinline__ TetGeo tet_geo(const double* __restrict__ nodes, int32_t v0, int32_t v1, int32_t v2, int32_t v3) {
  const double* p0 = nodes + 3 * int64_t(v0);
  const double* p1 = nodes + 3 * int64_t(v1);
  const double* p2 = nodes + 3 * int64_t(v2);
  const double* p3 = nodes + 3 * int64_t(v3);
  const double x0 = p0[0], y0 = p0[1], z0 = p0[2];
  const double a0 = p1[0] - x0, a1 = p1[1] - y0, a2 = p1[2] - z0;
  const double b0 = p2[0] - x0, b1 = p2[1] - y0, b2 = p2[2] - z0;
  const double c0 = p3[0] - x0, c1 = p3[1] - y0, c2 = p3[2] - z0;
  const double bc0 = b1 * c2 - b2 * c1, bc1 = b2 * c0 - b0 * c2, bc2 = b0 * c1 - b1 * c0;
  const double ca0 = c1 * a2 - c2 * a1, ca1 = c2 * a0 - c0 * a2, ca2 = c0 * a1 - c1 * a0;
  const double ab0 = a1 * b2 - a2 * b1, ab1 = a2 * b0 - a0 * b2, ab2 = a0 * b1 - a1 * b0;
  TetGeo g;
  g.det = (a0 * bc0 + a1 * bc1) + a2 * bc2;
  g.g1[0] = bc0 / g.det, g.g1[1] = bc1 / g.det, g.g1[2] = bc2 / g.det;
  g.g2[0] = ca0 / g.det, g.g2[1] = ca1 / g.det, g.g2[2] = ca2 / g.det;
  g.g3[0] = ab0 / g.det, g.g3[1] = ab1 / g.det, g.g3[2] = ab2 / g.det;
#pragma unroll
  for (int d = 0; d < 3; ++d) g.g0[d] = -((g.g1[d] + g.g2[d]) + g.g3[d]);
  return g;
}

// g_a[d] without a dynamically indexed array: the four values are read first, then selected
__device__ __forceinline__ double sel4(int a, double v0, double v1, double v2, double v3) {
  return a == 0 ? v0 : a == 1 ? v1 : a == 2 ? v2 : v3;
}
__device__ __forceinline__ double pick(const TetGeo& g, int a, int d) { return sel4(a, g.g0[d], g.g1[d], g.g2[d], g.g3[d]); }

__device__ __forceinline__ TetGeo tet_geo_of(const double* __restrict__ nodes, const int32_t* __restrict__ tets, int64_t t) {
  const int4 v = *reinterpret_cast<const int4*>(tets + 4 * t);
  return tet_geo(nodes, v.x, v.y, v.z, v.w);
}

// The checks: vertex range and repeated vertices (check_topology), then the determinant; the first
// offending tet wins (an integer atomicMin on one flag word).
__global__ void __launch_bounds__(256) k_fem_check(int64_t N, int64_t T, const double* __restrict__ nodes,
                                                   const int32_t* __restrict__ tets, bool check_topology,
                                                   unsigned long long* __restrict__ flag) {
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < T; t += int64_t(gridDim.x) * blockDim.x) {
    const int4 v = *reinterpret_cast<const int4*>(tets + 4 * t);
    int bad = -1;
    if (check_topology) {
      if (v.x < 0 || v.x >= N || v.y < 0 || v.y >= N || v.z < 0 || v.z >= N || v.w < 0 || v.w >= N) bad = kBadIndex;
      else if (v.x == v.y || v.x == v.z || v.x == v.w || v.y == v.z || v.y == v.w || v.z == v.w) bad = kBadRepeat;
    }
    if (bad < 0) {
      const double det = tet_geo(nodes, v.x, v.y, v.z, v.w).det;
      if (det == 0.0 || !isfinite(det)) bad = kBadDet;
    }
    if (bad >= 0) atomicMin(flag, (unsigned long long)(t) * 4ull + (unsigned long long)(bad));
  }
}

__global__ void __launch_bounds__(256) k_fem_keys(int64_t N, int64_t T, const int32_t* __restrict__ tets,
                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ ids) {
  const int64_t M = 16 * T + N;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < M; e += int64_t(gridDim.x) * blockDim.x) {
    uint64_t r, c;
    if (e < 16 * T) {
      const int64_t t = e >> 4;
      r = uint64_t(tets[4 * t + ((e >> 2) & 3)]);
      c = uint64_t(tets[4 * t + (e & 3)]);
    } else {
      r = c = uint64_t(e - 16 * T);
    }
    keys[e] = r * uint64_t(N) + c;
    ids[e] = uint32_t(e);
  }
}

__global__ void __launch_bounds__(256) k_fem_heads(int64_t M, const uint64_t* __restrict__ keys, int32_t* __restrict__ head) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < M; k += int64_t(gridDim.x) * blockDim.x)
    head[k] = (k == 0 || keys[k] != keys[k - 1]) ? 1 : 0;
}

// entry[k] = inclusive scan of head: the run starting at k is entry entry[k] - 1
__global__ void __launch_bounds__(256) k_fem_pattern(int64_t N, int64_t M, int64_t nnz, const uint64_t* __restrict__ keys,
                                                     const int32_t* __restrict__ head, const int32_t* __restrict__ entry,
                                                     int32_t* __restrict__ indptr, int32_t* __restrict__ indices,
                                                     int32_t* __restrict__ eptr) {
  const int64_t ts = int64_t(gridDim.x) * blockDim.x, t0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  for (int64_t k = t0; k < M; k += ts)
    if (head[k]) {
      const int32_t e = entry[k] - 1;
      indices[e] = int32_t(keys[k] % uint64_t(N));
      eptr[e] = int32_t(k);
    }
  if (t0 == 0) eptr[nnz] = int32_t(M);
  for (int64_t i = t0; i <= N; i += ts) {
    const uint64_t key = uint64_t(i) * uint64_t(N);
    int64_t lo = 0, hi = M;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    indptr[i] = lo < M ? entry[lo] - 1 : int32_t(nnz);  // the first key >= i N starts a run
  }
}

// m_i = Σ vol_t / 4 over the tets of vertex i, in the order of its diagonal entry's run
__global__ void __launch_bounds__(256) k_fem_mass(int64_t N, int64_t T, const double* __restrict__ nodes,
                                                  const int32_t* __restrict__ tets, const int32_t* __restrict__ indptr,
                                                  const int32_t* __restrict__ indices, const int32_t* __restrict__ eptr,
                                                  const uint32_t* __restrict__ contrib, double* __restrict__ m) {
  const uint32_t T16 = uint32_t(16 * T);
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += int64_t(gridDim.x) * blockDim.x) {
    int32_t lo = indptr[i], hi = indptr[i + 1];
    while (lo < hi) {  // the row's stored diagonal (it always exists)
      const int32_t mid = (lo + hi) >> 1;
      if (indices[mid] < i) lo = mid + 1;
      else hi = mid;
    }
    double s = 0.0;
    for (int32_t k = eptr[lo]; k < eptr[lo + 1]; ++k) {
      const uint32_t c = contrib[k];
      if (c >= T16) break;
      const double vol = fabs(tet_geo_of(nodes, tets, c >> 4).det) / 6.0;
      s = s + vol / 4.0;
    }
    m[i] = s;
  }
}

// ---- elasticity: the recomputing route (shape "b").  One thread per stored block walks its run and
// recomputes each incident tet's gradients from the node coordinates: 1152 B per tet never travel.
template <typename TO>
__global__ void __launch_bounds__(256) k_fem_elasticity(int64_t nnz, int64_t T, const double* __restrict__ nodes,
                                                        const int32_t* __restrict__ tets, const int32_t* __restrict__ eptr,
                                                        const uint32_t* __restrict__ contrib,
                                                        const double* __restrict__ young, const double* __restrict__ poisson,
                                                        double mass_coef, TO* __restrict__ out) {
  const uint32_t T16 = uint32_t(16 * T);
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < nnz; e += int64_t(gridDim.x) * blockDim.x) {
    double s[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) s[q] = 0.0;
    double m = 0.0;
    bool diag = false;
    const int32_t k1 = eptr[e + 1];
    for (int32_t k = eptr[e]; k < k1; ++k) {
      const uint32_t c = contrib[k];
      if (c >= T16) {
        diag = true;
        break;
      }
      const int64_t t = c >> 4;
      const int a = int(c >> 2) & 3, b = int(c) & 3;
      const TetGeo g = tet_geo_of(nodes, tets, t);
      const double vol = fabs(g.det) / 6.0;
      const double E = young[t], nu = poisson[t];
      const double lam = (E * nu) / ((1.0 + nu) * (1.0 - 2.0 * nu));
      const double mu = E / (2.0 * (1.0 + nu));
      const double ga[3] = {pick(g, a, 0), pick(g, a, 1), pick(g, a, 2)};
      const double gb[3] = {pick(g, b, 0), pick(g, b, 1), pick(g, b, 2)};
      const double gg = (ga[0] * gb[0] + ga[1] * gb[1]) + ga[2] * gb[2];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double dij = i == j ? 1.0 : 0.0;
          const double v = (lam * (ga[i] * gb[j]) + mu * (ga[j] * gb[i] + dij * gg)) * vol;
          s[i * 3 + j] = s[i * 3 + j] + v;
        }
      m = m + vol / 4.0;
    }
    if (diag) {
      const double mm = mass_coef * m;
      s[0] = s[0] + mm, s[4] = s[4] + mm, s[8] = s[8] + mm;
    }
    TO* dst = out + e * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) dst[q] = TO(s[q]);
  }
}

// ---- heat: the element route (shape "a" of DESIGN.md §17).  One thread per tet writes its 4x4 element
// matrix and vol / 4, one thread per stored entry then adds what its run points at.
__global__ void __launch_bounds__(256) k_fem_elem_heat(int64_t T, const double* __restrict__ nodes,
                                                       const int32_t* __restrict__ tets, const double* __restrict__ kappa,
                                                       double* __restrict__ elem, double* __restrict__ vol4) {
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < T; t += int64_t(gridDim.x) * blockDim.x) {
    const TetGeo g = tet_geo_of(nodes, tets, t);
    const double vol = fabs(g.det) / 6.0;
    const double w = kappa ? vol * kappa[t] : vol;
    const double* G[4] = {g.g0, g.g1, g.g2, g.g3};
    double* dst = elem + 16 * t;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) dst[4 * a + b] = ((G[a][0] * G[b][0] + G[a][1] * G[b][1]) + G[a][2] * G[b][2]) * w;
    vol4[t] = vol / 4.0;
  }
}

// one thread per stored entry: the sum of what its run points at, the mass term of a diagonal last
template <typename TO>
__global__ void __launch_bounds__(256) k_fem_gather_heat(int64_t nnz, int64_t T, const int32_t* __restrict__ eptr,
                                                         const uint32_t* __restrict__ contrib,
                                                         const double* __restrict__ elem, const double* __restrict__ vol4,
                                                         const double* __restrict__ density, double density_scalar,
                                                         TO* __restrict__ out) {
  const uint32_t T16 = uint32_t(16 * T);
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < nnz; e += int64_t(gridDim.x) * blockDim.x) {
    double s = 0.0, m = 0.0;
    int64_t diag = -1;
    const int32_t k1 = eptr[e + 1];
    for (int32_t k = eptr[e]; k < k1; ++k) {
      const uint32_t c = contrib[k];
      if (c >= T16) {  // the marker: a diagonal entry, and its run ends here
        diag = int64_t(c - T16);
        break;
      }
      s = s + elem[c];
      m = m + vol4[c >> 4];
    }
    if (diag >= 0) s = s + (density ? density[diag] : density_scalar) * m;
    out[e] = TO(s);
  }
}

int grid_of(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return int(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// run the checks on `nodes` (a device array) and report the first offending tet
int check_mesh(lspcg_fem* f, const double* nodes, bool topology, const char* who) {
  if (f->T == 0) return LSPCG_OK;
  hipStream_t st = f->ctx->stream;
  LSPCG_HIP(hipMemsetAsync(f->flag, 0xff, sizeof(unsigned long long), st));
  launch(k_fem_check, dim3(grid_of(f->T)), dim3(256), st, f->N, f->T, nodes, f->tets, topology, f->flag);
  LSPCG_HIP(hipGetLastError());
  unsigned long long h = kNoTet;
  LSPCG_HIP(hipMemcpyAsync(&h, f->flag, sizeof(h), hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  if (h == kNoTet) return LSPCG_OK;
  const char* what[] = {"has a vertex index outside 0..N-1", "repeats a vertex", "has a zero or non-finite determinant"};
  set_error(std::string(who) + ": tet " + std::to_string(h >> 2) + " " + what[h & 3]);
  return LSPCG_ERR_FORMAT;
}

int ensure_scratch(lspcg_fem* f, size_t bytes) {
  if (bytes <= f->scratch_bytes) return LSPCG_OK;
  LSPCG_HIP(hipStreamSynchronize(f->ctx->stream));  // the previous assembly may still be copied from it
  (void)hipFree(f->scratch);
  f->scratch = nullptr, f->scratch_bytes = 0;
  LSPCG_HIP(hipMalloc(&f->scratch, bytes));
  f->scratch_bytes = bytes;
  return LSPCG_OK;
}

// heat's element matrices [T,16] and vol / 4 [T], allocated on the first heat call
int ensure_elem(lspcg_fem* f) {
  if (f->elem) return LSPCG_OK;
  LSPCG_HIP(hipMalloc(&f->elem, sizeof(double) * 17 * size_t(std::max<int64_t>(f->T, 1))));
  return LSPCG_OK;
}

// out must be a matrix of the handle's shape; its pattern is compared by lspcg_mat_set_values
int check_out(const lspcg_fem* f, const lspcg_mat* out, int bs, const char* who) {
  LSPCG_CHECK(out->ctx == f->ctx, LSPCG_ERR_ARG, std::string(who) + ": out belongs to another context");
  LSPCG_CHECK(out->block_size == bs && out->nb == f->N && out->nnzb == f->nnz, LSPCG_ERR_FORMAT,
              std::string(who) + ": out is not a block-size-" + std::to_string(bs) +
                  " matrix of the mesh's size and entry count (nothing written)");
  return LSPCG_OK;
}

}  // namespace
}  // namespace lspcg

using namespace lspcg;

extern "C" {

int lspcg_fem_destroy(lspcg_fem* f) {
  if (!f) return LSPCG_OK;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  for (void* p : {(void*)f->nodes, (void*)f->tets, (void*)f->indptr, (void*)f->indices, (void*)f->eptr,
                  (void*)f->contrib, f->scratch, (void*)f->flag, (void*)f->elem})
    (void)hipFree(p);
  delete f;
  return LSPCG_OK;
}

int lspcg_fem_create(lspcg_ctx* ctx, int64_t N, int64_t T, const double* nodes, const int32_t* tets, lspcg_fem** out) {
  LSPCG_CHECK(ctx && out && (N == 0 || nodes) && (T == 0 || tets), LSPCG_ERR_ARG, "fem_create: NULL argument");
  LSPCG_CHECK(N >= 0 && T >= 0, LSPCG_ERR_ARG, "fem_create: negative size");
  const int64_t lim = int64_t(1) << 31;
  LSPCG_CHECK(N < lim && T < lim / 16 && 16 * T + N < lim, LSPCG_ERR_ARG,
              "fem_create: 16 T + N does not fit an int32 index");
  LSPCG_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::unique_ptr<lspcg_fem, int (*)(lspcg_fem*)> f(new lspcg_fem(), lspcg_fem_destroy);
  f->ctx = ctx;
  f->N = N;
  f->T = T;
  const int64_t M = 16 * T + N;
  LSPCG_HIP(hipMalloc(&f->nodes, sizeof(double) * 3 * std::max<int64_t>(N, 1)));
  LSPCG_HIP(hipMalloc(&f->tets, sizeof(int32_t) * 4 * std::max<int64_t>(T, 1)));
  LSPCG_HIP(hipMalloc(&f->indptr, sizeof(int32_t) * (N + 1)));
  LSPCG_HIP(hipMalloc(&f->contrib, sizeof(uint32_t) * std::max<int64_t>(M, 1)));
  LSPCG_HIP(hipMalloc(&f->flag, sizeof(unsigned long long)));
  if (N) LSPCG_HIP(hipMemcpyAsync(f->nodes, nodes, sizeof(double) * 3 * N, hipMemcpyDefault, st));
  if (T) LSPCG_HIP(hipMemcpyAsync(f->tets, tets, sizeof(int32_t) * 4 * T, hipMemcpyDefault, st));
  LSPCG_HIP(hipStreamSynchronize(st));  // host sources may be released by the caller
  if (int rc = check_mesh(f.get(), f->nodes, true, "fem_create")) return rc;
  if (N == 0) {  // (T > 0 was refused by the range check) the empty matrix
    LSPCG_HIP(hipMemsetAsync(f->indptr, 0, sizeof(int32_t), st));
    LSPCG_HIP(hipMalloc(&f->indices, sizeof(int32_t)));
    LSPCG_HIP(hipMalloc(&f->eptr, sizeof(int32_t)));
    LSPCG_HIP(hipMemsetAsync(f->eptr, 0, sizeof(int32_t), st));
    LSPCG_HIP(hipStreamSynchronize(st));
    *out = f.release();
    return LSPCG_OK;
  }
  DevBuf B;
  uint64_t *keys = nullptr, *ks = nullptr;
  uint32_t* ids = nullptr;
  int32_t *head = nullptr, *entry = nullptr;
  void* tmp = nullptr;
  if (int rc = B.get(&keys, M) | B.get(&ks, M) | B.get(&ids, M) | B.get(&head, M) | B.get(&entry, M)) return rc;
  launch(k_fem_keys, dim3(grid_of(M)), dim3(256), st, N, T, f->tets, keys, ids);
  LSPCG_HIP(hipGetLastError());
  int bits = 1;
  while (bits < 64 && (uint64_t(1) << bits) < uint64_t(N) * uint64_t(N)) ++bits;
  size_t tb_sort = 0, tb_scan = 0;
  LSPCG_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, keys, ks, ids, f->contrib, int(M), 0, bits, st));
  LSPCG_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, tb_scan, head, entry, int(M), st));
  if (int rc = B.get(&tmp, std::max(tb_sort, tb_scan))) return rc;
  LSPCG_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb_sort, keys, ks, ids, f->contrib, int(M), 0, bits, st));
  launch(k_fem_heads, dim3(grid_of(M)), dim3(256), st, M, ks, head);
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipcub::DeviceScan::InclusiveSum(tmp, tb_scan, head, entry, int(M), st));
  int nnz32 = 0;
  if (int rc = flag_value(entry + (M - 1), st, &nnz32)) return rc;
  const int64_t nnz = nnz32;
  LSPCG_CHECK(nnz > 0 && 9 * nnz < lim, LSPCG_ERR_ARG, "fem_create: 9 x the entry count does not fit an int32 index");
  f->nnz = nnz;
  LSPCG_HIP(hipMalloc(&f->indices, sizeof(int32_t) * nnz));
  LSPCG_HIP(hipMalloc(&f->eptr, sizeof(int32_t) * (nnz + 1)));
  launch(k_fem_pattern, dim3(grid_of(M)), dim3(256), st, N, M, nnz, ks, head, entry, f->indptr, f->indices, f->eptr);
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipStreamSynchronize(st));  // the scratch arrays go out of scope
  *out = f.release();
  return LSPCG_OK;
}

int lspcg_fem_set_nodes(lspcg_fem* f, const double* nodes) {
  LSPCG_CHECK(f && (f->N == 0 || nodes), LSPCG_ERR_ARG, "fem_set_nodes: NULL argument");
  LSPCG_HIP(hipSetDevice(f->ctx->device));
  if (f->N == 0) return LSPCG_OK;
  hipStream_t st = f->ctx->stream;
  DevBuf B;
  double* d = nullptr;
  if (int rc = B.get(&d, 3 * f->N)) return rc;
  LSPCG_HIP(hipMemcpyAsync(d, nodes, sizeof(double) * 3 * f->N, hipMemcpyDefault, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  if (int rc = check_mesh(f, d, false, "fem_set_nodes")) return rc;  // the old coordinates stay
  LSPCG_HIP(hipMemcpyAsync(f->nodes, d, sizeof(double) * 3 * f->N, hipMemcpyDeviceToDevice, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  return LSPCG_OK;
}

int lspcg_fem_info(const lspcg_fem* f, int64_t* N, int64_t* T, int64_t* nnz) {
  LSPCG_CHECK(f, LSPCG_ERR_ARG, "fem_info: NULL");
  if (N) *N = f->N;
  if (T) *T = f->T;
  if (nnz) *nnz = f->nnz;
  return LSPCG_OK;
}

int lspcg_fem_pattern(const lspcg_fem* f, int32_t* indptr, int32_t* indices) {
  LSPCG_CHECK(f, LSPCG_ERR_ARG, "fem_pattern: NULL");
  LSPCG_HIP(hipSetDevice(f->ctx->device));
  hipStream_t st = f->ctx->stream;
  if (indptr) LSPCG_HIP(hipMemcpyAsync(indptr, f->indptr, sizeof(int32_t) * (f->N + 1), hipMemcpyDefault, st));
  if (indices && f->nnz) LSPCG_HIP(hipMemcpyAsync(indices, f->indices, sizeof(int32_t) * f->nnz, hipMemcpyDefault, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  return LSPCG_OK;
}

int lspcg_fem_lumped_mass(lspcg_fem* f, double* m) {
  LSPCG_CHECK(f && (f->N == 0 || m), LSPCG_ERR_ARG, "fem_lumped_mass: NULL argument");
  LSPCG_HIP(hipSetDevice(f->ctx->device));
  if (f->N == 0) return LSPCG_OK;
  launch(k_fem_mass, dim3(grid_of(f->N)), dim3(256), f->ctx->stream, f->N, f->T, f->nodes, f->tets, f->indptr,
         f->indices, f->eptr, f->contrib, m);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

int lspcg_fem_heat(lspcg_fem* f, const double* kappa, const double* density, double density_scalar, lspcg_mat* out) {
  LSPCG_CHECK(f && out, LSPCG_ERR_ARG, "fem_heat: NULL argument");
  LSPCG_HIP(hipSetDevice(f->ctx->device));
  if (int rc = check_out(f, out, 1, "fem_heat")) return rc;
  const int64_t nnz = f->nnz;
  if (nnz) {
    if (int rc = ensure_scratch(f, size_t(nnz) * (out->dtype == LSPCG_F32 ? 4 : 8))) return rc;
    if (int rc = ensure_elem(f)) return rc;
    double* vol4 = f->elem + 16 * f->T;
    if (f->T)
      launch(k_fem_elem_heat, dim3(grid_of(f->T)), dim3(256), f->ctx->stream, f->T, f->nodes, f->tets, kappa, f->elem,
             vol4);
    by_dtype(out->dtype, [&](auto t) {
      using TO = decltype(t);
      launch(k_fem_gather_heat<TO>, dim3(grid_of(nnz)), dim3(256), f->ctx->stream, nnz, f->T, f->eptr, f->contrib,
             f->elem, vol4, density, density_scalar, as<TO>(f->scratch));
    });
    LSPCG_HIP(hipGetLastError());
  }
  return lspcg_mat_set_values(out, f->indptr, f->indices, f->scratch, out->dtype);
}

int lspcg_fem_elasticity(lspcg_fem* f, const double* young, const double* poisson, double mass_coef, lspcg_mat* out) {
  LSPCG_CHECK(f && out && (f->T == 0 || (young && poisson)), LSPCG_ERR_ARG, "fem_elasticity: NULL argument");
  LSPCG_HIP(hipSetDevice(f->ctx->device));
  if (int rc = check_out(f, out, 3, "fem_elasticity")) return rc;
  const int64_t nnz = f->nnz;
  if (nnz) {
    if (int rc = ensure_scratch(f, size_t(nnz) * 9 * (out->dtype == LSPCG_F32 ? 4 : 8))) return rc;
    by_dtype(out->dtype, [&](auto t) {
      using TO = decltype(t);
      launch(k_fem_elasticity<TO>, dim3(grid_of(nnz)), dim3(256), f->ctx->stream, nnz, f->T, f->nodes, f->tets,
             f->eptr, f->contrib, young, poisson, mass_coef, as<TO>(f->scratch));
    });
    LSPCG_HIP(hipGetLastError());
  }
  return lspcg_mat_set_values(out, f->indptr, f->indices, f->scratch, out->dtype);
}

}  // extern "C"
