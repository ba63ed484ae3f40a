// Backward of the SPAI GNN (NodeEdgeProcessing): the gradient of every Linear weight / bias and
// LayerNorm gamma / beta for a given d loss / d out, laid out like the packed weight blob.
//
// lspcg_gnn_backward recomputes instead of saving: a plain-fp32 training forward stores the
// per-layer inputs x_l [N,16], e_l [E,16] (CSC slot order) and the aggregated messages a_l, then
// the layers are walked in reverse and every pre-activation is recomputed inside the backward
// kernels.  It does not depend on which kernels (split-f16 / fp32) the inference forward runs.
//
// Layout: one wave (= one 64-thread workgroup) owns a tile of 16 items (edges or nodes); lane
// l = (item l & 15, quarter q = l >> 4) holds features 4q .. 4q+3 of each 16-wide block of its
// item ("accumulator layout" of v_mfma_f32_16x16x4_f32, as in lspcg_gnn.hip).  Weights sit in LDS
// in their natural [unit][input] layout (padded strides), so the same copy serves W (forward),
// W^T (input gradients) as the A operand.  The LayerNorm affine is folded into the first Linear
// (W1' = W1 diag(gamma), b1' = b1 + W1 beta), the kernels produce d W1', d b1', and k_unfold
// turns them into d W1, d gamma, d beta at the end.
//
// Parameter gradients dW = sum_items delta (x) in are MFMAs with the item index as K: the tile's
// delta and input rows go through LDS (a transpose), 16 items are four K steps, and the sums stay
// in registers over all tiles of a workgroup.  Each workgroup writes its partial block; k_reduce
// adds the partials in a fixed order in double.  The register sums are fp32 over at most kFlush
// tiles; they are then added into a double block of the workgroup in LDS, which becomes its
// partial.  No floating-point atomics anywhere; the grid depends on (N, E) only, so the same
// inputs give the same bits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>

#include "lspcg_internal.hpp"
#include "lspcg_gnn.hpp"

namespace lspcg {
namespace {

constexpr int kMaxGrid = 2048;  // workgroups (= partial blocks) of a tile kernel

// Padded gradient block of one FeedForward (partials and their double sums):
// [dW1 (16 x 48) | db1 | dW2 (16 x 16) | db2 | dW3 (16 x 16) | db3]
constexpr int FFG = 1328;
constexpr int gW1 = 0, gB1 = 768, gW2 = 784, gB2 = 1040, gW3 = 1056, gB3 = 1312;

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float comp(f4 v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }
__device__ __forceinline__ f4 zero4() { return f4{0.f, 0.f, 0.f, 0.f}; }

// sum over the 4 lanes of an item (l, l^16, l^32, l^48): gfx950's row-swap permutes
__device__ __forceinline__ float swap_sum16(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const unsigned long long r = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_permlane16_swap(u, u, false, false));
  return __builtin_bit_cast(float, unsigned(r)) + __builtin_bit_cast(float, unsigned(r >> 32));
}
__device__ __forceinline__ float swap_sum32(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const unsigned long long r = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_permlane32_swap(u, u, false, false));
  return __builtin_bit_cast(float, unsigned(r)) + __builtin_bit_cast(float, unsigned(r >> 32));
}
__device__ __forceinline__ float quad_sum(float v) { return swap_sum32(swap_sum16(v)); }

// exact-erf GELU and its derivative Phi(v) + v phi(v)
__device__ __forceinline__ float gelu1(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float dgelu1(float v) {
  const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752f));
  return fmaf(v * 0.39894228040143268f, expf(-0.5f * v * v), cdf);
}
__device__ __forceinline__ f4 gelu(f4 v) { return f4{gelu1(v.x), gelu1(v.y), gelu1(v.z), gelu1(v.w)}; }
__device__ __forceinline__ f4 dgelu(f4 v) { return f4{dgelu1(v.x), dgelu1(v.y), dgelu1(v.z), dgelu1(v.w)}; }

// ---- one FeedForward in LDS: W1' [16][16 NB] (row stride 16 NB + 1), b1', W2, W3 (stride 17), b2, b3
template <int NB>
struct FFL {
  static constexpr int S1 = 16 * NB + 1;
  static constexpr int oB1 = 16 * S1, oW2 = oB1 + 16, oB2 = oW2 + 16 * 17, oW3 = oB2 + 16, oB3 = oW3 + 16 * 17;
  static constexpr int SIZE = (oB3 + 16 + 3) & ~3;
};

// gw: the FF's block of the packed blob [W1 | b1 | W2 | b2 | W3 | b3]; ln: [gamma (in) | beta (in)] or null
template <int NB>
__device__ void load_ff(float* w, const float* __restrict__ gw, int in, int out, const float* __restrict__ ln,
                        int lane) {
  using L = FFL<NB>;
  const float* W1 = gw;
  const float* b1 = W1 + H * in;
  const float* W2 = b1 + H;
  const float* b2 = W2 + H * H;
  const float* W3 = b2 + H;
  const float* b3 = W3 + out * H;
  for (int idx = lane; idx < 16 * 16 * NB; idx += 64) {
    const int u = idx / (16 * NB), f = idx % (16 * NB);
    float v = 0.f;
    if (f < in) {
      v = W1[u * in + f];
      if (ln) v *= ln[f];
    }
    w[u * L::S1 + f] = v;
  }
  for (int idx = lane; idx < 256; idx += 64) {
    const int u = idx >> 4, k = idx & 15;
    w[L::oW2 + u * 17 + k] = W2[idx];
    w[L::oW3 + u * 17 + k] = u < out ? W3[idx] : 0.f;
  }
  if (lane < 16) {
    float bb = b1[lane];
    if (ln)
      for (int f = 0; f < in; ++f) bb = fmaf(W1[lane * in + f], ln[in + f], bb);
    w[L::oB1 + lane] = bb;
    w[L::oB2 + lane] = b2[lane];
    w[L::oB3 + lane] = lane < out ? b3[lane] : 0.f;
  }
}

template <int NB>
struct Acc {
  f4 w1[NB], b1, w2, b2, w3, b3;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int b = 0; b < NB; ++b) w1[b] = zero4();
    b1 = w2 = b2 = w3 = b3 = zero4();
  }
  // Adds the sums into the workgroup's double block `p` in LDS and clears them: lane (j = lane & 15,
  // q) owns rows 4q + r (unit), column j (input) of each product, so no two lanes share an entry.
  // Called every kFlush tiles, which keeps an fp32 sum to a few hundred terms.
  __device__ __forceinline__ void flush(double* p, int lane) {
    const int j = lane & 15, q = lane >> 4;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) p[gW1 + (4 * q + r) * 48 + 16 * b + j] += double(comp(w1[b], r));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[gW2 + (4 * q + r) * 16 + j] += double(comp(w2, r));
      p[gW3 + (4 * q + r) * 16 + j] += double(comp(w3, r));
    }
    if (j == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[gB1 + 4 * q + r] += double(comp(b1, r));
        p[gB2 + 4 * q + r] += double(comp(b2, r));
        p[gB3 + 4 * q + r] += double(comp(b3, r));
      }
    }
    zero();
  }
};

constexpr int kFlush = 8;  // tiles between two flushes of the fp32 sums into the double block

__device__ __forceinline__ void clear_block(double* p, int n, int lane) {
  for (int i = lane; i < n; i += 64) p[i] = 0.0;
}
// the workgroup's double block -> its partial block in global memory
__device__ __forceinline__ void store_block(double* __restrict__ out, const double* p, int n, int lane) {
  __syncthreads();
  for (int i = lane; i < n; i += 64) out[i] = p[i];
}

// forward: a1, a2 the two hidden pre-activations, o the output (accumulator layout)
template <int NB>
__device__ __forceinline__ void ff_fwd(const float* w, const f4 (&in)[NB], int lane, f4& a1, f4& a2, f4& o) {
  using L = FFL<NB>;
  const int i = lane & 15, q = lane >> 4;
  a1 = f4{w[L::oB1 + 4 * q], w[L::oB1 + 4 * q + 1], w[L::oB1 + 4 * q + 2], w[L::oB1 + 4 * q + 3]};
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int s = 0; s < 4; ++s) a1 = mfma(w[i * L::S1 + 16 * b + 4 * q + s], comp(in[b], s), a1);
  const f4 h1 = gelu(a1);
  a2 = f4{w[L::oB2 + 4 * q], w[L::oB2 + 4 * q + 1], w[L::oB2 + 4 * q + 2], w[L::oB2 + 4 * q + 3]};
#pragma unroll
  for (int s = 0; s < 4; ++s) a2 = mfma(w[L::oW2 + i * 17 + 4 * q + s], comp(h1, s), a2);
  const f4 h2 = gelu(a2);
  o = f4{w[L::oB3 + 4 * q], w[L::oB3 + 4 * q + 1], w[L::oB3 + 4 * q + 2], w[L::oB3 + 4 * q + 3]};
#pragma unroll
  for (int s = 0; s < 4; ++s) o = mfma(w[L::oW3 + i * 17 + 4 * q + s], comp(h2, s), o);
}

// dW += delta^T in over the tile's 16 items (K slot q of step s = item 4s + q), db += delta^T 1;
// tD: the tile's delta rows [16][16], tI: its input rows [16][stride] in LDS
__device__ __forceinline__ void grad_w(const float* tD, const float* tI, int stride, int col0, int lane, f4& dw) {
  const int i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) dw = mfma(tD[(4 * s + q) * 16 + i], tI[(4 * s + q) * stride + col0 + i], dw);
}
__device__ __forceinline__ void grad_b(const float* tD, int lane, f4& db) {
  const int i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) db = mfma(tD[(4 * s + q) * 16 + i], 1.0f, db);
}

// backward of one FF on a tile: dout = d loss / d output (zero for items past the end), tIn = the
// tile's input rows [16][16 NB] already in LDS; adds the parameter gradients into G and, with DIN,
// returns d loss / d input.  tD / tH: two [16][16] staging tiles of this wave.
template <int NB, bool DIN>
__device__ __forceinline__ void ff_bwd(const float* w, const float* tIn, float* tD, float* tH, f4 a1, f4 a2, f4 dout,
                                       int lane, Acc<NB>& G, f4 (&din)[NB]) {
  using L = FFL<NB>;
  const int i = lane & 15, q = lane >> 4, row = (lane & 15) * 16 + 4 * q;
  // layer 3
  __syncthreads();
  st4(tD + row, dout);
  st4(tH + row, gelu(a2));
  __syncthreads();
  grad_w(tD, tH, 16, 0, lane, G.w3);
  grad_b(tD, lane, G.b3);
  f4 d2 = zero4();
#pragma unroll
  for (int s = 0; s < 4; ++s) d2 = mfma(w[L::oW3 + (4 * q + s) * 17 + i], comp(dout, s), d2);
  d2 *= dgelu(a2);
  // layer 2
  __syncthreads();
  st4(tD + row, d2);
  st4(tH + row, gelu(a1));
  __syncthreads();
  grad_w(tD, tH, 16, 0, lane, G.w2);
  grad_b(tD, lane, G.b2);
  f4 d1 = zero4();
#pragma unroll
  for (int s = 0; s < 4; ++s) d1 = mfma(w[L::oW2 + (4 * q + s) * 17 + i], comp(d2, s), d1);
  d1 *= dgelu(a1);
  // layer 1
  __syncthreads();
  st4(tD + row, d1);
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NB; ++b) grad_w(tD, tIn, 16 * NB, 16 * b, lane, G.w1[b]);
  grad_b(tD, lane, G.b1);
  if constexpr (DIN) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      din[b] = zero4();
#pragma unroll
      for (int s = 0; s < 4; ++s) din[b] = mfma(w[(4 * q + s) * L::S1 + 16 * b + i], comp(d1, s), din[b]);
    }
  }
}

// LayerNorm without affine over the 16 NB features of an item (biased variance, eps 1e-5)
template <int NB>
__device__ __forceinline__ float ln_fwd(f4 (&f)[NB]) {
  constexpr float inv = 1.0f / float(16 * NB);
  float s = 0.f;
#pragma unroll
  for (int b = 0; b < NB; ++b) s += (f[b].x + f[b].y) + (f[b].z + f[b].w);
  const float mean = quad_sum(s) * inv;
  float sq = 0.f;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    f[b] -= mean;
    sq += (f[b].x * f[b].x + f[b].y * f[b].y) + (f[b].z * f[b].z + f[b].w * f[b].w);
  }
  const float rstd = 1.0f / sqrtf(quad_sum(sq) * inv + 1e-5f);
#pragma unroll
  for (int b = 0; b < NB; ++b) f[b] *= rstd;
  return rstd;
}
// df = rstd (dfh - mean(dfh) - fh mean(dfh fh))
template <int NB>
__device__ __forceinline__ void ln_bwd(const f4 (&fh)[NB], float rstd, f4 (&d)[NB]) {
  constexpr float inv = 1.0f / float(16 * NB);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    s1 += (d[b].x + d[b].y) + (d[b].z + d[b].w);
    const f4 p = d[b] * fh[b];
    s2 += (p.x + p.y) + (p.z + p.w);
  }
  s1 = quad_sum(s1) * inv;
  s2 = quad_sum(s2) * inv;
#pragma unroll
  for (int b = 0; b < NB; ++b) d[b] = (d[b] - s1 - fh[b] * s2) * rstd;
}

// ---------------------------------------------------------------------------
// Encoders: out = FF(in[row]) (forward) / parameter gradients for dy (backward)
// ---------------------------------------------------------------------------
template <int NB, bool BWD>
__global__ void __launch_bounds__(64) k_enc(int64_t M, const float* __restrict__ wenc, int fin,
                                            const float* __restrict__ in, const int32_t* __restrict__ idx,
                                            float* __restrict__ out, const float* __restrict__ dy,
                                            double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float w[FFL<NB>::SIZE];
  __shared__ __attribute__((aligned(16))) float tIn[16 * 16 * NB], tD[256], tH[256];
  __shared__ double gacc[BWD ? FFG : 1];
  const int lane = threadIdx.x, it = lane & 15, q = lane >> 4;
  load_ff<NB>(w, wenc, fin, H, nullptr, lane);
  if constexpr (BWD) clear_block(gacc, FFG, lane);
  __syncthreads();
  Acc<NB> G;
  G.zero();
  [[maybe_unused]] int done = 0;
  const int64_t ntiles = (M + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t m = t * 16 + it;
    const bool valid = m < M;
    const int64_t mm = valid ? m : M - 1;
    const int64_t row = idx ? int64_t(idx[mm]) : mm;
    f4 v[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float c[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * b + 4 * q + r;
        c[r] = f < fin ? in[row * fin + f] : 0.f;
      }
      v[b] = f4{c[0], c[1], c[2], c[3]};
    }
    f4 a1, a2, o;
    ff_fwd<NB>(w, v, lane, a1, a2, o);
    if constexpr (!BWD) {
      if (valid) st4(out + mm * H + 4 * q, o);
    } else {
      __syncthreads();
#pragma unroll
      for (int b = 0; b < NB; ++b) st4(tIn + it * 16 * NB + 16 * b + 4 * q, v[b]);
      const f4 d = valid ? ld4(dy + mm * H + 4 * q) : zero4();
      f4 din[NB];
      ff_bwd<NB, false>(w, tIn, tD, tH, a1, a2, d, lane, G, din);
      if ((++done & (kFlush - 1)) == 0) G.flush(gacc, lane);
    }
  }
  if constexpr (BWD) {
    G.flush(gacc, lane);
    store_block(part + int64_t(blockIdx.x) * FFG, gacc, FFG, lane);
  }
}

// ---------------------------------------------------------------------------
// Edge half of an MPLayer over CSC slots.  wl: the layer's block of the packed blob
// [node LN, FF | edge LN, FF | msg LN, FF].
// forward : enext_k = [res] e_k + FF_edge(LN f_k), msg_k = FF_msg(LN f_k), f_k = [x[dst], x[src], e_k]
// backward: delta msg_k = da[dst_k], delta enew_k = de_k  ->  dfd_k, dfs_k (d / d x[dst], x[src]),
//           de_k <- [res] de_k + d f_k[32:48], parameter partials [edge | msg]
// ---------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(64) k_edge_layer(int64_t E, const float* __restrict__ wl, int edge_res,
                                                   const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                   const float* __restrict__ x, const float* __restrict__ e,
                                                   float* __restrict__ enext, float* __restrict__ msg,
                                                   const float* __restrict__ da, float* __restrict__ de,
                                                   float* __restrict__ dfd, float* __restrict__ dfs,
                                                   double* __restrict__ part) {
  using L = FFL<3>;
  __shared__ __attribute__((aligned(16))) float wm[L::SIZE], we[L::SIZE];
  __shared__ __attribute__((aligned(16))) float tIn[16 * 48], tD[256], tH[256];
  __shared__ double gacc[BWD ? 2 * FFG : 1];  // [edge | msg]
  const int lane = threadIdx.x, it = lane & 15, q = lane >> 4;
  if constexpr (BWD) clear_block(gacc, 2 * FFG, lane);
  [[maybe_unused]] int done = 0;
  const float* gedge = wl + gnn_layer_off(kFFEdge);
  const float* gmsg = wl + gnn_layer_off(kFFMsg);
  load_ff<3>(we, gedge + 6 * H, 3 * H, H, gedge, lane);
  load_ff<3>(wm, gmsg + 6 * H, 3 * H, H, gmsg, lane);
  __syncthreads();
  Acc<3> Gm, Ge;
  Gm.zero();
  Ge.zero();
  const int64_t ntiles = (E + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t k = t * 16 + it;
    const bool valid = k < E;
    const int64_t kk = valid ? k : E - 1;
    const int64_t nd = dst[kk], ns = src[kk];
    f4 f[3] = {ld4(x + nd * H + 4 * q), ld4(x + ns * H + 4 * q), ld4(e + kk * H + 4 * q)};
    const f4 ea = f[2];
    const float rstd = ln_fwd<3>(f);
    f4 a1, a2, o;
    if constexpr (!BWD) {
      ff_fwd<3>(wm, f, lane, a1, a2, o);
      if (valid) st4(msg + kk * H + 4 * q, o);
      ff_fwd<3>(we, f, lane, a1, a2, o);
      if (edge_res) o += ea;
      if (valid) st4(enext + kk * H + 4 * q, o);
    } else {
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 3; ++b) st4(tIn + it * 48 + 16 * b + 4 * q, f[b]);
      const f4 dm = valid ? ld4(da + nd * H + 4 * q) : zero4();
      const f4 dee = valid ? ld4(de + kk * H + 4 * q) : zero4();
      f4 d[3], d2[3];
      ff_fwd<3>(wm, f, lane, a1, a2, o);
      ff_bwd<3, true>(wm, tIn, tD, tH, a1, a2, dm, lane, Gm, d);
      ff_fwd<3>(we, f, lane, a1, a2, o);
      ff_bwd<3, true>(we, tIn, tD, tH, a1, a2, dee, lane, Ge, d2);
#pragma unroll
      for (int b = 0; b < 3; ++b) d[b] += d2[b];
      ln_bwd<3>(f, rstd, d);
      if (valid) {
        st4(dfd + kk * H + 4 * q, d[0]);
        st4(dfs + kk * H + 4 * q, d[1]);
        st4(de + kk * H + 4 * q, edge_res ? dee + d[2] : d[2]);
      }
      if ((++done & (kFlush - 1)) == 0) {
        Ge.flush(gacc, lane);
        Gm.flush(gacc + FFG, lane);
      }
    }
  }
  if constexpr (BWD) {
    Ge.flush(gacc, lane);
    Gm.flush(gacc + FFG, lane);
    store_block(part + int64_t(blockIdx.x) * (2 * FFG), gacc, 2 * FFG, lane);
  }
}

// ---------------------------------------------------------------------------
// Node half of an MPLayer.  forward: a_i = sum of the messages of CSC row i (stored), xnext_i =
// [res] x_i + FF_node(LN a_i).  backward: dxn_i = d / d xnext_i -> da_i, parameter partials.
// ---------------------------------------------------------------------------
template <bool BWD>
__global__ void __launch_bounds__(64) k_node_layer(int64_t N, const float* __restrict__ wl, int node_res,
                                                   const int32_t* __restrict__ ptr, const float* __restrict__ msg,
                                                   const float* __restrict__ x, float* __restrict__ as,
                                                   float* __restrict__ xnext, const float* __restrict__ dxn,
                                                   float* __restrict__ da, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float w[FFL<1>::SIZE];
  __shared__ __attribute__((aligned(16))) float tIn[256], tD[256], tH[256];
  __shared__ double gacc[BWD ? FFG : 1];
  const int lane = threadIdx.x, it = lane & 15, q = lane >> 4;
  load_ff<1>(w, wl + 2 * H, H, H, wl, lane);
  if constexpr (BWD) clear_block(gacc, FFG, lane);
  [[maybe_unused]] int done = 0;
  __syncthreads();
  Acc<1> G;
  G.zero();
  const int64_t ntiles = (N + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i = t * 16 + it;
    const bool valid = i < N;
    const int64_t ii = valid ? i : N - 1;
    f4 a[1];
    if constexpr (!BWD) {
      a[0] = zero4();
      if (valid) {
        const int k1 = ptr[ii + 1];
        for (int k = ptr[ii]; k < k1; ++k) a[0] += ld4(msg + int64_t(k) * H + 4 * q);
        st4(as + ii * H + 4 * q, a[0]);
      }
    } else {
      a[0] = ld4(as + ii * H + 4 * q);
    }
    const float rstd = ln_fwd<1>(a);
    f4 a1, a2, o;
    ff_fwd<1>(w, a, lane, a1, a2, o);
    if constexpr (!BWD) {
      if (valid) {
        if (node_res) o += ld4(x + ii * H + 4 * q);
        st4(xnext + ii * H + 4 * q, o);
      }
    } else {
      __syncthreads();
      st4(tIn + it * 16 + 4 * q, a[0]);
      const f4 d = valid ? ld4(dxn + ii * H + 4 * q) : zero4();
      f4 din[1];
      ff_bwd<1, true>(w, tIn, tD, tH, a1, a2, d, lane, G, din);
      ln_bwd<1>(a, rstd, din);
      if (valid) st4(da + ii * H + 4 * q, din[0]);
      if ((++done & (kFlush - 1)) == 0) G.flush(gacc, lane);
    }
  }
  if constexpr (BWD) {
    G.flush(gacc, lane);
    store_block(part + int64_t(blockIdx.x) * FFG, gacc, FFG, lane);
  }
}

// ---------------------------------------------------------------------------
// Decoder backward over CSC slots: out_e = FF_dec([e_k, x[src], x[dst]]), e = perm[k];
// gout [E, OUT] in edge order -> de_k, dfs_k, dfd_k and the parameter partials
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_dec_bwd(int64_t E, const float* __restrict__ wdec, int nout,
                                                const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                const int32_t* __restrict__ perm, const float* __restrict__ x,
                                                const float* __restrict__ e, const float* __restrict__ gout,
                                                float* __restrict__ de, float* __restrict__ dfd,
                                                float* __restrict__ dfs, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float w[FFL<3>::SIZE];
  __shared__ __attribute__((aligned(16))) float tIn[16 * 48], tD[256], tH[256];
  __shared__ double gacc[FFG];
  const int lane = threadIdx.x, it = lane & 15, q = lane >> 4;
  load_ff<3>(w, wdec, 3 * H, nout, nullptr, lane);
  clear_block(gacc, FFG, lane);
  int done = 0;
  __syncthreads();
  Acc<3> G;
  G.zero();
  const int64_t ntiles = (E + 15) / 16;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t k = t * 16 + it;
    const bool valid = k < E;
    const int64_t kk = valid ? k : E - 1;
    const f4 f[3] = {ld4(e + kk * H + 4 * q), ld4(x + int64_t(src[kk]) * H + 4 * q),
                     ld4(x + int64_t(dst[kk]) * H + 4 * q)};
    const int64_t oe = perm[kk];
    float c[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = (valid && 4 * q + r < nout) ? gout[oe * nout + 4 * q + r] : 0.f;
    f4 a1, a2, o, d[3];
    ff_fwd<3>(w, f, lane, a1, a2, o);
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 3; ++b) st4(tIn + it * 48 + 16 * b + 4 * q, f[b]);
    ff_bwd<3, true>(w, tIn, tD, tH, a1, a2, f4{c[0], c[1], c[2], c[3]}, lane, G, d);
    if (valid) {
      st4(de + kk * H + 4 * q, d[0]);
      st4(dfs + kk * H + 4 * q, d[1]);
      st4(dfd + kk * H + 4 * q, d[2]);
    }
    if ((++done & (kFlush - 1)) == 0) G.flush(gacc, lane);
  }
  G.flush(gacc, lane);
  store_block(part + int64_t(blockIdx.x) * FFG, gacc, FFG, lane);
}

// dx_i = [res] dxn_i + sum over CSC row i of dfd + sum over the slots with source i of dfs
// (sslot[sptr[i] .. sptr[i+1]), ascending): two row sums in fixed order; 4 threads per node
__global__ void __launch_bounds__(256) k_gather(int64_t N, const int32_t* __restrict__ ptr,
                                                const int32_t* __restrict__ sptr, const int32_t* __restrict__ sslot,
                                                const float* __restrict__ dxn, const float* __restrict__ dfd,
                                                const float* __restrict__ dfs, float* __restrict__ dx) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t i = t >> 2;
  const int q = int(t & 3);
  if (i >= N) return;
  f4 s = dxn ? ld4(dxn + i * H + 4 * q) : zero4();
  for (int k = ptr[i], k1 = ptr[i + 1]; k < k1; ++k) s += ld4(dfd + int64_t(k) * H + 4 * q);
  for (int j = sptr[i], j1 = sptr[i + 1]; j < j1; ++j) s += ld4(dfs + int64_t(sslot[j]) * H + 4 * q);
  st4(dx + i * H + 4 * q, s);
}

// out[entry] = sum over the P partial blocks, in double, fixed order: 4 contiguous slices of the
// blocks summed sequentially, then ((s0 + s1) + s2) + s3
__global__ void __launch_bounds__(256) k_reduce(const double* __restrict__ part, int P, int size,
                                                double* __restrict__ out) {
  __shared__ double sh[4][64];
  const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int entry = blockIdx.x * 64 + c;
  const int p0 = int(int64_t(P) * sl / 4), p1 = int(int64_t(P) * (sl + 1) / 4);
  double s = 0.0;
  if (entry < size)
    for (int p = p0; p < p1; ++p) s += part[int64_t(p) * size + entry];
  sh[sl][c] = s;
  __syncthreads();
  if (sl == 0 && entry < size) out[entry] = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
}

// One workgroup per FeedForward (blob order): the double sums of the folded gradients -> the
// packed fp32 gradient blob.  With a LayerNorm in front (W1' = W1 diag(gamma), b1' = b1 + W1 beta):
// dW1 = dW1' diag(gamma) + db1' (x) beta, dgamma_f = sum_u dW1'_uf W1_uf, dbeta_f = sum_u db1'_u W1_uf.
__global__ void __launch_bounds__(256) k_unfold(int node_in, int edge_in, int nlayers, int edge_out,
                                                const double* __restrict__ gsum, const float* __restrict__ wts,
                                                float* __restrict__ gw) {
  const FFBlock B = gnn_ff_block(node_in, edge_in, nlayers, edge_out, blockIdx.x);
  const int in = B.in, out = B.out;
  const bool ln = B.ln;
  const int64_t off = B.off;
  const double* G = gsum + int64_t(blockIdx.x) * FFG;
  const int lnsz = ln ? 2 * in : 0;
  const float* gam = wts + off;
  const float* W1 = wts + off + lnsz;
  float* o = gw + off + lnsz;
  for (int idx = threadIdx.x; idx < H * in; idx += 256) {
    const int u = idx / in, f = idx % in;
    double g = G[gW1 + u * 48 + f];
    if (ln) g = g * double(gam[f]) + G[gB1 + u] * double(gam[in + f]);
    o[idx] = float(g);
  }
  o += H * in;
  for (int idx = threadIdx.x; idx < H; idx += 256) o[idx] = float(G[gB1 + idx]);
  o += H;
  for (int idx = threadIdx.x; idx < H * H; idx += 256) o[idx] = float(G[gW2 + idx]);
  o += H * H;
  for (int idx = threadIdx.x; idx < H; idx += 256) o[idx] = float(G[gB2 + idx]);
  o += H;
  for (int idx = threadIdx.x; idx < out * H; idx += 256) o[idx] = float(G[gW3 + idx]);
  o += out * H;
  for (int idx = threadIdx.x; idx < out; idx += 256) o[idx] = float(G[gB3 + idx]);
  if (ln)
    for (int f = threadIdx.x; f < in; f += 256) {
      double dg = 0.0, db = 0.0;
      for (int u = 0; u < H; ++u) {
        const double w = double(W1[u * in + f]);
        dg += G[gW1 + u * 48 + f] * w;
        db += G[gB1 + u] * w;
      }
      gw[off + f] = float(dg);
      gw[off + in + f] = float(db);
    }
}

// ---- slots ordered by source node (generic path): count, scan, fill, per-node sort ----
__global__ void k_bysrc_count(int64_t E, const int32_t* __restrict__ src, int32_t* __restrict__ cnt) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < E; k += int64_t(gridDim.x) * blockDim.x)
    atomicAdd(&cnt[src[k]], 1);
}
__global__ void k_bysrc_fill(int64_t E, const int32_t* __restrict__ src, const int32_t* __restrict__ sptr,
                             int32_t* __restrict__ fill, int32_t* __restrict__ sslot) {
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < E; k += int64_t(gridDim.x) * blockDim.x) {
    const int32_t s = src[k];
    sslot[sptr[s] + atomicAdd(&fill[s], 1)] = int32_t(k);
  }
}
__global__ void k_bysrc_sort(int64_t N, const int32_t* __restrict__ sptr, int32_t* __restrict__ sslot) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t b = sptr[i], e = sptr[i + 1];
    for (int32_t k = b + 1; k < e; ++k) {
      const int32_t v = sslot[k];
      int32_t m = k - 1;
      while (m >= b && sslot[m] > v) {
        sslot[m + 1] = sslot[m];
        --m;
      }
      sslot[m + 1] = v;
    }
  }
}

int grid_for(int64_t items) {
  const int64_t t = (items + 15) / 16;
  return int(t < 1 ? 1 : (t > kMaxGrid ? kMaxGrid : t));
}
template <bool BWD, typename... A>
void launch_enc(int fin, int grid, hipStream_t st, A... args) {  // one 16-wide input block, or two (fin <= 32)
  launch(fin <= 16 ? k_enc<1, BWD> : k_enc<2, BWD>, dim3(grid), dim3(64), st, args...);
}

int bwd_reserve(lspcg_gnn* g, int64_t N, int64_t E) {
  lspcg_gnn_bwd_ws& w = g->bw;
  if (N <= w.capN && E <= w.capE) return LSPCG_OK;
  lspcg_gnn_bwd_free(g);
  const int64_t L = g->d.num_mp_layers;
  const size_t n = size_t(N) * H * sizeof(float), e = size_t(E) * H * sizeof(float);
  LSPCG_HIP(hipMalloc(&w.xs, n * (L + 1)));
  LSPCG_HIP(hipMalloc(&w.es, e * (L + 1)));
  LSPCG_HIP(hipMalloc(&w.as, n * (L > 0 ? L : 1)));
  LSPCG_HIP(hipMalloc(&w.dxa, n));
  LSPCG_HIP(hipMalloc(&w.dxb, n));
  LSPCG_HIP(hipMalloc(&w.da, n));
  LSPCG_HIP(hipMalloc(&w.de, e));
  LSPCG_HIP(hipMalloc(&w.dfd, e));
  LSPCG_HIP(hipMalloc(&w.dfs, e));
  LSPCG_HIP(hipMalloc(&w.part, sizeof(double) * 2 * FFG * size_t(std::max(grid_for(N), grid_for(E)))));
  LSPCG_HIP(hipMalloc(&w.gsum, sizeof(double) * FFG * size_t(3 + 3 * L)));
  LSPCG_HIP(hipMalloc(&w.sptr, sizeof(int32_t) * size_t(N + 1)));
  LSPCG_HIP(hipMalloc(&w.scnt, sizeof(int32_t) * size_t(N + 1)));
  LSPCG_HIP(hipMalloc(&w.sslot, sizeof(int32_t) * size_t(E)));
  w.capN = N;
  w.capE = E;
  return LSPCG_OK;
}

// the by-source order of the slots for the generic path (once per analysed graph)
int bwd_bysrc(lspcg_gnn* g, int64_t N, int64_t E, const int64_t* edge_index) {
  lspcg_gnn_bwd_ws& w = g->bw;
  if (w.sei == edge_index && w.sN == N && w.sE == E) return LSPCG_OK;
  hipStream_t st = g->ctx->stream;
  LSPCG_HIP(hipMemsetAsync(w.scnt, 0, sizeof(int32_t) * (N + 1), st));
  launch(k_bysrc_count, dim3(egrid(E)), dim3(256), st, E, g->src, w.scnt);
  size_t tb = 0;
  LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, w.scnt, w.sptr, int(N + 1), st));
  LSPCG_CHECK(tb <= g->scan_bytes || tb <= 1, LSPCG_ERR_HIP, "gnn_backward: scan workspace too small");
  tb = g->scan_bytes ? g->scan_bytes : 1;
  LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(g->scan_tmp, tb, w.scnt, w.sptr, int(N + 1), st));
  LSPCG_HIP(hipMemsetAsync(w.scnt, 0, sizeof(int32_t) * (N + 1), st));
  launch(k_bysrc_fill, dim3(egrid(E)), dim3(256), st, E, g->src, w.sptr, w.scnt, w.sslot);
  launch(k_bysrc_sort, dim3(egrid(N)), dim3(256), st, N, w.sptr, w.sslot);
  LSPCG_HIP(hipGetLastError());
  w.sei = edge_index;
  w.sN = N;
  w.sE = E;
  return LSPCG_OK;
}

int reduce_into(lspcg_gnn* g, int P, int size, int ff_index) {
  launch(k_reduce, dim3((size + 63) / 64), dim3(256), g->ctx->stream, g->bw.part, P, size,
         g->bw.gsum + int64_t(ff_index) * FFG);
  return LSPCG_OK;
}

}  // namespace
}  // namespace lspcg

using namespace lspcg;

void lspcg_gnn_bwd_free(lspcg_gnn* g) {
  lspcg_gnn_bwd_ws& w = g->bw;
  for (void* p : {(void*)w.xs, (void*)w.es, (void*)w.as, (void*)w.dxa, (void*)w.dxb, (void*)w.da, (void*)w.de,
                  (void*)w.dfd, (void*)w.dfs, (void*)w.part, (void*)w.gsum, (void*)w.sptr, (void*)w.sslot,
                  (void*)w.scnt})
    (void)hipFree(p);
  w = lspcg_gnn_bwd_ws{};
}

extern "C" int lspcg_gnn_backward(lspcg_gnn* g, int64_t N, int64_t E, const float* x, const int64_t* edge_index,
                                  const float* edge_attr, const float* grad_out, float* grad_weights) {
  LSPCG_CHECK(g && grad_weights && (N == 0 || x) && (E == 0 || (edge_index && edge_attr && grad_out)), LSPCG_ERR_ARG,
              "gnn_backward: NULL argument");
  LSPCG_CHECK(N >= 0 && E >= 0 && N < (int64_t(1) << 31) && E < (int64_t(1) << 31), LSPCG_ERR_ARG,
              "gnn_backward: sizes out of range");
  LSPCG_HIP(hipSetDevice(g->ctx->device));
  hipStream_t st = g->ctx->stream;
  if (E == 0 || N == 0) {  // no output, no gradient
    LSPCG_HIP(hipMemsetAsync(grad_weights, 0, sizeof(float) * g->nweights, st));
    return LSPCG_OK;
  }
  if (!(g->gei == edge_index && g->gN == N && g->gE == E && N <= g->capN && E <= g->capE))
    if (int rc = lspcg_gnn_build_csc(g, N, E, edge_index)) return rc;
  if (int rc = bwd_reserve(g, N, E)) return rc;
  lspcg_gnn_bwd_ws& w = g->bw;
  const lspcg_gnn_desc& d = g->d;
  const int L = d.num_mp_layers;
  const int32_t *sptr = g->ptr, *sslot = g->perm;  // symmetric path: the slots with source i are perm[row i]
  if (g->gflag) {
    if (int rc = bwd_bysrc(g, N, E, edge_index)) return rc;
    sptr = w.sptr;
    sslot = w.sslot;
  }
  const int gN = grid_for(N), gE = grid_for(E);
  const int64_t nN = N * H, nE = E * H;
  const float* wts = g->wdev;
  auto blob_at = [&](int b) { return wts + gnn_ff_block(d, b).off; };  // FeedForward b of the packed weights
  const float *w_nenc = blob_at(0), *w_eenc = blob_at(1), *w_dec = blob_at(gnn_ff_dec(L));
  LSPCG_HIP(hipMemsetAsync(w.gsum, 0, sizeof(double) * FFG * size_t(gnn_ff_count(L)), st));

  // ---- training forward: x_0, e_0, then per layer msg -> a_l, x_{l+1}, e_{l+1}
  launch_enc<false>(d.node_in, gN, st, N, w_nenc, d.node_in, x, nullptr, w.xs, nullptr, nullptr);
  launch_enc<false>(d.edge_in, gE, st, E, w_eenc, d.edge_in, edge_attr, g->perm, w.es, nullptr, nullptr);
  for (int l = 0; l < L; ++l) {
    const float* wl = blob_at(gnn_ff_index(l, kFFNode));  // the layer's [node | edge | msg]
    launch(k_edge_layer<false>, dim3(gE), dim3(64), st, E, wl, d.edge_residual, g->src, g->dst, w.xs + nN * l,
           w.es + nE * l, w.es + nE * (l + 1), w.dfd, nullptr, nullptr, nullptr, nullptr, nullptr);
    launch(k_node_layer<false>, dim3(gN), dim3(64), st, N, wl, d.node_residual, g->ptr, w.dfd, w.xs + nN * l,
           w.as + nN * l, w.xs + nN * (l + 1), nullptr, nullptr, nullptr);
  }

  // ---- decoder
  launch(k_dec_bwd, dim3(gE), dim3(64), st, E, w_dec, d.edge_out, g->src, g->dst, g->perm, w.xs + nN * L,
         w.es + nE * L, grad_out, w.de, w.dfd, w.dfs, w.part);
  reduce_into(g, gE, FFG, gnn_ff_dec(L));
  float* dx = w.dxa;
  float* dx2 = w.dxb;
  const unsigned gg = unsigned((N * 4 + 255) / 256);
  launch(k_gather, dim3(gg), dim3(256), st, N, g->ptr, sptr, sslot, nullptr, w.dfd, w.dfs, dx);
  // ---- layers in reverse
  for (int l = L - 1; l >= 0; --l) {
    const float* wl = blob_at(gnn_ff_index(l, kFFNode));
    launch(k_node_layer<true>, dim3(gN), dim3(64), st, N, wl, d.node_residual, g->ptr, nullptr, nullptr,
           w.as + nN * l, nullptr, dx, w.da, w.part);
    reduce_into(g, gN, FFG, gnn_ff_index(l, kFFNode));
    launch(k_edge_layer<true>, dim3(gE), dim3(64), st, E, wl, d.edge_residual, g->src, g->dst, w.xs + nN * l,
           w.es + nE * l, nullptr, nullptr, w.da, w.de, w.dfd, w.dfs, w.part);
    static_assert(kFFMsg == kFFEdge + 1, "k_edge_layer's partial block is [edge | msg], two neighbours of gsum");
    reduce_into(g, gE, 2 * FFG, gnn_ff_index(l, kFFEdge));
    launch(k_gather, dim3(gg), dim3(256), st, N, g->ptr, sptr, sslot, d.node_residual ? dx : nullptr, w.dfd, w.dfs,
           dx2);
    std::swap(dx, dx2);
  }
  // ---- encoders
  launch_enc<true>(d.node_in, gN, st, N, w_nenc, d.node_in, x, nullptr, nullptr, dx, w.part);
  reduce_into(g, gN, FFG, 0);
  launch_enc<true>(d.edge_in, gE, st, E, w_eenc, d.edge_in, edge_attr, g->perm, nullptr, w.de, w.part);
  reduce_into(g, gE, FFG, 1);
  launch(k_unfold, dim3(gnn_ff_count(L)), dim3(256), st, d.node_in, d.edge_in, L, d.edge_out, w.gsum, wts,
         grad_weights);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}
