// lspcg_optim_step: gradient clipping and one optimizer step (SGD / Adam / AdamW) over a flat fp32
// parameter blob, as ONE launch of ONE workgroup.
//
// The SPAI GNN has ~17 k parameters (at most ~240 k at 64 message-passing layers): the job is bound
// by launch latency, not by bandwidth, and a single workgroup needs no cross-workgroup reduction --
// the two global norms are plain fixed-shape trees inside it.
//
//   phase 1  ‖grad_scale·grad‖ and ‖w‖: every thread sums the squares of its elements in double in
//            a fixed order, then a wave butterfly and a 16-entry LDS sum (no atomics: same bits)
//   phase 2  coef = min(1, clip_norm / (norm + 1e-6))  (torch.nn.utils.clip_grad_norm_), then
//            torch.optim's non-capturable single-tensor update per element, evaluated in double and
//            rounded once per stored value (w, m, v are fp32), and the sum of the new w²
//   phase 3  ‖w‖ after the step; thread 0 writes the four stats
//
// Element ownership: thread t owns the 4-element chunks t, t + W, t + 2W, ... of the blob, in both
// phases, so the in-place update of w never crosses threads.  A chunk is one 16-byte access when
// every pointer is 16-byte aligned and four scalar accesses otherwise; the owner and the order of
// every sum are the same either way, so the stats do not depend on the alignment.
#include "lspcg_internal.hpp"

#include <cmath>

namespace lspcg {
namespace {

constexpr int kOptThreads = 1024;  // one workgroup of 16 wave64
constexpr int kOptWaves = kOptThreads / 64;

struct OptArgs {
  int kind;
  int first;          // step == 1: SGD's momentum buffer starts as the gradient
  float grad_scale;
  double clip_norm;   // <= 0: no clipping
  double lr, beta1, beta2, eps, weight_decay, momentum;
  double step_size;   // Adam: lr / (1 - beta1^step)
  double bc2_sqrt;    // Adam: sqrt(1 - beta2^step)
};

struct Chunk {
  float a[4];
};

__device__ __forceinline__ Chunk load4(const float* p, int64_t i, int64_t n, bool vec) {
  Chunk c;
  if (vec && i + 4 <= n) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    c.a[0] = q.x, c.a[1] = q.y, c.a[2] = q.z, c.a[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) c.a[j] = i + j < n ? p[i + j] : 0.f;
  }
  return c;
}

__device__ __forceinline__ void store4(float* p, int64_t i, int64_t n, bool vec, const Chunk& c) {
  if (vec && i + 4 <= n) {
    *reinterpret_cast<float4*>(p + i) = make_float4(c.a[0], c.a[1], c.a[2], c.a[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = c.a[j];
  }
}

// Sum of NV doubles over the workgroup in a fixed shape; every thread returns with the totals.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*lds)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v[j] += __shfl_xor(v[j], m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) lds[threadIdx.x >> 6][j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double a = lds[0][j];
    for (int w = 1; w < kOptWaves; ++w) a += lds[w][j];
    v[j] = a;
  }
}

__global__ __launch_bounds__(kOptThreads) void k_optim_step(OptArgs o, int64_t n, float* __restrict__ w,
                                                             const float* __restrict__ grad, float* __restrict__ m,
                                                             float* __restrict__ v, double* __restrict__ stats,
                                                             int vec_) {
  __shared__ double lds1[kOptWaves][2];
  __shared__ double lds2[kOptWaves][1];
  const bool vec = vec_ != 0;
  const int64_t stride = int64_t(kOptThreads) * 4;
  const int64_t i0 = int64_t(threadIdx.x) * 4;

  // ---- phase 1: the two norms
  double s[2] = {0.0, 0.0};
  for (int64_t i = i0; i < n; i += stride) {
    const Chunk g = load4(grad, i, n, vec);
    const Chunk x = load4(w, i, n, vec);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double gj = double(o.grad_scale * g.a[j]);
      s[0] += gj * gj;
      s[1] += double(x.a[j]) * double(x.a[j]);
    }
  }
  block_sum<2>(s, lds1);  // its barrier also orders every read of w above before the writes below
  const double gnorm = sqrt(s[0]);
  const double wnorm = sqrt(s[1]);
  double coef = 1.0;
  if (o.clip_norm > 0.0) {
    const double c = o.clip_norm / (gnorm + 1e-6);
    coef = c > 1.0 ? 1.0 : c;  // a NaN norm gives a NaN coefficient, as torch.clamp does
  }

  // ---- phase 2: the update
  const bool adam = o.kind != LSPCG_OPT_SGD;
  const bool use_m = adam || o.momentum != 0.0;
  double s2[1] = {0.0};
  for (int64_t i = i0; i < n; i += stride) {
    const Chunk g4 = load4(grad, i, n, vec);
    Chunk x4 = load4(w, i, n, vec);
    Chunk m4 = {}, v4 = {};
    if (use_m && !(o.first && !adam)) m4 = load4(m, i, n, vec);
    if (adam) v4 = load4(v, i, n, vec);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double x = double(x4.a[j]);
      double g = double(o.grad_scale * g4.a[j]) * coef;
      if (adam) {
        if (o.kind == LSPCG_OPT_ADAMW) {
          x *= 1.0 - o.lr * o.weight_decay;
        } else if (o.weight_decay != 0.0) {
          g += o.weight_decay * x;
        }
        double mm = double(m4.a[j]);
        mm += (1.0 - o.beta1) * (g - mm);  // lerp
        const double vv = o.beta2 * double(v4.a[j]) + (1.0 - o.beta2) * g * g;
        m4.a[j] = float(mm);
        v4.a[j] = float(vv);
        // the stored (rounded) moments enter the update, as in torch
        x -= o.step_size * double(m4.a[j]) / (sqrt(double(v4.a[j])) / o.bc2_sqrt + o.eps);
      } else {
        if (o.weight_decay != 0.0) g += o.weight_decay * x;
        if (use_m) {
          const double b = o.first ? g : o.momentum * double(m4.a[j]) + g;
          m4.a[j] = float(b);
          g = double(m4.a[j]);
        }
        x -= o.lr * g;
      }
      x4.a[j] = float(x);
      if (i + j < n) s2[0] += double(x4.a[j]) * double(x4.a[j]);
    }
    store4(w, i, n, vec, x4);
    if (use_m) store4(m, i, n, vec, m4);
    if (adam) store4(v, i, n, vec, v4);
  }

  // ---- phase 3: ‖w‖ after the step, and the stats
  if (stats != nullptr) {
    block_sum<1>(s2, lds2);
    if (threadIdx.x == 0) {
      stats[0] = gnorm;
      stats[1] = coef;
      stats[2] = wnorm;
      stats[3] = sqrt(s2[0]);
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace lspcg

extern "C" int lspcg_optim_step(lspcg_ctx* ctx, const lspcg_optim_desc* desc, int64_t n, int64_t step, double lr,
                                float* w, const float* grad, float* m, float* v, double* stats) {
  using namespace lspcg;
  LSPCG_CHECK(ctx && desc, LSPCG_ERR_ARG, "optim_step: NULL argument");
  LSPCG_CHECK(n >= 0 && step >= 1, LSPCG_ERR_ARG, "optim_step: n must be >= 0 and step >= 1 (1-based)");
  const lspcg_optim_desc& d = *desc;
  LSPCG_CHECK(d.kind == LSPCG_OPT_SGD || d.kind == LSPCG_OPT_ADAM || d.kind == LSPCG_OPT_ADAMW, LSPCG_ERR_ARG,
              "optim_step: unknown optimizer kind " + std::to_string(d.kind));
  const bool adam = d.kind != LSPCG_OPT_SGD;
  if (n > 0) {
    LSPCG_CHECK(w && grad, LSPCG_ERR_ARG, "optim_step: NULL w or grad");
    LSPCG_CHECK(!adam || (m && v), LSPCG_ERR_ARG, "optim_step: Adam / AdamW need the m and v state");
    LSPCG_CHECK(adam || d.momentum == 0.0 || m, LSPCG_ERR_ARG, "optim_step: SGD with momentum needs the m state");
  }
  if (n == 0 && stats == nullptr) return LSPCG_OK;
  OptArgs o;
  o.kind = d.kind;
  o.first = step == 1;
  o.grad_scale = float(d.grad_scale);
  o.clip_norm = d.clip_norm;
  o.lr = lr;
  o.beta1 = d.beta1;
  o.beta2 = d.beta2;
  o.eps = d.eps;
  o.weight_decay = d.weight_decay;
  o.momentum = d.momentum;
  o.step_size = adam ? lr / (1.0 - std::pow(d.beta1, double(step))) : lr;
  o.bc2_sqrt = adam ? std::sqrt(1.0 - std::pow(d.beta2, double(step))) : 1.0;
  const bool use_m = adam || d.momentum != 0.0;
  const int vec = aligned16(w) && aligned16(grad) && (!use_m || aligned16(m)) && (!adam || aligned16(v));
  LSPCG_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_optim_step, dim3(1), dim3(kOptThreads), 0, ctx->stream, o, n, w, grad, m, v, stats, vec);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}
