// Host side of the GNN's weights: the packed blob (lspcg_gnn.hpp) -> the fragment blob the forward
// kernels read.  Pure host code on std::vector<float> (no HIP runtime calls); the sizes and offsets
// of the fragment blocks below are the ones the kernels of lspcg_gnn.hip index with, and every
// emitted block is checked against them (pack_fragments).
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <vector>

#include "lspcg_gnn.hpp"

namespace lspcg {

// Fragment block of one FeedForward (floats): [A1 (S1 x 64) | C1 (64 x 4) | A2 (4 x 64) |
// C2 (64 x 4) | A3 (4 x 64) | C3 (64 x 4)]
__host__ __device__ constexpr int frag_size(int s1) { return s1 * 64 + 5 * 256; }

// f16 block of one FeedForward(48 -> 16 -> 16 -> out) (dwords, 64 lanes): [W1 hi, K block 0 / 1 / 2
// (2 dwords = 4 halves per lane each) | W1 lo, blocks 0 / 1 / 2 | C1 (4 floats / lane) | W2 hi | W2 lo |
// C2 | W3 hi | W3 lo | C3 | 2^-s1, 2^-s2, 2^-s3, pad].  Every product is a v_mfma_f32_16x16x16f16:
// K slot (q, j) of block i is the lane's in[4i + j] (feature 16i + 4q + j, as feat48); C = 2^s b in
// accumulator layout.  (v_mfma_f32_16x16x32_f16 -- one instruction for blocks 0 and 1 -- lost its
// operands: hipcc reused its A / B registers for VALU results right after issue, and the products
// went missing in the edge decoder; 16x16x16 has no such hazard gap.)
constexpr int kH48 = 2052;
constexpr int kH48W1h = 0, kH48W1l = 384, kH48C1 = 768;
constexpr int kH48W2h = 1024, kH48W2l = 1152, kH48C2 = 1280, kH48W3h = 1536, kH48W3l = 1664, kH48C3 = 1792;
constexpr int kH48S = 2048;
// FeedForward(16 -> 16 -> 16 -> 16) (the node MLP) on split operands: block [W1 hi | W1 lo | C1 | W2 hi |
// W2 lo | C2 | W3 hi | W3 lo | C3 | 2^-s1..3, pad | the encoder's magnitude bounds B1, c1, B2, c2
// (ff1_16_enc)] (kH16 dwords; K slot (q, j) = the lane's in[j], i.e.
// feature 4q + j, as feat16); us = its 2^-s factors
constexpr int kH16 = 1548;
constexpr int kH16S = 1536;

struct FF {  // views into the packed (reference-layout) blob
  const float *W1, *b1, *W2, *b2, *W3, *b3;
  const float *gamma, *beta;  // the LayerNorm in front, or null
  int in, out;
};
inline FF ff_at(const float* w, const FFBlock& b) {
  FF f;
  f.in = b.in;
  f.out = b.out;
  f.gamma = b.ln ? w + b.off : nullptr;
  f.beta = b.ln ? w + b.off + b.in : nullptr;
  f.W1 = w + b.w1();
  f.b1 = f.W1 + H * b.in;
  f.W2 = f.b1 + H;
  f.b2 = f.W2 + H * H;
  f.W3 = f.b2 + H;
  f.b3 = f.W3 + b.out * H;
  return f;
}

// Layer 1 with the LayerNorm affine folded in, in double: W1' = W1 diag(gamma), b1' = b1 + W1 beta
struct Folded {
  std::vector<double> W1;  // [16][in]
  double b1[H];
};
inline Folded fold_layer1(const FF& f) {
  Folded r;
  r.W1.resize(size_t(H) * f.in);
  for (int i = 0; i < H; ++i) {
    double bb = f.b1[i];
    for (int k = 0; k < f.in; ++k) {
      const double w = f.W1[i * f.in + k];
      r.W1[i * f.in + k] = f.gamma ? w * f.gamma[k] : w;
      if (f.beta) bb += w * f.beta[k];
    }
    r.b1[i] = bb;
  }
  return r;
}

// s with max |W| 2^s in [2^10, 2^11) (the split-f16 weights' power-of-two scale: low halves stay normal f16)
inline int scale_exp(double mx) {
  if (mx == 0) return 0;
  int e;
  std::frexp(mx, &e);  // mx in [2^(e-1), 2^e)
  return 11 - e;
}

inline int feat48(int s, int q) { return (s >> 2) * 16 + 4 * q + (s & 3); }
inline int feat16(int s, int q) { return 4 * q + s; }
inline int featenc(int s, int q) { return 4 * s + q; }

// Append the f32 fragment block of `f` (frag_size(s1) floats).  feat(s, q) = input feature in K slot q
// of step s (-1 = zero).  Returns the floats appended.
inline size_t emit_frag(std::vector<float>& o, const FF& f, const Folded& l1, int s1, int (*feat)(int, int)) {
  const size_t start = o.size();
  for (int s = 0; s < s1; ++s)
    for (int l = 0; l < 64; ++l) {
      const int fi = feat(s, l >> 4);
      o.push_back(fi >= 0 && fi < f.in ? float(l1.W1[(l & 15) * f.in + fi]) : 0.f);
    }
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) o.push_back(float(l1.b1[4 * (l >> 4) + r]));
  for (int s = 0; s < 4; ++s)
    for (int l = 0; l < 64; ++l) o.push_back(f.W2[(l & 15) * H + 4 * (l >> 4) + s]);
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) o.push_back(f.b2[4 * (l >> 4) + r]);
  for (int s = 0; s < 4; ++s)
    for (int l = 0; l < 64; ++l) {
      const int i = l & 15;
      o.push_back(i < f.out ? f.W3[i * H + 4 * (l >> 4) + s] : 0.f);
    }
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * (l >> 4) + r;
      o.push_back(i < f.out ? f.b3[i] : 0.f);
    }
  return o.size() - start;
}

// Append the split-f16 block of `f`: in48, a FeedForward(48 -> 16 -> 16 -> out) (ff2_48 / ff1_48; kH48
// dwords), else one with <= 16 inputs (ff1_16 / ff1_16_enc; kH16 dwords).  Weights scaled by 2^s per
// matrix (scale_exp), split into RNE f16 pairs.  Returns the floats appended.
inline size_t emit_frag_h(std::vector<float>& o, const FF& f, const Folded& l1, bool in48) {
  const size_t start = o.size();
  std::vector<float> W1(l1.W1.begin(), l1.W1.end());
  float b1[H];
  for (int i = 0; i < H; ++i) b1[i] = float(l1.b1[i]);
  auto absmax = [](auto get, int rows, int cols) {
    double mx = 0;
    for (int i = 0; i < rows; ++i)
      for (int k = 0; k < cols; ++k) mx = std::max(mx, std::fabs(double(get(i, k))));
    return mx;
  };
  auto w1 = [&](int i, int k) { return k < f.in ? W1[i * f.in + k] : 0.f; };  // 16-slot blocks pad fin < 16
  auto w2 = [&](int i, int k) { return f.W2[i * H + k]; };
  auto w3 = [&](int i, int k) { return i < f.out ? f.W3[i * H + k] : 0.f; };
  const int s1 = scale_exp(absmax(w1, H, f.in)), s2 = scale_exp(absmax(w2, H, H)), s3 = scale_exp(absmax(w3, H, H));
  auto push_pairs = [&](auto get, int s, auto kidx, bool lo) {  // per lane: 4 halves
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 4; j += 2) {
        unsigned u = 0;
        for (int t = 0; t < 2; ++t) {
          const int k = kidx(l >> 4, j + t);
          const float x = k >= 0 ? std::ldexp(get(l & 15, k), s) : 0.f;
          const _Float16 h = static_cast<_Float16>(x);
          const _Float16 v = lo ? static_cast<_Float16>(x - static_cast<float>(h)) : h;
          u |= unsigned(__builtin_bit_cast(unsigned short, v)) << (16 * t);
        }
        o.push_back(__builtin_bit_cast(float, u));
      }
  };
  auto push_bias = [&](auto get, int s) {
    for (int l = 0; l < 64; ++l)
      for (int r = 0; r < 4; ++r) o.push_back(std::ldexp(get(4 * (l >> 4) + r), s));
  };
  auto kh = [](int q, int j) { return 4 * q + j; };  // 16-wide inputs / hidden layers: K slot (q, j) = feature 4q + j
  for (bool lo : {false, true}) {
    if (in48)  // three K blocks of 16: block i, slot (q, j) = feature 16 i + 4 q + j = feat48(4 i + j, q)
      for (int i = 0; i < 3; ++i) push_pairs(w1, s1, [i](int q, int j) { return feat48(4 * i + j, q); }, lo);
    else  // <= 16 inputs: one 16x16x16 product
      push_pairs(w1, s1, kh, lo);
  }
  push_bias([&](int i) { return b1[i]; }, s1);
  push_pairs(w2, s2, kh, false);
  push_pairs(w2, s2, kh, true);
  push_bias([&](int i) { return f.b2[i]; }, s2);
  push_pairs(w3, s3, kh, false);
  push_pairs(w3, s3, kh, true);
  push_bias([&](int i) { return i < f.out ? f.b3[i] : 0.f; }, s3);
  for (int s : {s1, s2, s3}) o.push_back(std::ldexp(1.0f, -s));
  o.push_back(0.f);
  if (!in48) {  // magnitude bounds for ff1_16_enc: max row sum of |W|, max |bias| + GELU's 0.17
    auto rowsum = [](auto get, int rows, int cols) {
      double mx = 0;
      for (int i = 0; i < rows; ++i) {
        double r = 0;
        for (int k = 0; k < cols; ++k) r += std::fabs(double(get(i, k)));
        mx = std::max(mx, r);
      }
      return float(mx);
    };
    auto biasmax = [](const float* b) {
      double mx = 0;
      for (int i = 0; i < H; ++i) mx = std::max(mx, std::fabs(double(b[i])));
      return float(mx + 0.17);
    };
    const float B1 = rowsum(w1, H, f.in), c1 = biasmax(b1), B2 = rowsum(w2, H, H), c2 = biasmax(f.b2);
    // the largest edge maximum m with max(B1 m + c1, B2 (B1 m + c1) + c2) < 2^14 (no hidden scale);
    // half the device threshold, so the float rounding of the bounds cannot matter
    const double lim = 16384.0, h1 = std::min(lim, (lim - c2) / std::max(double(B2), 1e-30));
    const double ms = (h1 - c1) / std::max(double(B1), 1e-30);
    for (float v : {B1, c1, B2, c2, float(std::max(0.0, ms)), 0.f, 0.f, 0.f}) o.push_back(v);
  }
  return o.size() - start;
}

// What decides fp32 for a LayerNorm-fed FeedForward, in one pass over its three matrices.
//  hidden: the largest |hidden activation| it can produce.  LayerNorm outputs are at most sqrt(n - 1)
//   in magnitude (gamma / beta folded into layer 1), |GELU(z)| <= max(|z|, 0.17), so |h1| <= ||W1'||_inf
//   sqrt(n - 1) + max |b1'| + 0.17 and |h2| <= ||W2||_inf |h1| + max |b2| + 0.17.  The split-f16 products
//   need it below 2^15 (f16 holds 65504).
//  scaled: the split-f16 GEMMs carry each layer's result scaled by 2^s (scale_exp); the last layer's
//   messages are summed over a node's edges while still scaled.  A matrix of tiny weights beside O(1)
//   biases (2^s large, the bias scaled alike) could push those scaled values past fp32's range, which the
//   per-message unscale never reached.  The largest scaled magnitude, 2^s x (|W| row bound x input bound
//   + max |bias|), over the three layers; fp32 runs when it exceeds 2^96, which leaves 2^32 for a node's
//   message sum.  (Seeded / trained weights: ~2^20.)
struct FFBounds {
  double hidden = 0, scaled = 0;
};
inline FFBounds ln_ff_bounds(const FF& f, const Folded& l1) {
  const double x1 = std::sqrt(double(f.in - 1));  // LayerNorm output bound
  double w1 = 0, w2 = 0, w3 = 0, r1 = 0, r2 = 0, r3 = 0, b1 = 0, b2 = 0, b3 = 0, hid1 = 0;
  for (int i = 0; i < H; ++i) {
    double r = 0;
    for (int k = 0; k < f.in; ++k) {
      w1 = std::max(w1, std::fabs(l1.W1[i * f.in + k]));
      r += std::fabs(l1.W1[i * f.in + k]);
    }
    r1 = std::max(r1, r);
    b1 = std::max(b1, std::fabs(l1.b1[i]));
    hid1 = std::max(hid1, r * x1 + std::fabs(l1.b1[i]) + 0.17);
    double q2 = 0, q3 = 0;
    for (int k = 0; k < H; ++k) {
      w2 = std::max(w2, std::fabs(double(f.W2[i * H + k])));
      q2 += std::fabs(double(f.W2[i * H + k]));
      if (i < f.out) {
        w3 = std::max(w3, std::fabs(double(f.W3[i * H + k])));
        q3 += std::fabs(double(f.W3[i * H + k]));
      }
    }
    r2 = std::max(r2, q2);
    r3 = std::max(r3, q3);
    b2 = std::max(b2, std::fabs(double(f.b2[i])));
    if (i < f.out) b3 = std::max(b3, std::fabs(double(f.b3[i])));
  }
  const double h1 = r1 * x1 + b1 + 0.17, h2 = r2 * h1 + b2 + 0.17;  // GELU outputs
  return {std::max(hid1, r2 * hid1 + b2 + 0.17),
          std::max({std::ldexp(r1 * x1 + b1, scale_exp(w1)), std::ldexp(r2 * h1 + b2, scale_exp(w2)),
                    std::ldexp(r3 * h2 + b3, scale_exp(w3))})};
}

struct Fragments {
  std::vector<float> blob;
  FragOffsets o;
  bool f32 = false;         // fp32-MFMA kernels: weights past the split-f16 range, or force_f32
  double hidden_bound = 0;  // largest FFBounds::hidden over the layers
};

// The fragment blob of the packed weights `w` (gnn_weight_count(d) floats).  The split-f16 GEMMs hold
// hidden activations below 2^15; weights whose LayerNorm-fed MLPs could exceed that (or force_f32) get
// the exact fp32-MFMA kernels' fragments instead (same results to ~1e-7, 1.2x slower).  A block whose
// size is not the constant the kernels index with would shift every later block: an error.
inline int pack_fragments(const lspcg_gnn_desc& d, const std::vector<float>& w, bool force_f32, Fragments* out) {
  const int L = d.num_mp_layers;
  std::vector<FF> ff;
  std::vector<Folded> l1;
  for (int b = 0; b < gnn_ff_count(L); ++b) {
    ff.push_back(ff_at(w.data(), gnn_ff_block(d, b)));
    l1.push_back(fold_layer1(ff.back()));
  }
  double scaled = 0;
  out->hidden_bound = 0;
  for (int b = 2; b < gnn_ff_dec(L); ++b) {  // the layers' MLPs: the ones a LayerNorm feeds
    const FFBounds bd = ln_ff_bounds(ff[b], l1[b]);
    out->hidden_bound = std::max(out->hidden_bound, bd.hidden);
    scaled = std::max(scaled, bd.scaled);
  }
  const bool f32 = out->f32 = !(out->hidden_bound < 32768.0) || !(scaled <= std::ldexp(1.0, 96)) || force_f32;
  std::vector<float>& fr = out->blob;
  fr.clear();
  const char* bad = nullptr;  // the first block of the wrong size
  auto emit = [&](int b, int s1, int (*feat)(int, int), const char* what) {  // s1 = 0: the split-f16 block
    const bool in48 = ff[b].in == 3 * H;
    const size_t got = s1 ? emit_frag(fr, ff[b], l1[b], s1, feat) : emit_frag_h(fr, ff[b], l1[b], in48);
    if (got != size_t(s1 ? frag_size(s1) : in48 ? kH48 : kH16) && !bad) bad = what;
  };
  FragOffsets& o = out->o;
  o = FragOffsets{};
  emit(0, (d.node_in + 3) / 4, featenc, "node_enc");
  o.edge_enc = int64_t(fr.size());
  emit(1, (d.edge_in + 3) / 4, featenc, "edge_enc");
  for (int l = 0; l < L; ++l) {
    o.layer.push_back(int64_t(fr.size()));
    emit(gnn_ff_index(l, kFFMsg), f32 ? 12 : 0, feat48, "msg");
    emit(gnn_ff_index(l, kFFEdge), f32 ? 12 : 0, feat48, "edge");
    emit(gnn_ff_index(l, kFFNode), f32 ? 4 : 0, feat16, "node");
  }
  o.dec = int64_t(fr.size());
  emit(gnn_ff_dec(L), f32 ? 12 : 0, feat48, "edge_dec");
  if (!f32) {
    // read by the first layer's fused encoder (edge_in <= 12); emitted up to 16 inputs, one 16-wide K block
    o.edge_enc_h = int64_t(fr.size());
    if (d.edge_in <= 16) emit(1, 0, nullptr, "edge_enc (split-f16)");
  }
  LSPCG_CHECK(!bad, LSPCG_ERR_UNSUPPORTED,
              std::string("gnn: the ") + (bad ? bad : "") + " fragment block is not the size the kernels index with");
  return LSPCG_OK;
}

}  // namespace lspcg
