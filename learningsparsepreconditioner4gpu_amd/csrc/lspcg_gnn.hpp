// State of a GNN handle and the layout of its packed weight blob, shared by the forward
// (lspcg_gnn.hip), the fragment packer (lspcg_gnn_pack.hpp) and the backward (lspcg_gnn_bwd.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "lspcg_internal.hpp"

namespace lspcg {

constexpr int H = 16;  // hidden = node_features = edge_features

using f4 = float __attribute__((ext_vector_type(4)));

// The packed weight blob (nn.py's _packed_params states the same order for Python): FeedForward b
// is 0 node_enc, 1 edge_enc, gnn_ff_index(l, kFFNode / kFFEdge / kFFMsg) in layer l, gnn_ff_dec(L)
// edge_dec.  A FeedForward(in, out, hidden = 16, num_layers = 2) is
//   [W1 (16 x in) | b1 (16) | W2 (16 x 16) | b2 (16) | W3 (out x 16) | b3 (out)],
// with its LayerNorm [gamma (in) | beta (in)] in front when `ln` (the three MLPs of a layer).
enum : int { kFFNode = 0, kFFEdge = 1, kFFMsg = 2 };
constexpr int gnn_ff_index(int l, int r) { return 2 + 3 * l + r; }
constexpr int gnn_ff_dec(int nlayers) { return 2 + 3 * nlayers; }
constexpr int gnn_ff_count(int nlayers) { return 3 + 3 * nlayers; }

struct FFBlock {
  int64_t off;  // first float of the block (the LayerNorm's gamma when ln)
  int in, out;
  bool ln;
  __host__ __device__ constexpr int64_t w1() const { return off + (ln ? 2 * in : 0); }  // first float of W1
};

// Block b of the blob of a descriptor (node_in, edge_in, num_mp_layers, edge_out); b = gnn_ff_count:
// off = the blob's size.
__host__ __device__ constexpr FFBlock gnn_ff_block(int node_in, int edge_in, int nlayers, int edge_out, int b) {
  auto ff_size = [](int in, int out, bool ln) {
    return int64_t((ln ? 2 * in : 0) + H * in + H + H * H + H + out * H + out);
  };
  const int64_t nenc = ff_size(node_in, H, false), enc = nenc + ff_size(edge_in, H, false);
  const int64_t node = ff_size(H, H, true), edge = ff_size(3 * H, H, true);  // msg: as edge
  const int64_t dec = enc + (node + 2 * edge) * nlayers;
  if (b == 0) return {0, node_in, H, false};
  if (b == 1) return {nenc, edge_in, H, false};
  if (b == gnn_ff_dec(nlayers)) return {dec, 3 * H, edge_out, false};
  if (b > gnn_ff_dec(nlayers)) return {dec + ff_size(3 * H, edge_out, false), 0, 0, false};
  const int l = (b - 2) / 3, r = (b - 2) % 3;
  return {enc + (node + 2 * edge) * l + (r > kFFNode ? node : 0) + (r > kFFEdge ? edge : 0), r == kFFNode ? H : 3 * H,
          H, true};
}
// FeedForward r of a layer, from the layer's first float
constexpr int gnn_layer_off(int r) {
  return int(gnn_ff_block(1, 1, 1, 1, gnn_ff_index(0, r)).off - gnn_ff_block(1, 1, 1, 1, gnn_ff_index(0, kFFNode)).off);
}
inline FFBlock gnn_ff_block(const lspcg_gnn_desc& d, int b) {
  return gnn_ff_block(d.node_in, d.edge_in, d.num_mp_layers, d.edge_out, b);
}

// Offsets of the fragment blocks in the device fragment blob (pack_fragments, lspcg_gnn_pack.hpp)
struct FragOffsets {
  int64_t node_enc = 0, edge_enc = 0, dec = 0;
  int64_t edge_enc_h = 0;      // split-f16 block of the edge encoder (the first layer's fused copy)
  std::vector<int64_t> layer;  // per layer: [msg | edge | node] fragment block
};

inline int egrid(int64_t n) {  // kThreads items per workgroup
  const int64_t g = (n + kThreads - 1) / kThreads;
  return int(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

}  // namespace lspcg

// Workspace of lspcg_gnn_backward (grown on first use; lspcg_gnn_bwd.hip)
struct lspcg_gnn_bwd_ws {
  int64_t capN = -1, capE = -1;
  float* xs = nullptr;   // node states x_0 .. x_L        [(L+1) N 16]
  float* es = nullptr;   // edge states e_0 .. e_L, CSC   [(L+1) E 16]
  float* as = nullptr;   // aggregated messages a_0..a_L-1 [L N 16]
  float *dxa = nullptr, *dxb = nullptr, *da = nullptr;  // [N 16]
  float *de = nullptr, *dfd = nullptr, *dfs = nullptr;  // [E 16]
  double* part = nullptr;  // per-workgroup parameter-gradient partials of one launch
  double* gsum = nullptr;  // reduced partials, padded per FeedForward
  // slots ordered by source node (generic path; the symmetric path uses ptr / perm)
  int32_t *sptr = nullptr, *sslot = nullptr, *scnt = nullptr;
  const int64_t* sei = nullptr;  // the graph sptr / sslot were built for
  int64_t sN = -1, sE = -1;
};

struct lspcg_gnn {
  lspcg_ctx* ctx = nullptr;
  lspcg_gnn_desc d{};
  float* frag = nullptr;  // device fragment blob
  int64_t frag_cap = 0;   // floats allocated at frag
  float* wdev = nullptr;  // the packed weights as given (unfolded), for the backward
  int64_t nweights = 0;
  lspcg::FragOffsets o;   // where the kernels' fragment blocks start in frag
  bool f32 = false;          // fp32-MFMA kernels (weights past the split-f16 range, or LSPCG_GNN_F32=1)
  double hidden_bound = 0;   // largest hidden-activation bound over the layers (what chose f32)
  // workspace
  int64_t capN = -1, capE = -1;
  float *xa = nullptr, *xb = nullptr, *ecsc = nullptr;
  int32_t *ptr = nullptr, *cnt = nullptr, *perm = nullptr, *inv = nullptr, *src = nullptr, *dst = nullptr;
  int* flag = nullptr;
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  // the CSC of the last graph (lspcg_gnn_set_graph): reused while forward gets the same
  // (edge_index pointer, N, E); gflag != 0: the generic (unsorted / asymmetric) path built it
  const int64_t* gei = nullptr;
  int64_t gN = -1, gE = -1;
  int gflag = 0;
  lspcg_gnn_bwd_ws bw;
};

inline int64_t gnn_weight_count(const lspcg_gnn_desc& d) {
  return lspcg::gnn_ff_block(d, lspcg::gnn_ff_count(d.num_mp_layers)).off;
}

// lspcg_gnn.hip: the CSC of a graph (lspcg_gnn_set_graph); lspcg_gnn_bwd.hip: frees the backward workspace
int lspcg_gnn_build_csc(lspcg_gnn* g, int64_t N, int64_t E, const int64_t* edge_index);
void lspcg_gnn_bwd_free(lspcg_gnn* g);
