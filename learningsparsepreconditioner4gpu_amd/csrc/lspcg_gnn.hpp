// State of a GNN handle, shared by the forward (lspcg_gnn.hip) and the backward
// (lspcg_gnn_bwd.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "lspcg_internal.hpp"

namespace lspcg {

constexpr int H = 16;  // hidden = node_features = edge_features

using f4 = float __attribute__((ext_vector_type(4)));

// FeedForward(in, out, hidden=16, num_layers=2) parameter block of the packed blob:
//   [W1 (16 x in) | b1 (16) | W2 (16 x 16) | b2 (16) | W3 (out x 16) | b3 (out)]
__host__ __device__ constexpr int ff_size(int in, int out) { return H * in + H + H * H + H + out * H + out; }

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
  int64_t o_node_enc = 0, o_edge_enc = 0, o_dec = 0;
  int64_t o_edge_enc_h = 0;  // split-f16 block of the edge encoder (the first layer's fused copy)
  bool f32 = false;          // fp32-MFMA kernels (weights past the split-f16 range, or LSPCG_GNN_F32=1)
  double hidden_bound = 0;   // largest ln_ff_hidden_bound over the layers (what chose f32)
  std::vector<int64_t> o_layer;  // per layer: [msg | edge | node] fragment block
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
  using lspcg::ff_size;
  using lspcg::H;
  int64_t n = ff_size(d.node_in, H) + ff_size(d.edge_in, H);
  n += int64_t(d.num_mp_layers) * ((2 * H + ff_size(H, H)) + 2 * (6 * H + ff_size(3 * H, H)));
  n += ff_size(3 * H, d.edge_out);
  return n;
}

// lspcg_gnn.hip: the CSC of a graph (lspcg_gnn_set_graph); lspcg_gnn_bwd.hip: frees the backward workspace
int lspcg_gnn_build_csc(lspcg_gnn* g, int64_t N, int64_t E, const int64_t* edge_index);
void lspcg_gnn_bwd_free(lspcg_gnn* g);
