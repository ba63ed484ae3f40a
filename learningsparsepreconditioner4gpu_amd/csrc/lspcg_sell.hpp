// Sliced-ELL (SELL-64) iteration view of a scalar CSR matrix, for the PCG loop.
//
// Why (DESIGN.md "SpMV formats"): in the staged CSR kernel one gather instruction covers the
// entries of ~17 consecutive rows at ~4 different stencil positions (~30 distinct cache lines),
// and every row tile pays a dependent rowptr load, an LDS round trip and two barriers.  In
// SELL-64 a wave owns a slice of 64 consecutive rows; entry k of row r is stored at
//     256*(gp[slice] + k/4) + 4*r + k%4
// so lane r loads 4 consecutive entries of ITS row with one 16-B load (values) and one 16-B
// load (columns), and one gather instruction reads x at the same in-row position of 64
// consecutive rows (~4 cache lines on banded FEM matrices).  The row sum stays in a register
// and is accumulated in the row's index order -- scipy's csr_matvec order, so results are
// bit-identical to the CSR kernels.  Padding slots (k >= row length) are skipped by a
// predicate, never added (0*inf and -0.0 + 0.0 must not leak into the sum).
//
// What is here: the layouts' constants and SellPattern; one kernel per layout -- k_spmv_sell
// (SELL-64, SELL-64C), k_spmv_sellj (SELL-64J / SELL-64X), k_spmv_bsell3 (BSELL-64), k_spmv_sdia
// (SELL-DIA), k_spmv_bsdia3 (BSELL-DIA); for solve_multi's K = 2, 4, 8 interleaved vectors
// k_spmv_sell takes K as its last template parameter and SELL-DIA has k_spmm_sdia -- over shared
// pieces: the column-word decode (sell_word / sell_decode), the SELL-DIA slice metadata
// (SdiaSlice), the gather of one or K vectors (gather_k) and the row hand-off to the epilogue
// (RowOut); and ONE launch function, launch_sell (grid rule, minimum-workgroups rule, argument
// builders, dispatch over the layout), which fails loudly where a layout has no kernel.
#pragma once

#include "lspcg_internal.hpp"
#include "lspcg_spmv.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace lspcg {

constexpr int kSellC = 64;  // rows per slice = one wave64

// Column storage: 16-bit offsets from the slice's first row when every |col - 64*slice| <=
// 32767 (banded FEM orderings: 6 instead of 8 B per fp32-valued entry), padding marked by the
// sentinel kSellPad16; otherwise int32 columns with padding sentinel -1.  Either way the kernel
// needs no row lengths (no dependent rowptr load before the entry loads).
constexpr int16_t kSellPad16 = -32768;

// Slice-diagonal layout ("SELL-DIA", col_bits == 1; structured-grid orderings: the Kuhn-tet
// stencil has 15 distinct row-relative offsets col - row per 64-row slice, the 2-D 5-point stencil
// 5, boundary rows use subsets).  Each slice s keeps its D_s <= 16 distinct offsets, ascending, in
// dict[16 s + j] and stores its rows' values slot-major, ONE slot per dictionary entry:
//     vals[64 (gp[s] + j) + lane]   (row 64 s + lane, column row + dict[16 s + j]),
// with bit lane of the LANE MASK mask[16 s + j] (64-bit words) set where the row has that entry
// (absent entries: value 0, bit clear, never added; the words of slots j >= D_s are 0).  Rows are
// sorted, so slot order = the row's column order = scipy's sum order.  No column storage at all: the
// offset of slot j is wave-uniform (a scalar register), the x / r / t / p "gather" of slot j is one
// contiguous 64-entry load, and a row costs D_s values + 2 bytes of mask (128 B per slice; Kuhn: 15
// slots per row where SELL-64's 4-entry groups store 16).
// Addressing: everything per slot is scalar.  A slot's mask word comes through a
// scalar load and is the select's lane mask as it stands.  The values of slot j are read at the
// slice's per-lane base + the compile-time offset 64 j, with no clamp: a surplus slot of the last
// batch reads the next slice's values (masked), and every value array ends in kSdiaPadSlots zeroed
// slots so that the last slice's surplus stays inside the allocation (BSELL-DIA keeps 16-bit row masks,
// the clamped slot index and the per-lane select: BsdiaSlice).  The vector window of slot j
// is loaded unconditionally at base + dict[j] + lane through a range-checked buffer load whose
// resource covers exactly the xn vector entries the pattern reads: a window that starts before row
// 0 or ends past xn returns 0 for those lanes, which the mask never adds (sdia_ranged: plain
// vectors of <= kSdiaRangedMax entries; fused gathers and longer vectors keep the per-lane select
// that reads the slice's first row in masked lanes).
constexpr int kSdiaMax = 16;       // slots (distinct offsets) per slice
constexpr int kSdiaPadSlots = kSdiaMax - 1;  // zeroed slots behind a SELL-DIA value array
// Largest vector (entries) read through the range-checked loads: the 32-bit byte offset
// 8 (base + dict[j] + lane) of a column in (-n, n + xn + 64) must neither wrap into [0, 8 xn) from
// below (2^32 - 8 n >= 8 xn) nor from above (8 (n + xn + 64) <= 2^32); 2^27 entries keep both.
constexpr int64_t kSdiaRangedMax = int64_t(1) << 27;
// column-storage choices for sell_build_pattern (bit mask); int32 columns are always possible
constexpr int kSellCol16 = 1;
constexpr int kSellColDia = 2;
constexpr int kSellColCode = 4;
// Coded SELL-64 ("SELL-64C", col_bits == 8; unstructured orderings after a bandwidth-reducing
// permutation, where a slice's rows share few row-relative offsets col - row but more than SELL-DIA's
// 16): SELL-64's slot layout and values, with ONE byte per slot -- the rank of the slot's offset in
// its slice's ascending dictionary dict[64 s + j] (<= 64 entries, kSellCodePad for padding) --
// instead of a 16-bit column offset.  The lane's dictionary entry sits in one register and a code
// is decoded with one ds_bpermute (no LDS allocation).  Slices with more than 64 distinct offsets
// keep 16-bit offsets in a second array: rgp[s] = their first group there (-1: coded slice).
constexpr int kSellCodeMax = 64;
constexpr uint8_t kSellCodePad = 0xff;
// Jagged SELL-64 ("SELL-64J", col_bits == kSellJag: 16-bit offsets; unstructured meshes, whose rows
// in one 64-row slice range from 4 to ~35 entries, so SELL-64's 64 x longest-row slots pad 1.6x).
// Inside each slice the LANES are sorted by descending row length (ties by row): lane l owns row
// 64 s + lmap[64 s + l], and group q (entries 4q .. 4q+3) holds only the cnt_q = jc[16 s + q] lanes
// whose rows reach it, a prefix of the lanes -- stored densely:
//     entry k of lane l at  gp[s] + 4 (cnt_0 + ... + cnt_{q-1}) + 4 l + k % 4,   q = k / 4, l < cnt_q,
// with gp[s] the slice's first ELEMENT.  Padding is only the row's last group (16.1 -> 17.6 entries
// per row on the 1 M Delaunay mesh, vs 26.1 for SELL-64).  Rows move only inside their slice, so x
// gathers and y / r / p accesses hit the same cache lines as before, and slot k is still entry k of
// its row: scipy's sum order, the same bits.  Rows of more than 64 entries (16 groups) keep SELL-64.
constexpr int kSellJag = 17;
constexpr int kSellJagMaxG = 16;   // groups per slice (jc bytes per slice)
constexpr int kSellColJag = 8;     // sell_build_pattern: jagged 16-bit layout allowed
constexpr double kSellJagPad = 1.15;  // taken when SELL-64 stores more than this x nnz slots
// x-staged SELL-64J ("SELL-64X", col_bits == kSellJagX): the jagged layout whose 16-bit column words
// are positions in an LDS copy of the vector blocks the row tile (4 slices, 256 rows) touches.  An
// unstructured mesh's 64-row slice gathers ~14 distinct 128-B lines per 64-lane gather (Kuhn grid: 4),
// mostly L1 misses (a slice's x footprint is ~11 KB, 24 resident slices per CU), and those gathers
// cost 40 % of the jagged SpMV (tools/jag_probe.py: 43.8 vs 26.8 us with contiguous gathers, delaunay1m).
// Here a tile's distinct 16-element x blocks (xl[xlp[t] .. xlp[t+1]), ascending; ~170 on delaunay1m)
// are loaded ONCE per tile with 16-B loads into LDS (barrier), and entry k's word is
// slot * 16 + col % 16 with slot the block's rank in the list: the gathers become LDS reads of the
// same values, so the bits are unchanged.  kx = the largest list (LDS: kx * 16 * sizeof(x) per
// workgroup); patterns whose tiles touch more than kSellXMax blocks keep SELL-64J.
constexpr int kSellJagX = 18;
constexpr int kSellColXs = 16;  // sell_build_pattern: the x-staged layout allowed (GatherVec only)
constexpr int kSellXMax = 256;  // blocks per tile (32 KB of fp64)
constexpr int kSellXBlk = 16;   // vector entries per staged block
// smallest pattern staged: below it the per-tile staging latency and barriers cost more than the
// gathers they replace (us per iteration, SELL-64X vs SELL-64J: delaunay1m 127.0 vs 134.9, delaunay64k
// 31.5 vs 28.6, bunny 18.8 vs 16.9; profiles/r6_sellx_probe.jsonl); sellx_min_n() is the floor in use
constexpr int64_t kSellXMinN = 262144;
// col_bits of the other layouts (with kSellJag / kSellJagX the `kind` numbers the C ABI reports)
constexpr int kSellDia = 1;     // SELL-DIA, BSELL-DIA
constexpr int kSellCoded = 8;   // SELL-64C
constexpr int kSellOff16 = 16;  // SELL-64 / BSELL-64, 16-bit offsets
constexpr int kSellInt32 = 32;  // SELL-64 / BSELL-64, int32 columns

// Pattern shared by every matrix with the same CSR (rowptr, colind).
//
// Block variant (bs == 3, "BSELL-64"; BSR 3x3 matrices): a wave owns 64
// consecutive BLOCK rows; slot q of block row I = 64 s + lane holds ONE column index (int32 block
// column or 16-bit offset from 64 s) and the block's 9 values (v = 3 a + c) in 16-byte lane
// chunks: planes 0-7 in groups of W = 16 / sizeof(value) (fp64 pairs, fp32 quads), plane 8 alone,
//     col[64 (gp[s] + q) + lane],
//     vals[576 (gp[s] + q) + 64 W (v / W) + W lane + v % W]   (v < 8),  vals[576 (gp[s] + q) + 512 + lane]
// so a slot is 8 / W + 1 value loads (16-B per lane, 1 KiB per wave instruction) + 1 column load
// and a block costs 9 values + 1 column instead of 9 scalar (value, column) pairs; x is gathered
// once per block (3 consecutive entries) for the lane's 3 scalar rows.  Row 3I + a sums its blocks in column
// order and inside a block c = 0, 1, 2: the order of the reference's expanded scalar CSR
// (validate.py:51), in-block zeros kept (adding an exact 0*x changes no finite sum).
struct SellPattern {
  int64_t n = 0;                   // scalar rows
  int64_t nb = 0;                  // rows of the pattern: scalar rows (bs 1) or block rows (bs 3)
  int bs = 1;
  int64_t ns = 0;                  // slices
  int64_t groups = 0;              // gp[ns]: 4-entry groups (bs 1) / block slots (bs 3) / DIA slots per lane, summed
  int32_t* gp = nullptr;           // [ns+1] exclusive prefix of per-slice groups (slots) per row
  void* col = nullptr;             // [256*groups] (bs 1) / [64*groups] (bs 3) int32 columns or int16 offsets;
                                   // SELL-DIA (col_bits 1): [16*ns] 64-bit lane masks, one per slot
                                   // (BSELL-DIA: [64*ns] uint16 row masks)
  int col_bits = kSellInt32;
  int32_t* dict = nullptr;         // SELL-DIA: [16*ns] ascending row-relative offsets per slice;
                                   // SELL-64C (col_bits 8): [64*ns], col = [256*groups] uint8 codes
  int32_t* rgp = nullptr;          // SELL-64C: [ns] group start in col2 of a slice kept uncoded, or -1
  int16_t* col2 = nullptr;         // SELL-64C: 16-bit offsets of the uncoded slices
  uint8_t* lmap = nullptr;         // SELL-64J: [64*ns] row (within the slice) of each lane
  uint8_t* jc = nullptr;           // SELL-64J: [16*ns] lanes per group (non-increasing, 0 past the last)
  int64_t elems = 0;               // SELL-64J: stored entries (gp is an element prefix, not a group prefix)
  int32_t* xlp = nullptr;          // SELL-64X: [ntiles+1] block-list prefix per 256-row tile
  int32_t* xl = nullptr;           // SELL-64X: the tiles' ascending x-block lists
  int kx = 0;                      // SELL-64X: the longest list
  int64_t xn = 0;                  // SELL-64X, SELL-DIA, BSELL-DIA: vector entries read (largest column + 1;
                                   // > n for dist_pcg's halo)
  const int32_t* rowptr = nullptr; // CSR row pointer (row lengths), not owned
  // Every field above, pointers and values alike, to f: what a launch captured in a graph holds of
  // the pattern (the solver's graph_key).  A new field belongs in the list above AND here.
  template <class F>
  void each_field(F f) const {
    f(n), f(nb), f(bs), f(ns), f(groups), f(gp), f(col), f(col_bits), f(dict), f(rgp), f(col2), f(lmap), f(jc);
    f(elems), f(xlp), f(xl), f(kx), f(xn), f(rowptr);
  }
  // the jagged element layout (SELL-64J / SELL-64X): gp is an element prefix
  bool jagged() const { return col_bits == kSellJag || col_bits == kSellJagX; }
  // entries of a value array of this pattern
  int64_t slots() const {
    if (bs == 3) return int64_t(576) * groups;  // BSELL-64 / BSELL-DIA: 9 values per block slot
    return jagged() ? elems : (col_bits == kSellDia ? int64_t(64) : int64_t(256)) * groups;
  }
  // entries sell_fill_values / bsell_fill_values allocate: slots() + SELL-DIA's zeroed surplus slots
  // (see kSdiaPadSlots)
  int64_t alloc_slots() const {
    return slots() + (col_bits == kSellDia && bs == 1 ? int64_t(kSdiaPadSlots) * 64 : 0);
  }
  void release() {  // the owned arrays (not rowptr)
    auto drop = [](auto*& p) {
      (void)hipFree(p);
      p = nullptr;
    };
    drop(gp), drop(col), drop(dict), drop(rgp), drop(col2), drop(lmap), drop(jc), drop(xlp), drop(xl);
  }
};

template <typename VT, typename CT>
struct SellArgs {
  int64_t n;
  int64_t ns;
  const int32_t* gp;
  const CT* col;
  const VT* vals;
  const int32_t* dict = nullptr;  // SELL-64C (CT = uint8_t): see kSellCodeMax
  const int32_t* rgp = nullptr;
  const int16_t* col2 = nullptr;
  const uint8_t* lmap = nullptr;  // SELL-64J: see kSellJag
  const uint8_t* jc = nullptr;
  const int32_t* xlp = nullptr;   // SELL-64X: see kSellJagX
  const int32_t* xl = nullptr;
  int64_t xn = 0;
};

template <typename VT>
struct SdiaArgs {
  int64_t n;
  int64_t ns;
  const int32_t* gp;
  const uint64_t* mask;  // [16 ns] lane masks (BSELL-DIA: the same bytes as [64 ns] uint16 row masks)
  const int32_t* dict;
  const VT* vals;
  int64_t xn;            // vector entries the pattern reads
};

// the kernel arguments of a pattern and one of its value arrays (a layout's kernel reads its own fields)
template <typename VT, typename CT>
inline SellArgs<VT, CT> sell_args(const SellPattern& P, const void* vals) {
  return {P.n,  P.ns,   P.gp, static_cast<const CT*>(P.col), static_cast<const VT*>(vals), P.dict, P.rgp, P.col2,
          P.lmap, P.jc, P.xlp, P.xl, P.xn};
}
template <typename VT>
inline SdiaArgs<VT> sdia_args(const SellPattern& P, const void* vals) {
  return {P.n, P.ns, P.gp, static_cast<const uint64_t*>(P.col), P.dict, static_cast<const VT*>(vals), P.xn};
}

// ---- the SpMV ----------------------------------------------------------------
template <typename VT>
struct Vec4Ld;
template <>
struct Vec4Ld<float> {
  __device__ static __forceinline__ void load(const float* p, float (&v)[4]) {
    const f32x4 a = *(const __attribute__((address_space(1))) f32x4*)(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  }
};
template <>
struct Vec4Ld<double> {
  __device__ static __forceinline__ void load(const double* p, double (&v)[4]) {
    const auto* q = (const __attribute__((address_space(1))) f64x2*)(p);
    const f64x2 a = q[0], b = q[1];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  }
};

using i16x4 = short __attribute__((ext_vector_type(4)));
using xs_u4 = unsigned __attribute__((ext_vector_type(4)));  // 16-B staging part (SELL-64X)

// Epilogues with a PREFETCH member (a device pointer) read one own-row value in row(); the SELL
// kernel loads it before the row's slot loop so it does not add a memory latency after the
// gathers, and passes it to row_pf() (latency-bound mid-size systems).
template <class E, class = void>
struct epi_prefetch : std::false_type {};
template <class E>
struct epi_prefetch<E, std::void_t<decltype(E::PREFETCH)>> : std::bool_constant<E::PREFETCH> {};

// K right-hand sides at once (k_spmm_sdia, k_spmv_sell with K > 1; launched by lspcg_multi.hip;
// DESIGN.md §6 "Several right-hand sides").  The vectors are interleaved [n][K]: entry (row, column k)
// at row * K + k, so the K entries one slot gathers are contiguous -- one load of K * sizeof(T) bytes
// in 16-B parts (8 B for two floats).  A slot's value, column and live flag are loaded once and
// applied to the K entries; per column the slots are added in the K = 1 order, so every column's row
// sums are the single-vector kernel's bit for bit.  The epilogue's row() takes the K row sums; NDOT
// counts all of its dots (K per reduced quantity).
template <typename T, int K>
struct RowK {
  static constexpr int W = K * sizeof(T) >= 16 ? 16 / int(sizeof(T)) : K;  // entries per load
  using V = T __attribute__((ext_vector_type(W)));
  __device__ static __forceinline__ void load(const T* p, T (&v)[K]) {
#pragma unroll
    for (int c = 0; c < K / W; ++c) {
      const V a = *(const __attribute__((address_space(1))) V*)(p + c * W);
#pragma unroll
      for (int w = 0; w < W; ++w) v[c * W + w] = a[w];
    }
  }
  __device__ static __forceinline__ void store(T* p, const T (&v)[K]) {
#pragma unroll
    for (int c = 0; c < K / W; ++c) {
      V a;
#pragma unroll
      for (int w = 0; w < W; ++w) a[w] = v[c * W + w];
      *(__attribute__((address_space(1))) V*)(p + c * W) = a;
    }
  }
};

// the vector at column c: the gather functor's entry (K = 1) or the K entries of row c of its vector
template <int K, typename T, class Gx>
__device__ __forceinline__ void gather_k(const Gx& gx, int64_t c, T (&xv)[K]) {
  if constexpr (K == 1) xv[0] = gx(c);
  else RowK<T, K>::load(gx.x + c * K, xv);
}

// a stored column word that is an entry, not padding (kSellPad16 in 16-bit words, -1 in int32 columns)
template <typename CT>
__device__ __forceinline__ bool sell_real(int o) {
  return sizeof(CT) == 2 ? o != kSellPad16 : o >= 0;
}

// A column word (a 16-bit offset from the slice's first row `base`, or an int32 column) -> the
// column to gather and the live flag.  Padding and the words of a clamped surplus group (!in) gather
// the slice's first row and are never added.
template <typename CT>
__device__ __forceinline__ void sell_word(int o, int32_t base, bool in, bool& m, int& c) {
  static_assert(std::is_same<CT, int16_t>::value || std::is_same<CT, int32_t>::value, "16-bit offsets or int32 columns");
  const bool real = sell_real<CT>(o);
  m = real && in;
  c = sizeof(CT) == 2 ? base + (real ? o : 0) : (real ? o : base);
}
// one 4-entry group's words, one 8- or 16-byte load
template <typename CT>
__device__ __forceinline__ void sell_decode(const CT* p, int32_t base, bool in, bool (&m)[4], int (&c)[4]) {
  using V = CT __attribute__((ext_vector_type(4)));
  const V cc = *(const __attribute__((address_space(1))) V*)(p);
  const int o[4] = {cc.x, cc.y, cc.z, cc.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) sell_word<CT>(o[j], base, in, m[j], c[j]);
}

// The hand-off of a lane's row sum (K = 1) or its K row sums to the epilogue.  prefetch() goes
// before the slot loop: a PREFETCH epilogue's own-row value is loaded there and handed to row_pf().
template <typename T, int K, class Epi>
struct RowOut {
  static constexpr bool PF = epi_prefetch<Epi>::value && K == 1;
  T pf = T(0);
  __device__ __forceinline__ void prefetch(Epi& epi, int64_t i, bool live) {
    if constexpr (PF) {
      if (live) pf = epi.prefetch(i);
    }
  }
  __device__ __forceinline__ void emit(Epi& epi, int64_t i, bool live, T acc, DD* d) const {
    if (!live) return;
    if constexpr (PF) epi.row_pf(i, acc, d, pf);
    else epi.row(i, acc, d);
  }
  __device__ __forceinline__ void emit(Epi& epi, int64_t i, bool live, const T (&acc)[K], DD* d) const {
    if constexpr (K == 1) {
      emit(epi, i, live, acc[0], d);
    } else {
      if (live) epi.row(i, acc, d);
    }
  }
};

// 256-thread workgroups = 4 slices = one 256-row tile (the same row tiles as k_spmv, so the
// prologue / epilogue functors and the dot-product reduction are shared).  QB groups of 4
// entries are loaded per lane before the first gather (branch-free: the group index is
// clamped, the surplus is masked at the add).
// MINW: minimum workgroups per CU the register allocation must allow (6 x 256 threads for the
// compact-value PCG kernels, whose reducing launches use a resident 6-per-CU grid; 1 for fp64
// values and the double-gather fused epilogues, which need more registers than 6/CU leaves).
// K > 1: K interleaved vectors (see RowK), K accumulators per lane; 16-bit offsets or int32 columns.
template <typename T, typename VT, typename CT, int QB, int TH, int MINW, class Pro, class Gx, class Epi, int K = 1>
__global__ void __launch_bounds__(TH, MINW) k_spmv_sell(SellArgs<VT, CT> a, Pro pro, Gx gx, Epi epi) {
  constexpr int ND = Epi::NDOT > 0 ? Epi::NDOT : 1;
  constexpr bool C8 = std::is_same<CT, uint8_t>::value;  // SELL-64C
  static_assert(K == 1 || !C8, "SELL-64C has no K-vector kernel");
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t ntiles = (a.n + TH - 1) / TH;
  // the first tile's slice range is loaded before the prologue's state read, so the two
  // dependent-free loads share one memory latency (the state line was written by another CU)
  int32_t gb[2] = {0, 0};
  [[maybe_unused]] int32_t rg = -1, dl = 0;  // SELL-64C: uncoded group start, this lane's dictionary entry
  if (int64_t(blockIdx.x) * (TH / 64) + w < a.ns) {
    gb[0] = a.gp[int64_t(blockIdx.x) * (TH / 64) + w];
    gb[1] = a.gp[int64_t(blockIdx.x) * (TH / 64) + w + 1];
    if constexpr (C8) {
      rg = a.rgp[int64_t(blockIdx.x) * (TH / 64) + w];
      dl = a.dict[kSellCodeMax * (int64_t(blockIdx.x) * (TH / 64) + w) + lane];
    }
  }
  if (pro.exit()) return;
  gx.prepare();
  epi.prepare();
  DD d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = dd_zero();
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * (TH / 64) + w;
    const int64_t i = tile * TH + threadIdx.x;
    if (s < a.ns) {  // wave-uniform
      if (tile != int64_t(blockIdx.x)) {
        gb[0] = a.gp[s];
        gb[1] = a.gp[s + 1];
        if constexpr (C8) {
          rg = a.rgp[s];
          dl = a.dict[kSellCodeMax * s + lane];
        }
      }
      const int32_t g0 = gb[0];
      const int nq = gb[1] - g0;
      const int32_t base = int32_t(s * kSellC);
      const VT* vp = a.vals + 256 * int64_t(g0) + 4 * lane;
      const CT* cp = a.col + 256 * int64_t(g0) + 4 * lane;
      [[maybe_unused]] const int16_t* cp2 = C8 ? a.col2 + 256 * int64_t(rg) + 4 * lane : nullptr;
      T acc[K];
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = T(0);
      RowOut<T, K, Epi> out;
      out.prefetch(epi, i, i < a.n);
      for (int q0 = 0; q0 < nq; q0 += QB) {
        VT v[QB][4];
        int c[QB][4];
        bool m[QB][4];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
          const int q = min(q0 + u, nq - 1);
          Vec4Ld<VT>::load(vp + 256 * q, v[u]);
          if constexpr (C8) {
            if (rg < 0) {  // wave-uniform: a coded slice
              const unsigned cc = *(const __attribute__((address_space(1))) unsigned*)(cp + 256 * q);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const unsigned b = (cc >> (8 * j)) & 0xffu;
                const int off = __builtin_amdgcn_ds_bpermute(int((b & 63u) << 2), dl);
                m[u][j] = (b != kSellCodePad) && (q0 + u < nq);
                c[u][j] = b != kSellCodePad ? base + lane + off : base;  // padding gathers row base
              }
            } else {
              sell_decode(cp2 + 256 * q, base, q0 + u < nq, m[u], c[u]);
            }
          } else {
            sell_decode(cp + 256 * q, base, q0 + u < nq, m[u], c[u]);
          }
        }
        T xv[QB][4][K];
#pragma unroll
        for (int u = 0; u < QB; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) gather_k<K>(gx, c[u][j], xv[u][j]);
#pragma unroll
        for (int u = 0; u < QB; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m[u][j]) {
#pragma unroll
              for (int k = 0; k < K; ++k) acc[k] = acc[k] + T(v[u][j]) * xv[u][j][k];
            }
      }
      out.emit(epi, i, i < a.n, acc, d);
    }
  }
  finish_epi_dots<Epi>(d, epi);
}

// SELL-64J SpMV (layout: see kSellJag): one wave = one 64-row slice; lane l sums row 64 s + lmap[l].
// The slice's metadata is its first element gp[s], the 16 group counts (two 8-byte scalar loads)
// and the lane's row byte, loaded in one batch (the first tile's before the prologue's state read).
// Group q's loads are issued only by its cnt_q active lanes (a prefix of the wave): a shorter row's
// lane neither loads nor adds past its last group.  The counts are consumed from a 128-bit scalar
// shift register, QB groups per batch, every load of a batch before the first add.
// XS (SELL-64X, kSellJagX): the column words index the tile's LDS copy of its x blocks (dynamic
// shared memory, kx * 16 entries), staged by the whole workgroup between two barriers per tile.
template <typename T, typename VT, int QB, int TH, int MINW, bool XS, class Pro, class Gx, class Epi>
__global__ void __launch_bounds__(TH, MINW) k_spmv_sellj(SellArgs<VT, int16_t> a, Pro pro, Gx gx, Epi epi) {
  static_assert(QB >= 1 && QB <= 4, "QB groups per batch");
  static_assert(!XS || std::is_same<Gx, GatherVec<T>>::value, "SELL-64X stages a plain vector");
  constexpr int ND = Epi::NDOT > 0 ? Epi::NDOT : 1;
  [[maybe_unused]] extern __shared__ __attribute__((aligned(16))) unsigned char sx_raw[];
  [[maybe_unused]] T* sx = reinterpret_cast<T*>(sx_raw);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t ntiles = (a.n + TH - 1) / TH;
  int32_t e0 = 0;
  uint64_t c0 = 0, c1 = 0;
  int rl = 0;
  auto meta = [&](int64_t sl) {
    e0 = a.gp[sl];
    const uint64_t* cp = reinterpret_cast<const uint64_t*>(a.jc + kSellJagMaxG * sl);
    c0 = cp[0];
    c1 = cp[1];
    rl = a.lmap[kSellC * sl + lane];
  };
  // QB groups' loads (values, column words) of the lane's row, issued for the active lanes only;
  // advances the element offset and the count shift register
  struct Batch {
    VT v[QB][4];
    i16x4 cc[QB];
  };
  auto issue = [&](Batch& B, int32_t& eo, uint64_t& lo, uint64_t& hi) {
#pragma unroll
    for (int u = 0; u < QB; ++u) {
      const int cq = int((lo >> (8 * u)) & 0xffu);
      B.cc[u] = i16x4{kSellPad16, kSellPad16, kSellPad16, kSellPad16};
      B.v[u][0] = B.v[u][1] = B.v[u][2] = B.v[u][3] = VT(0);
      if (lane < cq) {
        Vec4Ld<VT>::load(a.vals + int64_t(eo) + 4 * lane, B.v[u]);
        B.cc[u] = *(const __attribute__((address_space(1))) i16x4*)(a.col + int64_t(eo) + 4 * lane);
      }
      eo += 4 * cq;
    }
    lo = (lo >> (8 * QB)) | (hi << (64 - 8 * QB));
    hi >>= 8 * QB;
  };
  uint64_t lo = 0, hi = 0;
  int32_t eo = 0;
  Batch cur;
  {  // the first tile's metadata and first batch (matrix data only) before the prologue's state read
    const int64_t s = int64_t(blockIdx.x) * (TH / 64) + w;
    if (int64_t(blockIdx.x) < ntiles && s < a.ns) {
      meta(s);
      lo = c0;
      hi = c1;
      eo = e0;
      if (lo & 0xffu) issue(cur, eo, lo, hi);
    }
  }
  if (pro.exit()) return;
  gx.prepare();
  epi.prepare();
  DD d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = dd_zero();
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * (TH / 64) + w;
    const bool live = s < a.ns;  // wave-uniform
    if (live && tile != int64_t(blockIdx.x)) {  // the first batch's loads fly during the staging
      meta(s);
      lo = c0;
      hi = c1;
      eo = e0;
      if (lo & 0xffu) issue(cur, eo, lo, hi);
    }
    if constexpr (XS) {  // the tile's x blocks -> LDS (16-B loads; a block past n element by element)
      if (tile != int64_t(blockIdx.x)) __syncthreads();  // the previous tile's LDS reads are done
      const int32_t b0 = a.xlp[tile], nbk = a.xlp[tile + 1] - b0;
      constexpr int W = 16 / int(sizeof(T));   // entries per 16-B part
      constexpr int PPB = kSellXBlk / W;       // parts per block
      const T* xg = gx.x;
      for (int p = threadIdx.x; p < nbk * PPB; p += TH) {
        const int64_t e = int64_t(a.xl[b0 + p / PPB]) * kSellXBlk + (p % PPB) * W;
        T* dst = sx + (p / PPB) * kSellXBlk + (p % PPB) * W;
        if (e + W <= a.xn) {
          *reinterpret_cast<xs_u4*>(dst) = *(const __attribute__((address_space(1))) xs_u4*)(xg + e);
        } else {
#pragma unroll
          for (int k = 0; k < W; ++k) dst[k] = e + k < a.xn ? xg[e + k] : T(0);
        }
      }
      __syncthreads();
    }
    if (live) {
      const int32_t base = int32_t(s * kSellC);
      const int64_t i = int64_t(base) + rl;
      T acc = T(0);
      RowOut<T, 1, Epi> out;
      out.prefetch(epi, i, i < a.n);
      bool have = (c0 & 0xffu) != 0;
      while (have) {  // wave-uniform: software-pipelined, the next batch's loads beside this one's gathers
        const bool more = (lo & 0xffu) != 0;
        Batch nxt;
        if (more) issue(nxt, eo, lo, hi);
        bool m[QB][4];
        T xv[QB][4];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
          const int o[4] = {cur.cc[u].x, cur.cc[u].y, cur.cc[u].z, cur.cc[u].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            m[u][j] = sell_real<int16_t>(o[j]);
            if constexpr (XS) xv[u][j] = sx[m[u][j] ? o[j] : 0];
            else xv[u][j] = gx(base + (m[u][j] ? o[j] : 0));
          }
        }
#pragma unroll
        for (int u = 0; u < QB; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m[u][j]) acc = acc + T(cur.v[u][j]) * xv[u][j];
        if (more) cur = nxt;
        have = more;
      }
      out.emit(epi, i, i < a.n, acc, d);
    }
  }
  finish_epi_dots<Epi>(d, epi);
}

// position of plane v of lane `lane` inside a BSELL-64 slot (see SellPattern)
template <typename VT>
__host__ __device__ constexpr int bsell_pos(int v, int lane) {
  constexpr int W = 16 / int(sizeof(VT));
  return v < 8 ? 64 * W * (v / W) + W * lane + v % W : 512 + lane;
}

// the 9 values of this lane's block in slot `slot` (576 values): 16-B loads
__device__ __forceinline__ void bsell_load_block(const double* slot, double (&v)[9]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f64x2 a = *(const __attribute__((address_space(1))) f64x2*)(slot + bsell_pos<double>(2 * k, lane));
    v[2 * k] = a.x;
    v[2 * k + 1] = a.y;
  }
  v[8] = gld(slot + bsell_pos<double>(8, lane));
}
__device__ __forceinline__ void bsell_load_block(const float* slot, float (&v)[9]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const f32x4 a = *(const __attribute__((address_space(1))) f32x4*)(slot + bsell_pos<float>(4 * k, lane));
    v[4 * k] = a.x;
    v[4 * k + 1] = a.y;
    v[4 * k + 2] = a.z;
    v[4 * k + 3] = a.w;
  }
  v[8] = gld(slot + bsell_pos<float>(8, lane));
}

// BSR 3x3 over the BSELL-64 layout (see SellPattern): one lane = one block row = 3 scalar rows,
// QB block slots loaded per batch before the first gather.
template <typename T, typename VT, typename CT, int QB, int TH, int MINW, class Pro, class Gx, class Epi>
__global__ void __launch_bounds__(TH, MINW) k_spmv_bsell3(SellArgs<VT, CT> a, Pro pro, Gx gx, Epi epi) {
  constexpr int ND = Epi::NDOT > 0 ? Epi::NDOT : 1;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t nb = a.n / 3;
  const int64_t ntiles = (nb + TH - 1) / TH;
  int32_t gb[2] = {0, 0};  // first tile's slice range, loaded beside the prologue's state read
  if (int64_t(blockIdx.x) * (TH / 64) + w < a.ns) {
    gb[0] = a.gp[int64_t(blockIdx.x) * (TH / 64) + w];
    gb[1] = a.gp[int64_t(blockIdx.x) * (TH / 64) + w + 1];
  }
  if (pro.exit()) return;
  gx.prepare();
  epi.prepare();
  DD d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = dd_zero();
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * (TH / 64) + w;
    const int64_t I = tile * TH + threadIdx.x;
    if (s < a.ns) {  // wave-uniform
      if (tile != int64_t(blockIdx.x)) {
        gb[0] = a.gp[s];
        gb[1] = a.gp[s + 1];
      }
      const int32_t g0 = gb[0];
      const int nq = gb[1] - g0;
      const int32_t base = int32_t(s * kSellC);
      const VT* vp = a.vals + 576 * int64_t(g0);
      const CT* cp = a.col + 64 * int64_t(g0) + lane;
      T acc[3] = {T(0), T(0), T(0)};
      for (int q0 = 0; q0 < nq; q0 += QB) {
        VT v[QB][9];
        int c[QB];
        bool m[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
          const int q = min(q0 + u, nq - 1);
          bsell_load_block(vp + 576 * q, v[u]);
          const int o = int(gld(cp + 64 * q));
          sell_word<CT>(o, base, q0 + u < nq, m[u], c[u]);
        }
        T xv[QB][3];
#pragma unroll
        for (int u = 0; u < QB; ++u)
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) xv[u][cc] = gx(3 * int64_t(c[u]) + cc);
#pragma unroll
        for (int u = 0; u < QB; ++u)
          if (m[u]) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) acc[r] = acc[r] + T(v[u][3 * r + cc]) * xv[u][cc];
          }
      }
      if (I < nb) {
#pragma unroll
        for (int r = 0; r < 3; ++r) epi.row(3 * I + r, acc[r], d);
      }
    }
  }
  finish_epi_dots<Epi>(d, epi);
}

// A SELL-DIA slice's metadata: its slot range (gp) and its whole 16-entry offset
// dictionary, wave-uniform and loaded in one batch of scalar loads (dictionary entries past the
// slice's count are 0 and their lane masks are 0: such a slot loads legally and is never added).
// The lane masks are loaded batch by batch (masks): a ranged kernel needs them only at the adds, so
// their scalar loads fly beside the batch's value and window loads.
struct SdiaSlice {
  int32_t g0 = 0, g1 = 0;
  int32_t dct[kSdiaMax];
  const uint64_t* mp = nullptr;
  template <typename VT>
  __device__ __forceinline__ void load(const SdiaArgs<VT>& a, int64_t sl) {
    g0 = a.gp[sl];
    g1 = a.gp[sl + 1];
    const int32_t* dp = a.dict + kSdiaMax * sl;
#pragma unroll
    for (int j = 0; j < kSdiaMax; ++j) dct[j] = dp[j];
    mp = a.mask + kSdiaMax * sl;
  }
  template <int SB>
  __device__ __forceinline__ void masks(int j0, uint64_t (&mk)[SB]) const {
#pragma unroll
    for (int u = 0; u < SB; ++u) mk[u] = mp[j0 + u];
  }
  // this lane's values of slot 0 (slot j: + 64 j entries, a compile-time offset; SELL-DIA)
  template <typename VT>
  __device__ __forceinline__ const VT* values(const SdiaArgs<VT>& a, int lane) const {
    return a.vals + kSellC * int64_t(g0) + lane;
  }
};
// whether this lane's row has the slot of lane mask `word`: the word as the select's condition
__device__ __forceinline__ bool sdia_has(uint64_t word) { return __builtin_amdgcn_inverse_ballot_w64(word); }
// acc + v x where the row has the slot, acc untouched (not acc + 0 x) where not.  A select, not a
// branch: a branch lets the compiler sink the slot's loads behind the mask test, out of the batch.
template <typename T, typename VT>
__device__ __forceinline__ T sdia_add(uint64_t word, T acc, VT v, T x) {
  const T t = acc + T(v) * x;
  return sdia_has(word) ? t : acc;
}

// The vector windows of a SELL-DIA slice through range-checked buffer loads (see
// kSdiaMax): the resource covers the `entries` entries of x, the whole byte offset
// sizeof(T) * (first + per_lane * lane) is the per-lane offset the hardware checks (first: the
// window's wave-uniform first entry, possibly negative or past the end), and a lane outside the
// vector reads 0.  per_lane: entries per row (1; K for K interleaved vectors).
template <typename T>
struct SdiaWindow {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "fp32 or fp64 vectors");
  using u2 = unsigned __attribute__((ext_vector_type(2)));
  using u4 = unsigned __attribute__((ext_vector_type(4)));
  __amdgpu_buffer_rsrc_t rs;
  unsigned lane_b;
  __device__ __forceinline__ SdiaWindow(const T* x, int64_t entries, int lane, int per_lane)
      : rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, int(unsigned(entries) * unsigned(sizeof(T))),
                                             0x00020000)),
        lane_b(unsigned(lane * per_lane) * unsigned(sizeof(T))) {}
  // (readfirstlane: `first` is wave-uniform; it keeps the scalar part in scalar registers, so the
  // per-lane offset is ONE vector add -- otherwise the compiler re-associates the sum into two)
  __device__ __forceinline__ unsigned offset(int32_t first) const {
    return unsigned(__builtin_amdgcn_readfirstlane(int(unsigned(first) * unsigned(sizeof(T))))) + lane_b;
  }
  __device__ __forceinline__ T at(int32_t first) const {  // the lane's entry of the window at `first`
    const int off = int(offset(first));
    if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, u2(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0)));
    else return __builtin_bit_cast(T, unsigned(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0)));
  }
  template <int K>
  __device__ __forceinline__ void row(int32_t first, T (&v)[K]) const {  // its K entries, in RowK's parts
    constexpr int W = RowK<T, K>::W;
    using V = typename RowK<T, K>::V;
    static_assert(W * sizeof(T) == 8 || W * sizeof(T) == 16, "8- or 16-byte parts");
#pragma unroll
    for (int c = 0; c < K / W; ++c) {
      const int off = int(offset(first) + unsigned(c * W * sizeof(T)));
      V p;
      if constexpr (W * sizeof(T) == 16) p = __builtin_bit_cast(V, u4(__builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0)));
      else p = __builtin_bit_cast(V, u2(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0)));
#pragma unroll
      for (int w = 0; w < W; ++w) v[c * W + w] = p[w];
    }
  }
};
// whether a launch on a plain vector (K interleaved ones) may take them: short enough for the
// 32-bit offset check (kSdiaRangedMax)
inline bool sdia_ranged(const SellPattern& P, int K = 1) {
  return P.xn > 0 && int64_t(K) * std::max(P.n, P.xn) <= kSdiaRangedMax;
}

// SELL-DIA SpMV (layout and addressing: see kSdiaMax): one wave = one 64-row slice of a 256-row
// tile, SB slots per batch, every load of a batch issued before the first add (value loads and
// vector loads are independent: the slot's offset is a scalar).  The first tile's metadata is
// loaded before the prologue's state read: one memory latency before the value / vector loads
// instead of three in a row (state, gp, dictionary).
// RANGED (sdia_ranged; Gx = GatherVec): the vector windows are range-checked buffer loads with no
// per-lane select; otherwise masked lanes gather the slice's first row through gx.
template <typename T, typename VT, int SB, int TH, int MINW, bool RANGED, class Pro, class Gx, class Epi>
__global__ void __launch_bounds__(TH, MINW) k_spmv_sdia(SdiaArgs<VT> a, Pro pro, Gx gx, Epi epi) {
  static_assert(!RANGED || std::is_same<Gx, GatherVec<T>>::value, "range-checked windows read a plain vector");
  constexpr int ND = Epi::NDOT > 0 ? Epi::NDOT : 1;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t ntiles = (a.n + TH - 1) / TH;
  SdiaSlice sl;
  {
    const int64_t s = int64_t(blockIdx.x) * (TH / 64) + w;
    if (int64_t(blockIdx.x) < ntiles && s < a.ns) sl.load(a, s);
  }
  if (pro.exit()) return;
  gx.prepare();
  epi.prepare();
  [[maybe_unused]] const auto win = [&] {
    if constexpr (RANGED) return SdiaWindow<T>(gx.x, a.xn, lane, 1);
    else return 0;
  }();
  DD d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = dd_zero();
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * (TH / 64) + w;
    const int64_t i = tile * TH + threadIdx.x;
    if (s < a.ns) {  // wave-uniform
      if (tile != int64_t(blockIdx.x)) sl.load(a, s);
      const int nd = sl.g1 - sl.g0;
      const int32_t base = int32_t(s * kSellC);
      const VT* vp = sl.values(a, lane);
      T acc = T(0);
      RowOut<T, 1, Epi> out;
      out.prefetch(epi, i, i < a.n);
#pragma unroll
      for (int j0 = 0; j0 < kSdiaMax; j0 += SB) {
        if (j0 >= nd) break;  // wave-uniform
        VT v[SB];
        T xv[SB];
        uint64_t mk[SB];
        sl.masks(j0, mk);
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const int j = j0 + u;
          v[u] = gld(vp + kSellC * j);
          if constexpr (RANGED) xv[u] = win.at(base + sl.dct[j]);
          else xv[u] = gx(sdia_has(mk[u]) ? base + lane + sl.dct[j] : base);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) acc = sdia_add(mk[u], acc, v[u], xv[u]);
      }
      out.emit(epi, i, i < a.n, acc, d);
    }
  }
  finish_epi_dots<Epi>(d, epi);
}

// SELL-DIA SpMV of K interleaved vectors (see RowK): k_spmv_sdia's walk with K accumulators per
// lane.  A kernel of its own, with the vector as a restrict pointer argument and no
// minimum-workgroups bound: as a K parameter of k_spmv_sdia (the vector inside the gather functor,
// after the prologue's argument) the same loop measured 0.6-2.4 % slower per solve on systems of
// 65 k - 70 k rows (profiles/sell_kernels_refactor_ab.json, "k_merged_into_k_spmv_sdia").
// RANGED (sdia_ranged(P, K)): the windows of K a.xn entries through range-checked loads.
template <typename T, typename VT, int K, int SB, int TH, bool RANGED, class Pro, class Epi>
__global__ void __launch_bounds__(TH) k_spmm_sdia(SdiaArgs<VT> a, const T* __restrict__ x, Pro pro, Epi epi) {
  constexpr int ND = Epi::NDOT > 0 ? Epi::NDOT : 1;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t ntiles = (a.n + TH - 1) / TH;
  SdiaSlice sl;
  {
    const int64_t s = int64_t(blockIdx.x) * (TH / 64) + w;
    if (int64_t(blockIdx.x) < ntiles && s < a.ns) sl.load(a, s);
  }
  if (pro.exit()) return;
  [[maybe_unused]] const auto win = [&] {
    if constexpr (RANGED) return SdiaWindow<T>(x, a.xn * K, lane, K);
    else return 0;
  }();
  DD d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = dd_zero();
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * (TH / 64) + w;
    const int64_t i = tile * TH + threadIdx.x;
    if (s < a.ns) {  // wave-uniform
      if (tile != int64_t(blockIdx.x)) sl.load(a, s);
      const int nd = sl.g1 - sl.g0;
      const int32_t base = int32_t(s * kSellC);
      const VT* vp = sl.values(a, lane);
      T acc[K];
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = T(0);
#pragma unroll
      for (int j0 = 0; j0 < kSdiaMax; j0 += SB) {
        if (j0 >= nd) break;  // wave-uniform
        VT v[SB];
        T xv[SB][K];
        uint64_t mk[SB];
        sl.masks(j0, mk);
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const int j = j0 + u;
          v[u] = gld(vp + kSellC * j);
          if constexpr (RANGED) win.row((base + sl.dct[j]) * K, xv[u]);
          else RowK<T, K>::load(x + int64_t(sdia_has(mk[u]) ? base + lane + sl.dct[j] : base) * K, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u)
#pragma unroll
          for (int k = 0; k < K; ++k) acc[k] = sdia_add(mk[u], acc[k], v[u], xv[u][k]);
      }
      if (i < a.n) epi.row(i, acc, d);
    }
  }
  finish_epi_dots<Epi>(d, epi);
}

// A BSELL-DIA slice's metadata (BSELL-DIA keeps SELL-DIA's first form: 16-bit ROW masks, a per-lane
// select for masked lanes and a clamped slot index; the lean form measured 0.6-1.6 us per C4 iteration
// slower): its slot range (gp), its whole 16-entry offset dictionary
// (one scalar block load: entries past the slice's count are never used, masked lanes read x[base])
// and the lane's row mask, loaded in one batch.
struct BsdiaSlice {
  int32_t g0 = 0, g1 = 0;
  unsigned msk = 0;
  int32_t dct[kSdiaMax];
  template <typename VT>
  __device__ __forceinline__ void load(const SdiaArgs<VT>& a, int64_t sl, int lane) {
    g0 = a.gp[sl];
    g1 = a.gp[sl + 1];
    msk = gld(reinterpret_cast<const uint16_t*>(a.mask) + kSellC * sl + lane);
    const int32_t* dp = a.dict + kSdiaMax * sl;
#pragma unroll
    for (int j = 0; j < kSdiaMax; ++j) dct[j] = dp[j];
  }
  // slot j of a batch: whether this lane's row has it (nd = the slice's slot count), and where its
  // values start (clamped: the surplus slots of the last batch load the last slot and are masked)
  __device__ __forceinline__ bool has(int j, int nd) const { return (j < nd) && ((msk >> j) & 1u); }
  __device__ __forceinline__ int64_t slot(int j, int nd) const { return int64_t(g0 + min(j, nd - 1)); }
};

// BSR 3x3 over the BSELL-DIA layout (SELL-DIA's slot dictionary on the block graph + BSELL-64's
// 9-value lane chunks): k_spmv_sdia's walk with one lane = one block row = 3 scalar rows; slot j of
// the slice holds the block at block column I + dict[j] (bit j of the block row's mask), so the x entries of a slot
// are three contiguous 64-block loads at a wave-uniform offset and no column is loaded at all.  The
// slot order is the row's block column order, c = 0, 1, 2 inside a block: the expanded scalar CSR's
// summation order.
template <typename T, typename VT, int SB, int TH, int MINW, class Pro, class Gx, class Epi>
__global__ void __launch_bounds__(TH, MINW) k_spmv_bsdia3(SdiaArgs<VT> a, Pro pro, Gx gx, Epi epi) {
  constexpr int ND = Epi::NDOT > 0 ? Epi::NDOT : 1;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t nb = a.n / 3;
  const int64_t ntiles = (nb + TH - 1) / TH;
  BsdiaSlice sl;
  {
    const int64_t s = int64_t(blockIdx.x) * (TH / 64) + w;
    if (int64_t(blockIdx.x) < ntiles && s < a.ns) sl.load(a, s, lane);
  }
  if (pro.exit()) return;
  gx.prepare();
  epi.prepare();
  DD d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = dd_zero();
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * (TH / 64) + w;
    const int64_t I = tile * TH + threadIdx.x;
    if (s < a.ns) {  // wave-uniform
      if (tile != int64_t(blockIdx.x)) sl.load(a, s, lane);
      const int nd = sl.g1 - sl.g0;
      const int32_t base = int32_t(s * kSellC);
      const int32_t brow = base + lane;
      T acc[3] = {T(0), T(0), T(0)};
#pragma unroll
      for (int j0 = 0; j0 < kSdiaMax; j0 += SB) {
        if (j0 >= nd) break;  // wave-uniform
        VT v[SB][9];
        T xv[SB][3];
        bool m[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const int j = j0 + u;
          m[u] = sl.has(j, nd);
          const int64_t c = 3 * int64_t(m[u] ? brow + sl.dct[j] : base);
          bsell_load_block(a.vals + 576 * sl.slot(j, nd), v[u]);
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) xv[u][cc] = gx(c + cc);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u)
          if (m[u]) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) acc[r] = acc[r] + T(v[u][3 * r + cc]) * xv[u][cc];
          }
      }
      if (I < nb) {
#pragma unroll
        for (int r = 0; r < 3; ++r) epi.row(3 * I + r, acc[r], d);
      }
    }
  }
  finish_epi_dots<Epi>(d, epi);
}

// Reducing launches use a resident grid: 6 workgroups per CU (the compact-value kernels'
// __launch_bounds__ guarantee), i.e. 1536 on MI355X -- one wave of workgroups, each walking its
// row tiles, so no straggler round delays the ticket (8 per CU / 2048 measured the same; caps of
// 1024 / 1342 / 2013 / 4025 measured no better).  Capped by the solver's 4096
// partial slots.  Non-reducing launches take one workgroup per row tile.
inline int64_t sell_cap(bool reducing) {
  static const int64_t rcap = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    return std::max<int64_t>(1, std::min<int64_t>(int64_t(6) * cus, 4096));
  }();
  return reducing ? rcap : int64_t(1) << 40;
}

// largest padded-slots / nnz ratio for which a SELL view is built (LSPCG_SELL_MAXPAD, read once)
inline double sell_max_pad() {
  static const double v = [] {
    const char* e = std::getenv("LSPCG_SELL_MAXPAD");
    return e ? std::atof(e) : 2.0;  // 2-D 5-point rows (5 -> 8 slots) still run faster as SELL
  }();
  return v;
}

// ---- the launch ----------------------------------------------------------------
constexpr int kSellWG = 256;  // 4 slices per workgroup (512 / 1024 measured slower: DESIGN.md §5)

// Grid of a SELL launch: one workgroup per row tile of 256 scalar (bs 1) or block (bs 3) rows, capped
// by sell_cap (the solver sizes the split-reduction groups from it).  one_tile_per_wg (batched
// solves): never capped -- workgroup b owns exactly row tile b, so its dot partial is that tile's
// and its prologue may test the tile's own system.
inline int64_t sell_grid(const SellPattern& P, bool reducing, bool one_tile_per_wg = false) {
  const int64_t tiles = (P.nb + kSellWG - 1) / kSellWG;
  return one_tile_per_wg ? tiles : std::min<int64_t>(tiles, sell_cap(reducing));
}

// Entries in flight per lane and batch.
constexpr int kSdiaSB = 8;   // SELL-DIA slots
// SELL-64 / SELL-64C: 2 groups of 4 entries (tools/sell_sweep.py on kuhn101, dictionary columns, cold:
// fp64 values 32.2 us vs 33.8 with 4 groups and 46.0 with 8; fp32 values 22.7 vs 24.1 / 37.0)
constexpr int kSellQB = 2;
constexpr int kBsellQB = 2;  // BSELL-64 block slots (18 values, 6 gathers)
#ifndef LSPCG_BSDIA_SB64
#define LSPCG_BSDIA_SB64 2
#endif
#ifndef LSPCG_BSDIA_SB32
#define LSPCG_BSDIA_SB32 2
#endif
// BSELL-DIA block slots (2: 18 values, 6 x loads) by value size
template <typename VT>
constexpr int bsdia_sb() { return sizeof(VT) == 8 ? LSPCG_BSDIA_SB64 : LSPCG_BSDIA_SB32; }
#ifndef LSPCG_JAG_QB
#define LSPCG_JAG_QB 2  // SELL-64J / SELL-64X groups of 4 entries
#endif
// K vectors: SELL-DIA batches 8 / 8 / 4 slots for K = 2 / 4 / 8 (<= 32 vector entries of
// K * sizeof(T) bytes in flight per lane: mid-size systems run one wave per SIMD, so a lane's own
// loads in flight, not occupancy, hide the latency there; half as many slots measured a few per
// cent slower on Poisson 256^2); SELL-64 batches two 4-entry groups for K = 2 and one for K = 4, 8.
// Register counts and occupancy: DESIGN.md §6.
template <int K>
constexpr int spmm_sb() { return K == 8 ? 4 : 8; }
template <int K>
constexpr int spmm_qb() { return K == 2 ? 2 : 1; }
// the layouts with a K-vector kernel: scalar SELL-DIA, 16-bit offsets, int32 columns
inline bool spmm_supported(const SellPattern& P) {
  return P.bs == 1 && (P.col_bits == kSellDia || P.col_bits == kSellOff16 || P.col_bits == kSellInt32);
}

// The one launch of every SELL kernel: y = epi(A gx) over pattern P with the value array `vals`
// (VT: its type), K = 1 vector or K interleaved ones (gx.x is then [n][K]).  Dispatches over the
// layout (col_bits, bs); a layout / gather / K combination without a kernel is an error
// (LSPCG_ERR_UNSUPPORTED), never a silent return.
// MINW, the workgroups per CU the registers must allow: 6 x 256 threads for the compact-value
// kernels over a plain vector (the resident reducing grid); 1 for fp64 values, the double-gather
// fused epilogues and the K-vector kernels, which need more registers than 6 per CU leaves.
template <typename T, typename VT, int K = 1, class Pro, class Gx, class Epi>
inline int launch_sell(const SellPattern& P, const void* vals, Gx gx, Pro pro, Epi epi, hipStream_t st,
                       bool one_tile_per_wg = false) {
  constexpr bool plain = std::is_same<Gx, GatherVec<T>>::value;
  constexpr int MINW = (K == 1 && sizeof(VT) == 4 && plain) ? 1536 / kSellWG : 1;
  LSPCG_CHECK(K == 1 || spmm_supported(P), LSPCG_ERR_UNSUPPORTED,
              "SELL launch: no K-vector kernel for view kind " + std::to_string(P.col_bits) + ", block size " +
                  std::to_string(P.bs));
  LSPCG_CHECK(plain || P.col_bits != kSellJagX, LSPCG_ERR_UNSUPPORTED,
              "SELL launch: a SELL-64X view stages a plain vector, not a fused gather");
  const int64_t grid = sell_grid(P, Epi::NDOT > 0, one_tile_per_wg);
  if (grid <= 0) return LSPCG_OK;
  const dim3 g{unsigned(grid)}, b{kSellWG};
  if (P.col_bits == kSellDia) {
    const SdiaArgs<VT> a = sdia_args<VT>(P, vals);
    // range-checked vector windows wherever the vector is a plain one and short enough (sdia_ranged)
    by_flag(plain && sdia_ranged(P, K), [&](auto ranged) {
      constexpr bool RANGED = plain && decltype(ranged)::value;
      if constexpr (K > 1) {
        LSPCG_LAUNCH_SPMV((k_spmm_sdia<T, VT, K, spmm_sb<K>(), kSellWG, RANGED, Pro, Epi>), g, b, 0, st, a, gx.x, pro,
                          epi);
      } else if (P.bs == 3) {
        LSPCG_LAUNCH_SPMV((k_spmv_bsdia3<T, VT, bsdia_sb<VT>(), kSellWG, MINW, Pro, Gx, Epi>), g, b, 0, st, a, pro, gx,
                          epi);
      } else {
        LSPCG_LAUNCH_SPMV((k_spmv_sdia<T, VT, kSdiaSB, kSellWG, MINW, RANGED, Pro, Gx, Epi>), g, b, 0, st, a, pro, gx,
                          epi);
      }
    });
    return LSPCG_OK;
  }
  if constexpr (K == 1) {
    if (P.jagged()) {
      const SellArgs<VT, int16_t> a = sell_args<VT, int16_t>(P, vals);
      by_flag(plain && P.col_bits == kSellJagX, [&](auto xs) {
        constexpr bool XS = plain && decltype(xs)::value;
        const size_t lds = XS ? size_t(P.kx) * kSellXBlk * sizeof(T) : 0;
        LSPCG_LAUNCH_SPMV((k_spmv_sellj<T, VT, LSPCG_JAG_QB, kSellWG, MINW, XS, Pro, Gx, Epi>), g, b, lds, st, a, pro,
                          gx, epi);
      });
      return LSPCG_OK;
    }
  }
  // SELL-64 by column word; BSELL-64 (bs 3) has 16-bit offsets or int32 columns
  auto sell64 = [&](auto ct) {
    using CT = decltype(ct);
    const SellArgs<VT, CT> a = sell_args<VT, CT>(P, vals);
    if constexpr (K == 1 && !std::is_same<CT, uint8_t>::value) {
      if (P.bs == 3) {
        LSPCG_LAUNCH_SPMV((k_spmv_bsell3<T, VT, CT, kBsellQB, kSellWG, MINW, Pro, Gx, Epi>), g, b, 0, st, a, pro, gx,
                          epi);
        return;
      }
    }
    constexpr int QB = K == 1 ? kSellQB : spmm_qb<K>();
    LSPCG_LAUNCH_SPMV((k_spmv_sell<T, VT, CT, QB, kSellWG, MINW, Pro, Gx, Epi, K>), g, b, 0, st, a, pro, gx, epi);
  };
  if constexpr (K == 1) {
    if (P.col_bits == kSellCoded) {
      sell64(uint8_t{});
      return LSPCG_OK;
    }
  }
  if (P.col_bits == kSellOff16) sell64(int16_t{});
  else sell64(int32_t{});
  return LSPCG_OK;
}

}  // namespace lspcg

// SELL copy attached to a matrix handle for the standalone SpMV (same values, same dtype)
// (reordered: the copy is of P A Pᵀ; lspcg_spmv gathers x into xs and the SpMV stores each row at
// its original place, EpiStorePerm; ys is unused)
struct SellCopy {
  lspcg::SellPattern P;
  void* vals = nullptr;
  lspcg::Reorder ro;
  lspcg_mat* Ap = nullptr;  // P A Pᵀ (owned), its rowptr is P.rowptr
  void* xs = nullptr;
  void* ys = nullptr;
  void release() {
    P.release();
    (void)hipFree(vals);
    vals = nullptr;
    ro.release();
    if (Ap) lspcg_mat_destroy(Ap);
    Ap = nullptr;
    (void)hipFree(xs);
    (void)hipFree(ys);
    xs = ys = nullptr;
  }
};

namespace lspcg {
// Host-side construction (lspcg_sell.hip), enqueued on `st`.
// Builds the SELL-64 pattern of a scalar CSR (n rows); fails with LSPCG_ERR_UNSUPPORTED when the
// padded size exceeds max_pad x nnz (irregular row lengths: the CSR kernel is used instead).
// cols (kSellCol16 | kSellColDia | kSellColCode | kSellColJag | kSellColXs): the column storages
// allowed besides int32.  The build tries them in this order, one function per layout (dia_try,
// code_try, jag_try + xs_try, plain_columns), and takes the first that applies:
//   SELL-DIA (kSellColDia) when every slice has <= 16 distinct offsets, every row is sorted and it
//     stores no more slots than the 4-entry groups would;
//   SELL-64C (kSellColCode, 16-bit offsets fit) when at least half of the slots fall in slices of
//     <= 64 distinct offsets;
//   SELL-64J (kSellColJag, 16-bit offsets fit) when SELL-64 would pad more than kSellJagPad x nnz and
//     no row has more than 64 entries -- the only layout left past max_pad; SELL-64X on top of it
//     (kSellColXs, n >= sellx_min_n()) when every 256-row tile reads <= kSellXMax x blocks;
//   16-bit offsets (kSellCol16) when they fit, else int32 columns.
// Host waits: one for the group total, one for (SELL-DIA fits, its slot total, 16-bit offsets fit)
// together, then one per later attempt (two for SELL-64C when taken).  On failure *out is untouched.
int sell_build_pattern(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* colind, double max_pad,
                       int cols, hipStream_t st, SellPattern* out);
// Allocates and fills the SELL value array of a CSR with the same pattern (*out == nullptr), or
// refills *out in place (an array of this pattern and dst_dtype).  src_dtype / dst_dtype:
// LSPCG_F32 or LSPCG_F64 (fp64 -> fp32 only for exactly representable values).
int sell_fill_values(const SellPattern& P, const int32_t* colind, const void* src, int src_dtype, int dst_dtype,
                     hipStream_t st, void** out);
// BSELL-64 pattern of a BSR 3x3 (nb block rows, nnzb blocks, sorted block columns); the same
// padding rule on block slots (64 x groups <= max_pad x nnzb) and 16-bit block-column offsets.
// allow_dia: BSELL-DIA (col_bits 1) when every slice has <= 16 distinct block offsets and it
// stores at most 1/16 more block slots than BSELL-64 (env LSPCG_BSDIA=0 turns it off: bsdia_allowed()).
int bsell_build_pattern(int64_t nb, int64_t nnzb, const int32_t* rowptr, const int32_t* colind, double max_pad,
                        bool allow16, bool allow_dia, hipStream_t st, SellPattern* out);
// SELL-64C for the solver's views of >= LSPCG_SELLC_MIN_N rows (env LSPCG_SELLC=0 turns it off): the
// byte codes pay where the loop streams matrix bytes; below, the decode's ds_bpermute in the gathers'
// dependency chain costs more than the bytes save (us per iteration, SELL-64C vs 16-bit: bunny 6.3 k
// rows 17.4 vs 16.6, kuhn41rcm 69 k 28.6 vs 27.1, kuhn64rcm 262 k 37.7 vs 37.4, kuhn80rcm 512 k 53.0 vs
// 55.5, kuhn101rcm 1 M 86.7 vs 90.2)
inline bool sellc_allowed(int64_t n) {
  const char* e = std::getenv("LSPCG_SELLC");
  if (e && e[0] == '0') return false;
  const char* m = std::getenv("LSPCG_SELLC_MIN_N");
  return n >= (m ? std::atoll(m) : int64_t(400000));
}
// smallest pattern that gets SELL-64X (kSellXMinN; env LSPCG_SELLX_MIN_N moves the floor, read at
// every pattern build: the tests lower it to reach the staged kernel at a few thousand rows)
inline int64_t sellx_min_n() {
  const char* m = std::getenv("LSPCG_SELLX_MIN_N");
  return m ? std::atoll(m) : kSellXMinN;
}
inline bool bsdia_allowed() {
  const char* e = std::getenv("LSPCG_BSDIA");
  return !(e && e[0] == '0');
}
// its block values (16-B lane chunks) from the BSR's [nnzb][3][3] array
int bsell_fill_values(const SellPattern& P, const void* src, int src_dtype, int dst_dtype, hipStream_t st, void** out);
}  // namespace lspcg
