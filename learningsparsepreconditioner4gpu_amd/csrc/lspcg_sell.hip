// SELL-64 view construction (layout and rationale: lspcg_sell.hpp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <memory>

#include "lspcg_sell.hpp"

namespace lspcg {

// ---- construction kernels --------------------------------------------------
// groups-per-row of each slice = ceil(max row length / 4)
__global__ void k_sell_len(int64_t n, int64_t ns, const int32_t* __restrict__ rowptr, int32_t* __restrict__ cnt) {
  const int64_t s = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= ns) return;
  const int64_t i = s * kSellC + lane;
  int len = i < n ? rowptr[i + 1] - rowptr[i] : 0;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) len = max(len, __shfl_xor(len, m, 64));
  if (lane == 0) cnt[s] = (len + 3) >> 2;
}

// Slot-parallel fill: one workgroup per slice, threads over the slice's 256·G destination slots
// in storage order (coalesced writes; the 4 slots of a row group read 4 consecutive entries of
// that row).  Slot p -> row 64s + (p % 256) / 4, entry 4 (p / 256) + p % 4.  Writes column
// indices (col32 / col16, whichever is non-null) and, if dst != nullptr, values; slots past a
// row's end (or of rows >= n) get value 0 and the padding column (-1 / kSellPad16), so every
// slot of the view is written.
template <typename VS, typename VD>
__global__ void __launch_bounds__(256) k_sell_fill(int64_t n, int64_t ns, const int32_t* __restrict__ gp,
                                                   const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ colind, const VS* __restrict__ src,
                                                   int32_t* __restrict__ col32, int16_t* __restrict__ col16,
                                                   VD* __restrict__ dst) {
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    const int64_t base = 256 * int64_t(gp[s]);
    const int32_t slots = 256 * (gp[s + 1] - gp[s]);
    for (int32_t p = threadIdx.x; p < slots; p += blockDim.x) {
      const int64_t i = s * kSellC + ((p & 255) >> 2);
      const int32_t k = 4 * (p >> 8) + (p & 3);
      int32_t b = 0, len = 0;
      if (i < n) {
        b = rowptr[i];
        len = rowptr[i + 1] - b;
      }
      const bool real = k < len;
      if (col32) col32[base + p] = real ? colind[b + k] : int32_t(-1);
      if (col16) col16[base + p] = real ? int16_t(colind[b + k] - int32_t(s * kSellC)) : kSellPad16;
      if (dst) dst[base + p] = real ? VD(src[b + k]) : VD(0);
    }
  }
}

// flag |= bit when some column is more than 32767 away from its slice's first row: the bit says
// that 16-bit offsets do NOT fit (the hosts' fits16 is its negation)
__global__ void k_sell_fit16(int64_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                             int* __restrict__ flag, int bit) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int32_t base = int32_t((i / kSellC) * kSellC);
    const int32_t b = rowptr[i], e = rowptr[i + 1];
    // every entry (rows need not be sorted: dist_pcg's extended matrices keep the global order)
    bool far = false;
    for (int32_t k = b; k < e; ++k) {
      const int32_t o = colind[k] - base;
      far |= o < -32767 || o > 32767;
    }
    if (far) atomicOr(flag, bit);
  }
}

// ---- SELL-DIA (layout: lspcg_sell.hpp kSdiaMax) ----------------------------------------------
// Dictionary of slice s: one wave merges its 64 rows' row-relative offsets col - row: every round
// takes the wave minimum m of the lanes' current heads, appends it and advances the lanes whose head
// equals m, so with sorted rows the dictionary comes out ascending and duplicate-free.  cnt[s] =
// D_s.  flag bit 0: some slice has more than 16 offsets, or some row is not sorted (a lane's next
// head not above the value it just consumed) -- no SELL-DIA.  flag[2]: the largest column (sorted
// rows: the largest last entry), one atomic per slice.
__global__ void k_sdia_dict(int64_t n, int64_t ns, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                            int32_t* __restrict__ dict, int32_t* __restrict__ cnt, int* __restrict__ flag) {
  const int64_t s = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= ns) return;  // wave-uniform
  const int64_t i = s * kSellC + lane;
  int32_t k = 0, e = 0;
  if (i < n) {
    k = rowptr[i];
    e = rowptr[i + 1];
  }
  int nd = 0, mine = 0;
  bool bad = false;
  int prev = INT_MIN;
  for (;;) {
    const int h = k < e ? int(int64_t(colind[k]) - i) : INT_MAX;
    bad |= k < e && h <= prev;  // unsorted (or duplicate) column in this row
    int m = h;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = min(m, __shfl_xor(m, d, 64));
    if (m == INT_MAX) break;
    if (nd == kSdiaMax) {
      bad = true;
      break;
    }
    if (lane == nd) mine = m;
    ++nd;
    if (h == m) {
      prev = h;
      ++k;
    }
  }
  if (__any(bad)) {
    if (lane == 0) atomicOr(flag, 1);
    return;
  }
  int top = e > 0 && i < n && rowptr[i] < e ? colind[e - 1] : 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) top = max(top, __shfl_xor(top, d, 64));
  if (lane == 0) atomicMax(flag + 2, top);
  if (lane < kSdiaMax) dict[kSdiaMax * s + lane] = lane < nd ? mine : 0;
  if (lane == 0) cnt[s] = nd;
}

// BSELL-DIA's row masks (block rows): bit j of row i <=> the row has the offset dict[16 s + j]
__global__ void k_bsdia_mask(int64_t n, int64_t ns, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                            const int32_t* __restrict__ dict, const int32_t* __restrict__ gp, uint16_t* __restrict__ mask) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < ns * kSellC; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t s = i / kSellC;
    unsigned m = 0;
    if (i < n) {
      const int nd = gp[s + 1] - gp[s];
      int j = 0;
      for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int off = int(int64_t(colind[k]) - i);
        while (j < nd && dict[kSdiaMax * s + j] != off) ++j;  // both ascending
        m |= 1u << j;
        ++j;
      }
    }
    mask[i] = uint16_t(m);
  }
}

// lane masks, one wave per slice: bit l of mask[16 s + j] <=> row 64 s + l has the offset
// dict[16 s + j] (one ballot per slot; the words of the slots past the slice's count are 0)
__global__ void __launch_bounds__(256) k_sdia_mask(int64_t n, int64_t ns, const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ colind, const int32_t* __restrict__ dict,
                                                   const int32_t* __restrict__ gp, uint64_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  for (int64_t s = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); s < ns; s += int64_t(gridDim.x) * 4) {  // wave-uniform
    const int64_t i = s * kSellC + lane;
    unsigned m = 0;
    if (i < n) {
      const int nd = gp[s + 1] - gp[s];
      int j = 0;
      for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int off = int(int64_t(colind[k]) - i);
        while (j < nd && dict[kSdiaMax * s + j] != off) ++j;  // both ascending
        m |= 1u << j;
        ++j;
      }
    }
#pragma unroll
    for (int j = 0; j < kSdiaMax; ++j) {
      const uint64_t word = __ballot((m >> j) & 1u);
      if (lane == j) mask[kSdiaMax * s + j] = word;
    }
  }
}

// row `lane` of a slice's 16 lane masks: bit j <=> the row has slot j
__device__ __forceinline__ unsigned sdia_row_mask(const uint64_t* __restrict__ words, int lane) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < kSdiaMax; ++j) m |= unsigned((words[j] >> lane) & 1u) << j;
  return m;
}

// values: slot j of row i holds the row's entry number popcount(mask & (2^j - 1)) when bit j is set
// (256 threads: a thread keeps its lane, so its row mask is gathered once per slice)
template <typename VS, typename VD>
__global__ void __launch_bounds__(256) k_sdia_fill(int64_t n, int64_t ns, const int32_t* __restrict__ gp,
                                                   const uint64_t* __restrict__ mask, const int32_t* __restrict__ rowptr,
                                                   const VS* __restrict__ src, VD* __restrict__ dst) {
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    const int64_t g0 = gp[s];
    const int32_t slots = kSellC * (gp[s + 1] - gp[s]);
    const unsigned m = sdia_row_mask(mask + kSdiaMax * s, threadIdx.x & 63);
    for (int32_t p = threadIdx.x; p < slots; p += blockDim.x) {
      const int lane = p & 63;
      const int j = p >> 6;
      const int64_t i = s * kSellC + lane;
      VD v = VD(0);
      if (i < n && ((m >> j) & 1u)) v = VD(src[rowptr[i] + __builtin_popcount(m & ((1u << j) - 1u))]);
      dst[kSellC * g0 + p] = v;
    }
  }
}

// ---- SELL-64C (layout: lspcg_sell.hpp kSellCodeMax) ------------------------------------------
// Dictionary of slice s: the distinct row-relative offsets col - row of its 64 rows, gathered in a
// per-wave LDS hash set (linear probing, 256 slots), so rows need not be sorted (a reordered solver's
// permuted rows keep their original entry order).  Entries are numbered in slot order: the order is
// immaterial -- a code only names its offset, and slot k stays entry k of its row, so the sum order
// is the CSR's.  dict[64 s + j] (0 past the count); raw[s] = the slice's groups when it has more
// than kSellCodeMax offsets (kept as 16-bit offsets), else 0.
constexpr int kSellcHash = 256;
constexpr int kSellcEmpty = INT_MIN;  // never an offset: |col - row| < 2^31 - 1
__global__ void __launch_bounds__(256) k_sellc_dict(int64_t n, int64_t ns, const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ colind, const int32_t* __restrict__ gp,
                                                    int32_t* __restrict__ dict, int32_t* __restrict__ raw) {
  __shared__ int tab[4][kSellcHash];
  __shared__ int dd[4][kSellCodeMax];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = int64_t(blockIdx.x) * 4 + w;
  if (s >= ns) return;  // wave-uniform; only this wave's tables are used below
  for (int j = lane; j < kSellcHash; j += 64) tab[w][j] = kSellcEmpty;
  dd[w][lane] = 0;
  __builtin_amdgcn_wave_barrier();
  const int64_t i = s * kSellC + lane;
  int32_t k = 0, e = 0;
  if (i < n) {
    k = rowptr[i];
    e = rowptr[i + 1];
  }
  bool over = false;
  for (; k < e && !over; ++k) {
    const int off = int(int64_t(colind[k]) - i);
    unsigned h = (unsigned(off) * 0x9E3779B1u) >> 24;  // 8 bits: kSellcHash slots
    int probe = 0;
    for (; probe < kSellcHash; ++probe) {
      const int prev = atomicCAS(&tab[w][h], kSellcEmpty, off);
      if (prev == kSellcEmpty || prev == off) break;
      h = (h + 1) & (kSellcHash - 1);
    }
    over = probe == kSellcHash;  // > 256 distinct offsets
  }
  __builtin_amdgcn_wave_barrier();
  int total = 0;
  for (int c = 0; c < kSellcHash / 64; ++c) {
    const int v = tab[w][64 * c + lane];
    const bool used = v != kSellcEmpty;
    const unsigned long long bal = __ballot(used);
    const int pos = total + __popcll(bal & ((1ull << lane) - 1ull));
    if (used && pos < kSellCodeMax) dd[w][pos] = v;
    total += __popcll(bal);
  }
  __builtin_amdgcn_wave_barrier();
  const bool raw_slice = __any(over) || total > kSellCodeMax;
  dict[kSellCodeMax * s + lane] = raw_slice ? 0 : dd[w][lane];
  if (lane == 0) raw[s] = raw_slice ? gp[s + 1] - gp[s] : 0;
}

// rgp[s] = the first col2 group of an uncoded slice (exclusive prefix of raw), -1 for a coded one
__global__ void k_sellc_rgp(int64_t ns, const int32_t* __restrict__ raw, const int32_t* __restrict__ rscan,
                            int32_t* __restrict__ rgp) {
  for (int64_t s = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < ns; s += int64_t(gridDim.x) * blockDim.x)
    rgp[s] = raw[s] ? rscan[s] : -1;
}

// codes (coded slices) or 16-bit offsets (the others), every slot written, in k_sell_fill's order
__global__ void __launch_bounds__(256) k_sellc_fill(int64_t n, int64_t ns, const int32_t* __restrict__ gp,
                                                    const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ colind, const int32_t* __restrict__ dict,
                                                    const int32_t* __restrict__ rgp, uint8_t* __restrict__ col8,
                                                    int16_t* __restrict__ col2) {
  __shared__ int32_t sd[kSellCodeMax];
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    __syncthreads();  // the previous slice's lookups are done
    if (threadIdx.x < kSellCodeMax) sd[threadIdx.x] = dict[kSellCodeMax * s + threadIdx.x];
    __syncthreads();
    const int32_t r0 = rgp[s];
    const int64_t base = 256 * int64_t(gp[s]);
    const int32_t slots = 256 * (gp[s + 1] - gp[s]);
    for (int32_t p = threadIdx.x; p < slots; p += blockDim.x) {
      const int64_t i = s * kSellC + ((p & 255) >> 2);
      const int32_t k = 4 * (p >> 8) + (p & 3);
      int32_t b = 0, len = 0;
      if (i < n) {
        b = rowptr[i];
        len = rowptr[i + 1] - b;
      }
      const bool real = k < len;
      if (r0 < 0) {
        uint8_t code = kSellCodePad;
        if (real) {
          const int off = int(int64_t(colind[b + k]) - i);
          int j = 0;
          while (j < kSellCodeMax - 1 && sd[j] != off) ++j;  // present, once: the dictionary is the slice's set
          code = uint8_t(j);
        }
        col8[base + p] = code;
      } else {
        col8[base + p] = kSellCodePad;
        col2[256 * int64_t(r0) + p] = real ? int16_t(colind[b + k] - int32_t(s * kSellC)) : kSellPad16;
      }
    }
  }
}

// ---- SELL-64J (layout: lspcg_sell.hpp kSellJag) ---------------------------------------------
// One wave per slice: the lanes' ranks by (row length descending, row ascending) -> lmap, the
// per-group lane counts -> jc, the slice's stored entries -> etot.  flag |= 1 when a row has more
// than 16 groups (64 entries): no jagged layout.
__global__ void k_jag_meta(int64_t n, int64_t ns, const int32_t* __restrict__ rowptr, uint8_t* __restrict__ lmap,
                           uint8_t* __restrict__ jc, int32_t* __restrict__ etot, int* __restrict__ flag) {
  const int64_t s = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= ns) return;  // wave-uniform
  const int64_t i = s * kSellC + lane;
  const int len = i < n ? rowptr[i + 1] - rowptr[i] : 0;
  const int g = (len + 3) >> 2;
  if (__any(g > kSellJagMaxG)) {
    if (lane == 0) atomicOr(flag, 1);
    return;
  }
  int rank = 0;
  for (int j = 0; j < 64; ++j) {
    const int lj = __shfl(len, j, 64);
    rank += (lj > len) || (lj == len && j < lane);
  }
  lmap[kSellC * s + rank] = uint8_t(lane);
  int total = 0;
#pragma unroll
  for (int q = 0; q < kSellJagMaxG; ++q) {
    const int c = __popcll(__ballot(g > q));
    if (lane == q) jc[kSellJagMaxG * s + q] = uint8_t(c);
    total += c;
  }
  if (lane == 0) etot[s] = 4 * total;
}

// Element-parallel fill: one workgroup per slice, threads over its stored entries in storage order
// (coalesced writes): element p of the slice -> group q (the counts' prefix in LDS), lane (p - start_q)
// / 4, entry 4 q + p % 4 of that lane's row.  16-bit offsets (col16) and / or values (dst); entries
// past the row's end get kSellPad16 / 0.
template <typename VS, typename VD>
__global__ void __launch_bounds__(256) k_jag_fill(int64_t n, int64_t ns, const int32_t* __restrict__ gp,
                                                  const uint8_t* __restrict__ jc, const uint8_t* __restrict__ lmap,
                                                  const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                  const VS* __restrict__ src, int16_t* __restrict__ col16,
                                                  VD* __restrict__ dst) {
  __shared__ int32_t start[kSellJagMaxG + 1];
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    __syncthreads();  // the previous slice's lookups are done
    if (threadIdx.x == 0) {
      int32_t e = 0;
      for (int q = 0; q < kSellJagMaxG; ++q) {
        start[q] = e;
        e += 4 * jc[kSellJagMaxG * s + q];
      }
      start[kSellJagMaxG] = e;
    }
    __syncthreads();
    const int64_t e0 = gp[s];
    const int32_t total = start[kSellJagMaxG];
    for (int32_t p = threadIdx.x; p < total; p += blockDim.x) {
      int q = 0;
      while (q + 1 < kSellJagMaxG && start[q + 1] <= p) ++q;
      const int l = (p - start[q]) >> 2;
      const int64_t i = s * kSellC + lmap[kSellC * s + l];
      const int32_t k = 4 * q + (p & 3);
      int32_t b = 0, len = 0;
      if (i < n) {
        b = rowptr[i];
        len = rowptr[i + 1] - b;
      }
      const bool real = k < len;
      if (col16) col16[e0 + p] = real ? int16_t(colind[b + k] - int32_t(s * kSellC)) : kSellPad16;
      if (dst) dst[e0 + p] = real ? VD(src[b + k]) : VD(0);
    }
  }
}

// ---- SELL-64X (layout: lspcg_sell.hpp kSellJagX) --------------------------------------------
// The distinct x blocks (col / 16) of one 256-row tile in an LDS hash set (one workgroup per tile,
// one row per thread); returns the count, or kSellXMax + 1 once the set outgrows the limit.
constexpr int kXsHash = 1024;
__device__ int xs_tile_set(int64_t n, int64_t tile, const int32_t* __restrict__ rowptr,
                           const int32_t* __restrict__ colind, int* tab, int* count, int* maxcol = nullptr) {
  for (int j = threadIdx.x; j < kXsHash; j += blockDim.x) tab[j] = -1;
  if (threadIdx.x == 0) *count = 0;
  __syncthreads();
  const int64_t i = tile * kSellWG + threadIdx.x;
  if (i < n) {
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int b = colind[k] / kSellXBlk;
      if (maxcol) atomicMax(maxcol, colind[k]);
      unsigned h = (unsigned(b) * 0x9E3779B1u) >> 22;  // 10 bits
      for (int probe = 0; probe < kXsHash; ++probe, h = (h + 1) & (kXsHash - 1)) {
        const int prev = atomicCAS(&tab[h], -1, b);
        if (prev == -1) {
          atomicAdd(count, 1);
          break;
        }
        if (prev == b) break;
      }
      if (*count > kSellXMax) break;  // (racy read: only ends the insertion early, the flag follows)
    }
  }
  __syncthreads();
  return *count;
}

__global__ void __launch_bounds__(256) k_xs_count(int64_t n, int64_t ntiles, const int32_t* __restrict__ rowptr,
                                                  const int32_t* __restrict__ colind, int32_t* __restrict__ cnt,
                                                  int* __restrict__ flag) {
  __shared__ int tab[kXsHash];
  __shared__ int count;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int c = xs_tile_set(n, t, rowptr, colind, tab, &count, flag + 3);
    if (threadIdx.x == 0) {
      cnt[t] = c;
      if (c > kSellXMax) atomicOr(flag, 1);
      atomicMax(flag + 1, c);
    }
    __syncthreads();
  }
}

// The tile's ascending block list (xl at xlp[t]) and every stored entry's word: slot * 16 + col % 16
// (the jagged storage order of k_jag_fill; padding keeps kSellPad16).
__global__ void __launch_bounds__(256) k_xs_fill(int64_t n, int64_t ns, int64_t ntiles, const int32_t* __restrict__ rowptr,
                                                 const int32_t* __restrict__ colind, const int32_t* __restrict__ xlp,
                                                 const int32_t* __restrict__ gp, const uint8_t* __restrict__ jc,
                                                 const uint8_t* __restrict__ lmap, int32_t* __restrict__ xl,
                                                 int16_t* __restrict__ code) {
  __shared__ int tab[kXsHash];
  __shared__ int sorted[kSellXMax];
  __shared__ int count;
  __shared__ int32_t start[kSellJagMaxG + 1];
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int c = xs_tile_set(n, t, rowptr, colind, tab, &count);
    for (int j = threadIdx.x; j < kXsHash; j += blockDim.x) {  // rank = number of smaller keys
      const int b = tab[j];
      if (b < 0) continue;
      int r = 0;
      for (int k = 0; k < kXsHash; ++k) r += (tab[k] >= 0 && tab[k] < b);
      sorted[r] = b;
      xl[xlp[t] + r] = b;
    }
    __syncthreads();
    for (int w = 0; w < kSellWG / kSellC; ++w) {
      const int64_t s = t * (kSellWG / kSellC) + w;
      if (s >= ns) break;  // uniform
      if (threadIdx.x == 0) {
        int32_t e = 0;
        for (int q = 0; q < kSellJagMaxG; ++q) {
          start[q] = e;
          e += 4 * jc[kSellJagMaxG * s + q];
        }
        start[kSellJagMaxG] = e;
      }
      __syncthreads();
      const int64_t e0 = gp[s];
      for (int32_t p = threadIdx.x; p < start[kSellJagMaxG]; p += blockDim.x) {
        int q = 0;
        while (q + 1 < kSellJagMaxG && start[q + 1] <= p) ++q;
        const int64_t i = s * kSellC + lmap[kSellC * s + ((p - start[q]) >> 2)];
        const int32_t k = 4 * q + (p & 3);
        int16_t word = kSellPad16;
        if (i < n && k < rowptr[i + 1] - rowptr[i]) {
          const int col = colind[rowptr[i] + k];
          const int b = col / kSellXBlk;
          int lo = 0, hi = c - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sorted[mid] < b) lo = mid + 1;
            else hi = mid;
          }
          word = int16_t(lo * kSellXBlk + col % kSellXBlk);
        }
        code[e0 + p] = word;
      }
      __syncthreads();  // start[] is rewritten for the next slice
    }
  }
}


// ---- BSELL-64 (BSR 3x3) ----------------------------------------------------------
// block slots per row of each slice = its longest block row
__global__ void k_bsell_len(int64_t nb, int64_t ns, const int32_t* __restrict__ rowptr, int32_t* __restrict__ cnt) {
  const int64_t s = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= ns) return;
  const int64_t I = s * kSellC + lane;
  int len = I < nb ? rowptr[I + 1] - rowptr[I] : 0;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) len = max(len, __shfl_xor(len, m, 64));
  if (lane == 0) cnt[s] = len;
}

// one workgroup per slice, threads over its 64 x G slots in storage order: slot p -> block row
// 64 s + p % 64, block q = p / 64; columns and/or the 9 values in 16-B lane chunks (padding: value 0,
// padding column)
template <typename VS, typename VD>
__global__ void __launch_bounds__(256) k_bsell_fill(int64_t nb, int64_t ns, const int32_t* __restrict__ gp,
                                                    const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ colind, const VS* __restrict__ src,
                                                    int32_t* __restrict__ col32, int16_t* __restrict__ col16,
                                                    VD* __restrict__ dst) {
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    const int64_t g0 = gp[s];
    const int32_t slots = 64 * (gp[s + 1] - gp[s]);
    for (int32_t p = threadIdx.x; p < slots; p += blockDim.x) {
      const int lane = p & 63;
      const int32_t q = p >> 6;
      const int64_t I = s * kSellC + lane;
      int32_t b = 0, len = 0;
      if (I < nb) {
        b = rowptr[I];
        len = rowptr[I + 1] - b;
      }
      const bool real = q < len;
      if (col32) col32[64 * g0 + p] = real ? colind[b + q] : int32_t(-1);
      if (col16) col16[64 * g0 + p] = real ? int16_t(colind[b + q] - int32_t(s * kSellC)) : kSellPad16;
      if (dst) {
#pragma unroll
        for (int v = 0; v < 9; ++v)
          dst[576 * (g0 + q) + bsell_pos<VD>(v, lane)] = real ? VD(src[9 * (int64_t(b) + q) + v]) : VD(0);
      }
    }
  }
}

// BSELL-DIA values: slot j of block row I holds the row's block number popcount(mask & (2^j - 1))
// when bit j is set (9 values in the BSELL-64 16-B lane chunks), zeros otherwise
template <typename VS, typename VD>
__global__ void __launch_bounds__(256) k_bsdia_fill(int64_t nb, int64_t ns, const int32_t* __restrict__ gp,
                                                    const uint16_t* __restrict__ mask, const int32_t* __restrict__ rowptr,
                                                    const VS* __restrict__ src, VD* __restrict__ dst) {
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    const int64_t g0 = gp[s];
    const int32_t slots = kSellC * (gp[s + 1] - gp[s]);
    for (int32_t p = threadIdx.x; p < slots; p += blockDim.x) {
      const int lane = p & 63;
      const int j = p >> 6;
      const int64_t I = s * kSellC + lane;
      const unsigned m = mask[I];
      const bool real = I < nb && ((m >> j) & 1u);
      const int64_t b = real ? int64_t(rowptr[I]) + __builtin_popcount(m & ((1u << j) - 1u)) : 0;
#pragma unroll
      for (int v = 0; v < 9; ++v) dst[576 * (g0 + j) + bsell_pos<VD>(v, lane)] = real ? VD(src[9 * b + v]) : VD(0);
    }
  }
}

// ---- the view builder (host) -----------------------------------------------------------------
// Scratch comes from a DevBuf and dies at scope exit; an array a layout keeps is handed to the
// SellPattern with keep().  Every host wait of a build is a read_words() or an explicit
// hipStreamSynchronize in this section.
static int slice_grid(int64_t ns) { return int(std::max<int64_t>(1, std::min<int64_t>(ns, 16384))); }
static int fill_grid(int64_t n) {
  return int(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, kElemBlocksMax)));
}

// The pattern under construction: released on scope exit unless commit() handed it to *out, so a
// failed build leaves *out untouched and frees everything P owned.
struct Building {
  SellPattern P;
  bool committed = false;
  int commit(SellPattern* out) {
    *out = P;
    committed = true;
    return LSPCG_OK;
  }
  ~Building() {
    if (!committed) P.release();
  }
};

template <typename T>
static void replace(T*& slot, T* v) {  // slot = v, freeing the array it held
  (void)hipFree(slot);
  slot = v;
}

// prefix[0..m] = exclusive sum of cnt[0..m] (prefix[m]: the total), enqueued; the total also goes to
// the device word *total_dev (a flag read fused with it) and / or to *total_host (valid after the
// caller's wait) where given.
static int scan_counts(int32_t* cnt, int32_t* prefix, int64_t m, DevBuf& B, hipStream_t st, int* total_dev,
                       int32_t* total_host) {
  size_t tb = 0;
  void* tmp = nullptr;
  LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, prefix, int(m + 1), st));  // size query
  if (int rc = B.get(reinterpret_cast<uint8_t**>(&tmp), tb)) return rc;
  LSPCG_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, prefix, int(m + 1), st));
  if (total_dev) LSPCG_HIP(hipMemcpyAsync(total_dev, prefix + m, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (total_host) LSPCG_HIP(hipMemcpyAsync(total_host, prefix + m, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  return LSPCG_OK;
}

// `count` device words to the host: a host wait
static int read_words(int* host, const int* dev, int count, hipStream_t st) {
  LSPCG_HIP(hipMemcpyAsync(host, dev, count * sizeof(int), hipMemcpyDeviceToHost, st));
  LSPCG_HIP(hipStreamSynchronize(st));
  return LSPCG_OK;
}

// Head of the scalar and the block build (P: n, nb, bs, ns, rowptr set): the slices' groups (bs 1) /
// block slots (bs 3) per row, their prefix P->gp and total P->groups (one host wait), and whether
// the padded slots exceed max_pad x nnz.
static int build_head(int64_t nnz, double max_pad, hipStream_t st, SellPattern* P, bool* overpad) {
  DevBuf B;
  int32_t* cnt = nullptr;
  int32_t groups = 0;
  if (int rc = B.get(&cnt, P->ns + 1)) return rc;
  LSPCG_HIP(hipMalloc(&P->gp, sizeof(int32_t) * (P->ns + 1)));
  LSPCG_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (P->ns + 1), st));
  const dim3 g(unsigned((P->ns + 3) / 4)), b(256);
  if (P->ns && P->bs == 3) hipLaunchKernelGGL(k_bsell_len, g, b, 0, st, P->nb, P->ns, P->rowptr, cnt);
  else if (P->ns) hipLaunchKernelGGL(k_sell_len, g, b, 0, st, P->nb, P->ns, P->rowptr, cnt);
  if (int rc = scan_counts(cnt, P->gp, P->ns, B, st, nullptr, &groups)) return rc;
  LSPCG_HIP(hipStreamSynchronize(st));
  P->groups = groups;
  *overpad = double(P->bs == 3 ? 64 : 256) * double(groups) > max_pad * double(std::max<int64_t>(nnz, 1));
  return LSPCG_OK;
}

// SELL-DIA / BSELL-DIA attempt on P's row graph (k_sdia_dict and k_sdia_mask run on block rows and
// block columns for bs 3), in two halves so that the caller fetches flag together with whatever else
// it asked the device, in one host wait.  dia_enqueue: the slices' dictionaries, their sizes' prefix;
// flag[0] |= 1 when there is no such layout (k_sdia_dict), flag[1] = its slot total, flag[2] = the
// largest column (of the row graph).
struct DiaScratch {
  int32_t* dict = nullptr;
  int32_t* gp = nullptr;
};
static int dia_enqueue(const SellPattern& P, const int32_t* colind, int* flag, DevBuf& B, hipStream_t st,
                       DiaScratch* D) {
  int32_t* cnt = nullptr;
  if (int rc = B.get(&D->dict, kSdiaMax * P.ns) | B.get(&cnt, P.ns + 1) | B.get(&D->gp, P.ns + 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (P.ns + 1), st));
  hipLaunchKernelGGL(k_sdia_dict, dim3(unsigned((P.ns + 3) / 4)), dim3(256), 0, st, P.nb, P.ns, P.rowptr, colind,
                     D->dict, cnt, flag);
  return scan_counts(cnt, D->gp, P.ns, B, st, flag + 1, nullptr);
}
// dia_try, with the host's copy of flag: *taken = true when the layout exists and stores at most
// `budget` slots; P then holds it (gp, dict, groups, the lane masks in col, xn).  B is the attempt's scratch
// (the caller's flag included): when taken it is freed here, before the mask kernel is enqueued, so
// that no hipFree waits behind that kernel.
static int dia_try(const int32_t* colind, const DiaScratch& D, const int* flag_h, int64_t budget, DevBuf& B,
                   hipStream_t st, SellPattern* P, bool* taken) {
  *taken = !(flag_h[0] & 1) && int64_t(flag_h[1]) <= budget;
  if (!*taken) return LSPCG_OK;
  replace(P->gp, B.keep(D.gp));
  P->dict = B.keep(D.dict);
  P->groups = flag_h[1];
  P->col_bits = 1;
  P->xn = int64_t(P->bs) * (int64_t(flag_h[2]) + 1);
  // 128 B per slice either way: 16 lane masks (SELL-DIA) or 64 row masks (BSELL-DIA)
  LSPCG_HIP(hipMalloc(&P->col, sizeof(uint64_t) * kSdiaMax * std::max<int64_t>(P->ns, 1)));
  B.release();
  if (P->bs == 3)
    hipLaunchKernelGGL(k_bsdia_mask, dim3(fill_grid(P->ns * kSellC)), dim3(kThreads), 0, st, P->nb, P->ns, P->rowptr,
                       colind, P->dict, P->gp, static_cast<uint16_t*>(P->col));
  else
    hipLaunchKernelGGL(k_sdia_mask, dim3(slice_grid((P->ns + 3) / 4)), dim3(256), 0, st, P->nb, P->ns, P->rowptr, colind,
                       P->dict, P->gp, static_cast<uint64_t*>(P->col));
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

// SELL-64C from the SELL-64 pattern (16-bit offsets fit): *taken = true when at least half of the
// slots lie in slices of <= 64 distinct offsets.
static int code_try(const int32_t* colind, hipStream_t st, SellPattern* P, bool* taken) {
  *taken = false;
  const int64_t ns = P->ns;
  DevBuf B;
  int32_t *dict = nullptr, *raw = nullptr, *rscan = nullptr;
  int32_t rawg = 0;
  if (int rc = B.get(&dict, kSellCodeMax * ns) | B.get(&raw, ns + 1) | B.get(&rscan, ns + 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(raw, 0, sizeof(int32_t) * (ns + 1), st));
  hipLaunchKernelGGL(k_sellc_dict, dim3(unsigned((ns + 3) / 4)), dim3(256), 0, st, P->n, ns, P->rowptr, colind, P->gp,
                     dict, raw);
  if (int rc = scan_counts(raw, rscan, ns, B, st, nullptr, &rawg)) return rc;
  LSPCG_HIP(hipStreamSynchronize(st));
  if (int64_t(rawg) * 2 > P->groups) return LSPCG_OK;
  P->dict = B.keep(dict);
  LSPCG_HIP(hipMalloc(&P->rgp, sizeof(int32_t) * ns));
  LSPCG_HIP(hipMalloc(&P->col, std::max<size_t>(size_t(256) * size_t(P->groups), 1)));
  LSPCG_HIP(hipMalloc(&P->col2, sizeof(int16_t) * std::max<size_t>(size_t(256) * size_t(rawg), 1)));
  hipLaunchKernelGGL(k_sellc_rgp, dim3(fill_grid(ns)), dim3(kThreads), 0, st, ns, raw, rscan, P->rgp);
  hipLaunchKernelGGL(k_sellc_fill, dim3(slice_grid(ns)), dim3(256), 0, st, P->n, ns, P->gp, P->rowptr, colind, P->dict,
                     P->rgp, static_cast<uint8_t*>(P->col), P->col2);
  LSPCG_HIP(hipGetLastError());
  LSPCG_HIP(hipStreamSynchronize(st));  // raw / rscan, which k_sellc_rgp reads, are freed on return
  P->col_bits = 8;
  *taken = true;
  return LSPCG_OK;
}

// SELL-64J from the SELL-64 pattern (16-bit offsets fit): *taken = true when every row has <= 64
// entries; P's gp becomes the element prefix, col the jagged 16-bit offsets.
static int jag_try(const int32_t* colind, hipStream_t st, SellPattern* P, bool* taken) {
  *taken = false;
  const int64_t ns = P->ns;
  DevBuf B;
  int32_t *etot = nullptr, *egp = nullptr;
  uint8_t *lmap = nullptr, *jc = nullptr;
  int* flag = nullptr;
  int flag_h[2] = {1, 0};  // [a row of more than 64 entries, stored entries]
  if (int rc = B.get(&flag, 2) | B.get(&etot, ns + 1) | B.get(&egp, ns + 1) | B.get(&lmap, kSellC * ns) |
               B.get(&jc, kSellJagMaxG * ns))
    return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, 2 * sizeof(int), st));
  LSPCG_HIP(hipMemsetAsync(etot, 0, sizeof(int32_t) * (ns + 1), st));
  hipLaunchKernelGGL(k_jag_meta, dim3(unsigned((ns + 3) / 4)), dim3(256), 0, st, P->n, ns, P->rowptr, lmap, jc, etot,
                     flag);
  if (int rc = scan_counts(etot, egp, ns, B, st, flag + 1, nullptr)) return rc;
  if (int rc = read_words(flag_h, flag, 2, st)) return rc;
  if (flag_h[0] & 1) return LSPCG_OK;
  replace(P->gp, B.keep(egp));
  P->lmap = B.keep(lmap);
  P->jc = B.keep(jc);
  P->elems = flag_h[1];
  P->col_bits = kSellJag;
  LSPCG_HIP(hipMalloc(&P->col, sizeof(int16_t) * std::max<int64_t>(P->elems, 1)));
  hipLaunchKernelGGL((k_jag_fill<float, float>), dim3(slice_grid(ns)), dim3(256), 0, st, P->n, ns, P->gp, P->jc, P->lmap,
                     P->rowptr, colind, static_cast<const float*>(nullptr), static_cast<int16_t*>(P->col),
                     static_cast<float*>(nullptr));
  LSPCG_HIP(hipGetLastError());
  *taken = true;
  return LSPCG_OK;
}

// SELL-64X from a SELL-64J pattern: *taken = true when every 256-row tile touches <= kSellXMax x
// blocks; the column words are rewritten as LDS positions, the tiles' block lists added.
static int xs_try(const int32_t* colind, hipStream_t st, SellPattern* P, bool* taken) {
  *taken = false;
  const int64_t n = P->n, ntiles = (n + kSellWG - 1) / kSellWG;
  DevBuf B;
  int32_t *cnt = nullptr, *xlp = nullptr;
  int* flag = nullptr;
  int flag_h[4] = {1, 0, 0, 0};  // [over the limit, longest list, total, largest column]
  if (int rc = B.get(&flag, 4) | B.get(&cnt, ntiles + 1) | B.get(&xlp, ntiles + 1)) return rc;
  LSPCG_HIP(hipMemsetAsync(flag, 0, 4 * sizeof(int), st));
  LSPCG_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (ntiles + 1), st));
  const int grid = int(std::max<int64_t>(1, std::min<int64_t>(ntiles, 8192)));
  hipLaunchKernelGGL(k_xs_count, dim3(grid), dim3(256), 0, st, n, ntiles, P->rowptr, colind, cnt, flag);
  if (int rc = scan_counts(cnt, xlp, ntiles, B, st, flag + 2, nullptr)) return rc;
  if (int rc = read_words(flag_h, flag, 4, st)) return rc;
  if (flag_h[0] & 1) return LSPCG_OK;
  P->xlp = B.keep(xlp);
  P->kx = flag_h[1];
  P->xn = int64_t(flag_h[3]) + 1;
  P->col_bits = kSellJagX;
  LSPCG_HIP(hipMalloc(&P->xl, sizeof(int32_t) * std::max(flag_h[2], 1)));
  hipLaunchKernelGGL(k_xs_fill, dim3(grid), dim3(256), 0, st, n, P->ns, ntiles, P->rowptr, colind, P->xlp, P->gp, P->jc,
                     P->lmap, P->xl, static_cast<int16_t*>(P->col));
  LSPCG_HIP(hipGetLastError());
  *taken = true;
  return LSPCG_OK;
}

// SELL-64 / BSELL-64 columns: 16-bit offsets from the slice's first row when they fit, else int32
// columns.  The fill writes every slot, padding included.
static int plain_columns(const int32_t* colind, bool fits16, hipStream_t st, SellPattern* P) {
  P->col_bits = fits16 ? 16 : 32;
  const int64_t slots = (P->bs == 3 ? 64 : 256) * P->groups;
  LSPCG_HIP(hipMalloc(&P->col, size_t(P->col_bits / 8) * size_t(std::max<int64_t>(slots, 1))));
  int32_t* c32 = fits16 ? nullptr : static_cast<int32_t*>(P->col);
  int16_t* c16 = fits16 ? static_cast<int16_t*>(P->col) : nullptr;
  const float* nosrc = nullptr;
  float* nodst = nullptr;
  const dim3 g(slice_grid(P->ns)), b(256);
  if (P->ns && P->bs == 3)
    hipLaunchKernelGGL((k_bsell_fill<float, float>), g, b, 0, st, P->nb, P->ns, P->gp, P->rowptr, colind, nosrc, c32, c16,
                       nodst);
  else if (P->ns)
    hipLaunchKernelGGL((k_sell_fill<float, float>), g, b, 0, st, P->n, P->ns, P->gp, P->rowptr, colind, nosrc, c32, c16,
                       nodst);
  LSPCG_HIP(hipGetLastError());
  return LSPCG_OK;
}

// The rule, top to bottom (lspcg_sell.hpp, above the declaration).  Host waits: the head, one read
// of (SELL-DIA fits, its slot total, 16-bit offsets fit), then one or two per later attempt.
int sell_build_pattern(int64_t n, int64_t nnz, const int32_t* rowptr, const int32_t* colind, double max_pad,
                       int cols, hipStream_t st, SellPattern* out) {
  Building W;
  SellPattern& P = W.P;
  P.n = n;
  P.nb = n;
  P.ns = (n + kSellC - 1) / kSellC;
  P.rowptr = rowptr;
  bool overpad = false, taken = false;
  if (int rc = build_head(nnz, max_pad, st, &P, &overpad)) return rc;
  auto reject = [] {
    set_error("sell: padding exceeds the limit (irregular row lengths)");
    return LSPCG_ERR_UNSUPPORTED;
  };
  // padding past max_pad: only the jagged layout (which pads just each row's last group) may remain
  if (overpad && !(cols & kSellColJag)) return reject();
  if (overpad) cols &= ~(kSellColDia | kSellColCode);
  bool fits16 = cols & kSellCol16;  // every column within 32767 of its slice's first row
  if (n) {
    DevBuf B;
    DiaScratch D;
    int* flag = nullptr;     // [bit 0: no SELL-DIA, bit 1: some offset beyond 16 bits | SELL-DIA slots | its largest column]
    int flag_h[3] = {1, 0, 0};
    if (int rc = B.get(&flag, 3)) return rc;
    LSPCG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flag), (cols & kSellColDia) ? 0 : 1, 1, st));
    LSPCG_HIP(hipMemsetAsync(flag + 1, 0, 2 * sizeof(int), st));
    if (cols & kSellColDia)
      if (int rc = dia_enqueue(P, colind, flag, B, st, &D)) return rc;
    if (cols & kSellCol16)
      hipLaunchKernelGGL(k_sell_fit16, dim3(fill_grid(n)), dim3(kThreads), 0, st, n, rowptr, colind, flag, 2);
    if (int rc = read_words(flag_h, flag, 3, st)) return rc;
    fits16 = fits16 && !(flag_h[0] & 2);
    // SELL-DIA when it fits and stores no more slots than the 4-entry groups
    if (int rc = dia_try(colind, D, flag_h, 4 * P.groups, B, st, &P, &taken)) return rc;
    if (taken) return W.commit(out);
  }
  if ((cols & kSellColCode) && fits16 && n && P.groups > 0) {
    if (int rc = code_try(colind, st, &P, &taken)) return rc;
    if (taken) return W.commit(out);
  }
  // irregular row lengths: the jagged layout stores ~1.1 x nnz instead
  if ((cols & kSellColJag) && fits16 && n && double(256) * double(P.groups) > kSellJagPad * double(nnz)) {
    if (int rc = jag_try(colind, st, &P, &taken)) return rc;
    if (taken && (cols & kSellColXs) && n >= sellx_min_n()) {  // stage each tile's x blocks in LDS where they fit
      bool xs = false;
      if (int rc = xs_try(colind, st, &P, &xs)) return rc;
    }
    if (taken) return W.commit(out);
  }
  if (overpad) return reject();
  if (int rc = plain_columns(colind, fits16, st, &P)) return rc;
  return W.commit(out);
}

int bsell_build_pattern(int64_t nb, int64_t nnzb, const int32_t* rowptr, const int32_t* colind, double max_pad,
                        bool allow16, bool allow_dia, hipStream_t st, SellPattern* out) {
  Building W;
  SellPattern& P = W.P;
  P.n = 3 * nb;
  P.nb = nb;
  P.bs = 3;
  P.ns = (nb + kSellC - 1) / kSellC;
  P.rowptr = rowptr;
  bool overpad = false, taken = false;
  if (int rc = build_head(nnzb, max_pad, st, &P, &overpad)) return rc;
  if (overpad) {
    set_error("bsell: padding exceeds the limit (irregular block-row lengths)");
    return LSPCG_ERR_UNSUPPORTED;
  }
  if (allow_dia && nb) {
    DevBuf B;
    DiaScratch D;
    int* flag = nullptr;
    int flag_h[3] = {1, 0, 0};  // [no BSELL-DIA, BSELL-DIA slots, largest block column]
    if (int rc = B.get(&flag, 3)) return rc;
    LSPCG_HIP(hipMemsetAsync(flag, 0, 3 * sizeof(int), st));
    if (int rc = dia_enqueue(P, colind, flag, B, st, &D)) return rc;
    if (int rc = read_words(flag_h, flag, 3, st)) return rc;
    // a slice whose distinct offsets outnumber its longest row pads a little more than BSELL-64
    // (C4: 24,574 vs 24,572 slots); the column loads it drops are worth up to 1/16 more slots
    if (int rc = dia_try(colind, D, flag_h, P.groups + P.groups / 16, B, st, &P, &taken)) return rc;
    if (taken) return W.commit(out);
  }
  bool fits16 = false;  // every block column within 32767 of its slice's first block row
  if (allow16 && nb) {
    DevBuf B;
    int* flag = nullptr;
    int far = 1;
    if (int rc = B.get(&flag, 1)) return rc;
    LSPCG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_sell_fit16, dim3(fill_grid(nb)), dim3(kThreads), 0, st, nb, rowptr, colind, flag, 1);
    if (int rc = read_words(&far, flag, 1, st)) return rc;
    fits16 = far == 0;
  }
  if (int rc = plain_columns(colind, fits16, st, &P)) return rc;
  return W.commit(out);
}

// f(VS(), VD()) with the value types of (src_dtype, dst_dtype), each LSPCG_F32 or LSPCG_F64
template <class F>
static void with_value_types(int src_dtype, int dst_dtype, F f) {
  if (src_dtype == LSPCG_F64 && dst_dtype == LSPCG_F64) f(double(), double());
  else if (src_dtype == LSPCG_F64 && dst_dtype == LSPCG_F32) f(double(), float());
  else if (src_dtype == LSPCG_F32 && dst_dtype == LSPCG_F32) f(float(), float());
  else f(float(), double());
}

// the zeroed surplus slots behind a new value array (slice-diagonal layouts: kSdiaPadSlots)
static int zero_surplus(const SellPattern& P, void* v, size_t es, hipStream_t st) {
  if (P.alloc_slots() > P.slots())
    LSPCG_HIP(hipMemsetAsync(static_cast<char*>(v) + es * P.slots(), 0, es * (P.alloc_slots() - P.slots()), st));
  return LSPCG_OK;
}

int sell_fill_values(const SellPattern& P, const int32_t* colind, const void* src, int src_dtype, int dst_dtype,
                     hipStream_t st, void** out) {
  const size_t es = dst_dtype == LSPCG_F32 ? 4 : 8;
  void* v = *out;  // an existing array of this pattern and dtype is refilled in place
  const bool mine = v == nullptr;
  if (!v) {
    LSPCG_HIP(hipMalloc(&v, es * std::max<int64_t>(P.alloc_slots(), 1)));
    if (int rc = zero_surplus(P, v, es, st)) {
      (void)hipFree(v);
      return rc;
    }
  }
  const dim3 g(slice_grid(P.ns)), b(256);
  if (P.ns)
    with_value_types(src_dtype, dst_dtype, [&](auto vs, auto vd) {
      using VS = decltype(vs);
      using VD = decltype(vd);
      const VS* s = static_cast<const VS*>(src);
      VD* d = static_cast<VD*>(v);
      int32_t* no32 = nullptr;
      int16_t* no16 = nullptr;
      if (P.jagged())
        hipLaunchKernelGGL((k_jag_fill<VS, VD>), g, b, 0, st, P.n, P.ns, P.gp, P.jc, P.lmap, P.rowptr, colind, s, no16, d);
      else if (P.col_bits == 1)
        hipLaunchKernelGGL((k_sdia_fill<VS, VD>), g, b, 0, st, P.n, P.ns, P.gp, static_cast<const uint64_t*>(P.col),
                           P.rowptr, s, d);
      else
        hipLaunchKernelGGL((k_sell_fill<VS, VD>), g, b, 0, st, P.n, P.ns, P.gp, P.rowptr, colind, s, no32, no16, d);
    });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    if (mine) (void)hipFree(v);
    set_error(std::string("sell_fill_values: ") + hipGetErrorString(e));
    return LSPCG_ERR_HIP;
  }
  *out = v;
  return LSPCG_OK;
}

int bsell_fill_values(const SellPattern& P, const void* src, int src_dtype, int dst_dtype, hipStream_t st, void** out) {
  const size_t es = dst_dtype == LSPCG_F32 ? 4 : 8;
  void* v = *out;  // an existing array of this pattern and dtype is refilled in place
  const bool mine = v == nullptr;
  if (!v) {
    LSPCG_HIP(hipMalloc(&v, es * std::max<int64_t>(P.alloc_slots(), 1)));
    if (int rc = zero_surplus(P, v, es, st)) {
      (void)hipFree(v);
      return rc;
    }
  }
  const dim3 g(slice_grid(P.ns)), b(256);
  if (P.ns)
    with_value_types(src_dtype, dst_dtype, [&](auto vs, auto vd) {
      using VS = decltype(vs);
      using VD = decltype(vd);
      const VS* s = static_cast<const VS*>(src);
      VD* d = static_cast<VD*>(v);
      const int32_t* nocol = nullptr;
      int32_t* no32 = nullptr;
      int16_t* no16 = nullptr;
      if (P.col_bits == 1)
        hipLaunchKernelGGL((k_bsdia_fill<VS, VD>), g, b, 0, st, P.nb, P.ns, P.gp, static_cast<const uint16_t*>(P.col),
                           P.rowptr, s, d);
      else
        hipLaunchKernelGGL((k_bsell_fill<VS, VD>), g, b, 0, st, P.nb, P.ns, P.gp, P.rowptr, nocol, s, no32, no16, d);
    });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    if (mine) (void)hipFree(v);
    set_error(std::string("bsell_fill_values: ") + hipGetErrorString(e));
    return LSPCG_ERR_HIP;
  }
  *out = v;
  return LSPCG_OK;
}

}  // namespace lspcg
