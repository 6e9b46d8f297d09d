// wave.hpp — device helpers of the census family (stage_f / stage_l / stage_m / stage_n / stage_p / stage_q, census_rows) and the sequence scans (seq_scan.hpp): wave and
// workgroup folds, searches in ascending arrays, the window of a barcode list, the compaction step and the list append. No kernels here. Everything is wave-uniform where it says so: call it from
// code that every lane of the wave reaches.
#pragma once
#include "common.hpp"

namespace h10x {

// ---- folds: the 64-lane butterfly (every lane gets the result), and the workgroup's ending
__device__ __forceinline__ u32 wave_sum(u32 v) { for (int k = 32; k; k >>= 1) v += (u32)__shfl_xor((int)v, k); return v; }
__device__ __forceinline__ u64 wave_sum(u64 v) { for (int k = 32; k; k >>= 1) v += __shfl_xor(v, k); return v; }
__device__ __forceinline__ u32 wave_max(u32 v) { for (int k = 32; k; k >>= 1) { const u32 o = (u32)__shfl_xor((int)v, k); v = v > o ? v : o; } return v; }

// the workgroup's sum / maximum of v, for the caller's one atomic per workgroup: THREAD 0 gets it, what the others get means nothing.
// s = blockDim.x / WAVE words of LDS. Holds a __syncthreads(): every thread of the workgroup calls it
template <bool MAX>
__device__ __forceinline__ u32 wg_fold(u32 v, u32 *s) {
  v = MAX ? wave_max(v) : wave_sum(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (u32 w = 1; w < blockDim.x / WAVE; ++w) v = MAX ? (v > s[w] ? v : s[w]) : v + s[w];
  return v;
}
__device__ __forceinline__ u32 wg_sum(u32 v, u32 *s) { return wg_fold<false>(v, s); }
__device__ __forceinline__ u32 wg_max(u32 v, u32 *s) { return wg_fold<true>(v, s); }

// ---- searches. rows[l .. r) ascends (global memory or LDS: inlined, the reads keep their address space)
// the first index in [l, r) with rows[index] >= lo (r if there is none)
template <typename E, typename I>
__device__ __forceinline__ I lower_bound(const E *rows, I l, I r, E lo) {
  while (l < r) { const I m = (l + r) >> 1; if (rows[m] < lo) l = m + 1; else r = m; }
  return l;
}
// the first index in [l, r) with rows[index] > v
template <typename I>
__device__ __forceinline__ I upper_bound(const u32 *rows, I l, I r, u32 v) {
  while (l < r) { const I m = (l + r) >> 1; if (rows[m] <= v) l = m + 1; else r = m; }
  return l;
}
// the last q in [0, n) with base[q] <= u (base ascends, base[0] <= u): the slot of unit u behind an exclusive sum
__device__ __forceinline__ u32 last_le(const u64 *__restrict__ base, u32 n, u64 u) {
  u32 l = 0, r = n;
  while (r - l > 1) { const u32 m = (l + r) >> 1; if (base[m] <= u) l = m; else r = m; }
  return l;
}

// entries [a, b) of the barcode list of goodRow word d (row >> rowShift | len << 32; ascending barcode) with barcode in [lo, hi);
// full = the window covers every barcode
__device__ __forceinline__ void list_window(const u32 *__restrict__ rows, u64 d, u32 rowShift, u32 lo, u32 hi, bool full, u64 &a, u64 &b) {
  a = (u64)(u32)d << rowShift; b = a + (u32)(d >> 32);
  if (full) return;
  a = lower_bound(rows, a, b, lo); b = lower_bound(rows, a, b, hi);
}

// entries [a, b) of hash x's barcode list (rowStart / hashDepth, unsharded) with block in [lo, hi); full = the window covers every block (stage_p.hip, stage_r.hip)
__device__ __forceinline__ void sp_window(const u32 *__restrict__ rows, const u64 *__restrict__ rowStart, const u32 *__restrict__ hashDepth, u32 x, u32 lo, u32 hi,
                                          bool full, u64 &a, u64 &b) {
  a = rowStart[x]; b = a + hashDepth[x];
  if (full) return;
  a = lower_bound(rows, a, b, lo); b = lower_bound(rows, a, b, hi);
}

// entries of block `code`'s good lists in the window, over the whole wave (wave-uniform; every lane gets the sum); n = its good ranks
__device__ __forceinline__ u64 good_list_entries(u32 code, const u32 *__restrict__ nGood, const u64 *__restrict__ blockOff, const u64 *__restrict__ goodRow,
                                                 const u32 *__restrict__ rows, u32 rowShift, u32 lo, u32 hi, bool full, u32 &n) {
  n = nGood[code]; const u64 o = blockOff[code];
  u64 s = 0;
  for (u32 i = threadIdx.x & (WAVE - 1); i < n; i += WAVE) { u64 a, b; list_window(rows, goodRow[o + i], rowShift, lo, hi, full, a, b); s += b - a; }
  return wave_sum(s);
}

// ---- compaction (wave-uniform): the place of this lane's kept item, behind p0 and the kept items of the lanes below; p0 moves past them all
template <typename P>
__device__ __forceinline__ P wave_place(bool keep, P &p0) {
  const u64 m = __ballot(keep);
  const P p = p0 + (P)__popcll(m & ((1ull << (threadIdx.x & (WAVE - 1))) - 1));
  p0 += (P)__popcll(m);
  return p;
}
// The slot of this lane's item in a list that grows behind *counter: one reservation per wave step, made by the lowest lane that emits. EVERY lane of
// the wave must reach it (the ballot and the shuffle are over all 64); what a lane without an item gets means nothing
__device__ __forceinline__ u64 wave_append(bool emit, u64 *counter) {
  const u64 m = __ballot(emit);
  if (!m) return 0;
  const int lane = threadIdx.x & (WAVE - 1), leader = __ffsll((long long)m) - 1;
  const u64 base = lane == leader ? atomicAdd((unsigned long long *)counter, (unsigned long long)__popcll(m)) : 0;
  return __shfl(base, leader) + (u64)__popcll(m & (((u64)1 << lane) - 1));
}

}  // namespace h10x
