// stage_q.hip — row links, behind --seqLinks: which lists of block numbers share at least M blocks (include/h10x.h "row links"). The lists
// are the --seqBlocks rows of sequence ends, the "hashes" of this census are the blocks, and the join is the scan-placed census of stage_l.hip / stage_p.hip
// turned round: a block's run in the sorted accumulator is the list of ends that hold it, and every pair (e < f) of that run is one key.
//   append   every row entry becomes a key block << 32 | list in a device array that grows by doubling: lists are numbered on from those added before,
//            so the array stands in (list, block) order. Rows come from the host or straight from the rows stage_p.hip keeps;
//   sort     the keys repacked as block << listBits | list and sorted with prim_sort_keys_u64 on the bits in use: a block's run ascends in list;
//   runs     one lane per sorted key: at a run's head its length is ends(d); used and skipped blocks are counted, one atomic per workgroup each;
//   units    one lane per row entry in (list, block) order: its place p in its block's run by one search, the run's end by a galloping search from
//            there, src = p + 1 and end = the run's end (src for a skipped block): the later members of the run are the partners f > e, n = end - src. The exclusive sum of n is every unit's place and
//            the difference over a list its size: no atomics, no reservations, a fixed output order;
//   gather   one LANE per output pair: its unit by a search in the places, then key = (e - first list of batch) << listBits | f. The units are short
//            (a block stands in few ends), a wave per unit would idle most lanes; a lane per pair keeps whole waves and coalesced stores.
//            32-bit keys where slot and list fit, else 64-bit;
//   sort     prim_sort_keys_u32 / _u64 on the bits in use;
//   runs     a run of equal keys is one (e, f) with shared = its length; runs of length >= M are flagged, siblings (2s, 2s + 1) are not;
//   rows     a scan of the flags places (f, shared) behind the rows of the batches before; rows per list by two searches in the slot column.
// Batches are cut by list against "neighbour_budget" (pairs gathered); a list above it runs alone in windows of the other list's number (its units'
// partners ascend, so a window is a stretch of each). The run, emit and row-count kernels are this file's own copies of stage_l.hip's.
#include "common.hpp"
#include "prim.hpp"
#include "wave.hpp"

namespace h10x {

static constexpr u64 SQ_DEFAULT_BUDGET = 1ull << 26;       // pairs per batch (stage_l.hip's SG_DEFAULT_BUDGET)
static constexpr unsigned SQ_EMIT_GRID = 2048;
static constexpr u64 SQ_LIST_MASK = 0xFFFFFFFFull;         // accumulator key = block << 32 | list

// the first index in [l, r) with keys[index] >= v
__device__ __forceinline__ u64 sq_lower64(const u64 *__restrict__ keys, u64 l, u64 r, u64 v) {
  while (l < r) { const u64 m = (l + r) >> 1; if (keys[m] < v) l = m + 1; else r = m; }
  return l;
}
// the first entry of list e in the accumulator (its list field ascends)
__device__ __forceinline__ u64 sq_list_start(const u64 *__restrict__ acc, u64 n, u64 e) {
  u64 l = 0, r = n;
  while (l < r) { const u64 m = (l + r) >> 1; if ((acc[m] & SQ_LIST_MASK) < e) l = m + 1; else r = m; }
  return l;
}

// the end of the run of block d that holds sorted[p]: the first r > p with r == n or another block there (doubling steps, then bisection: the runs are short)
__device__ __forceinline__ u64 sq_run_end(const u64 *__restrict__ sorted, u64 n, u64 p, int lb, u64 d) {
  u64 l = p, step = 1, r = p + 1;
  while (r < n && (sorted[r] >> lb) == d) { l = r; step <<= 1; r = l + step; }
  if (r > n) r = n;
  while (r - l > 1) { const u64 m = (l + r) >> 1; if ((sorted[m] >> lb) == d) l = m; else r = m; }
  return r;
}

// entry j of rows in CSR form (off[0] = 0, m = off[nLists]) -> acc[j]
__global__ __launch_bounds__(256) void sq_append_kernel(const u64 *__restrict__ off, const u32 *__restrict__ block, u32 nLists, u64 m, u32 listBase,
                                                        u64 *__restrict__ acc) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride)
    acc[j] = (u64)block[j] << 32 | (u64)(listBase + last_le(off, nLists, j));
}

__global__ __launch_bounds__(256) void sq_pack_kernel(const u64 *__restrict__ acc, u64 n, int lb, u64 *__restrict__ out) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { const u64 k = acc[i]; out[i] = (k >> 32) << lb | (k & SQ_LIST_MASK); }
}

// tally[0] += blocks with 1 .. maxLists ends (every block that has one when maxLists = 0), tally[1] += the others that have one
__global__ __launch_bounds__(256) void sq_blocks_kernel(const u64 *__restrict__ sorted, u64 n, int lb, u32 maxLists, u32 *__restrict__ tally) {
  __shared__ u32 sA[256 / WAVE], sB[256 / WAVE];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u32 used = 0, skipped = 0;
  for (u64 i0 = (u64)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {   // wave-uniform: whole workgroups
    const u64 i = i0 + threadIdx.x;
    if (i < n) {
      const u64 d = sorted[i] >> lb;
      if (!i || (sorted[i - 1] >> lb) != d) {
        const u64 len = sq_run_end(sorted, n, i, lb, d) - i;
        if (!maxLists || len <= maxLists) ++used; else ++skipped;
      }
    }
  }
  used = wg_sum(used, sA); skipped = wg_sum(skipped, sB);
  if (threadIdx.x == 0) { if (used) atomicAdd(tally, used); if (skipped) atomicAdd(tally + 1, skipped); }
}

// one lane per row entry i (list order): src[i] = the place behind it in its block's run, end[i] = the run's end (src[i] where the block is skipped),
// cnt[i] = end - src; cnt[n] = 0
__global__ __launch_bounds__(256) void sq_unit_kernel(const u64 *__restrict__ acc, const u64 *__restrict__ sorted, u64 n, int lb, u32 maxLists,
                                                      u32 *__restrict__ src, u32 *__restrict__ end, u32 *__restrict__ cnt) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) { cnt[i] = 0; return; }
  const u64 k = acc[i], d = k >> 32;
  const u64 at = sq_lower64(sorted, 0, n, d << lb | (k & SQ_LIST_MASK)), p = at + 1;   // the key itself: it is there
  const u64 re = sq_run_end(sorted, n, at, lb, d);
  u64 e = re;
  if (maxLists) {                                             // the run's start matters only within maxLists of the key: a run that reaches further back is too long
    const u64 lo = at > maxLists ? at - maxLists : 0;
    if (re - sq_lower64(sorted, lo, at, d << lb) > maxLists) e = p;
  }
  src[i] = (u32)p; end[i] = (u32)e; cnt[i] = (u32)(e - p);
}

__global__ void sq_offsets_kernel(const u64 *__restrict__ acc, u64 n, u64 nLists, u64 *__restrict__ off) {
  const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e <= nLists) off[e] = sq_list_start(acc, n, e);
}

__global__ void sq_size_kernel(const u64 *__restrict__ off, const u64 *__restrict__ place, u64 nLists, u64 *__restrict__ size) {
  const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nLists) size[e] = place[off[e + 1]] - place[off[e]];
}

// the partners of unit i with list number in [lo, hi): [a, b) of the sorted keys
__device__ __forceinline__ void sq_window(const u64 *__restrict__ acc, const u64 *__restrict__ sorted, const u32 *__restrict__ src, const u32 *__restrict__ end,
                                          u64 i, int lb, u64 lo, u64 hi, bool full, u64 &a, u64 &b) {
  a = src[i]; b = end[i];
  if (full) return;
  const u64 base = (acc[i] >> 32) << lb;
  a = sq_lower64(sorted, a, b, base + lo); b = sq_lower64(sorted, a, b, base + hi);
}

// one lane per unit u of the batch (row entry i0 + u): cntW[u] = its partners in the window, from srcW[u]; cntW[units] = 0
__global__ __launch_bounds__(256) void sq_window_kernel(const u64 *__restrict__ acc, const u64 *__restrict__ sorted, const u32 *__restrict__ src,
                                                        const u32 *__restrict__ end, u64 i0, u64 units, int lb, u64 lo, u64 hi, int full,
                                                        u32 *__restrict__ cntW, u32 *__restrict__ srcW) {
  const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (u > units) return;
  if (u == units) { cntW[u] = 0; return; }
  u64 a, b; sq_window(acc, sorted, src, end, i0 + u, lb, lo, hi, full != 0, a, b);
  cntW[u] = (u32)(b - a); srcW[u] = (u32)a;
}

// ONE workgroup: out[0] = the partners of the units [i0, i0 + units) in the window (the size of one list in one window)
__global__ __launch_bounds__(256) void sq_window_size_kernel(const u64 *__restrict__ acc, const u64 *__restrict__ sorted, const u32 *__restrict__ src,
                                                             const u32 *__restrict__ end, u64 i0, u64 units, int lb, u64 lo, u64 hi, u64 *__restrict__ out) {
  __shared__ u64 s[256 / WAVE];
  u64 sum = 0;
  for (u64 u = threadIdx.x; u < units; u += blockDim.x) { u64 a, b; sq_window(acc, sorted, src, end, i0 + u, lb, lo, hi, false, a, b); sum += b - a; }
  sum = wave_sum(sum);
  if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = sum;
  __syncthreads();
  if (threadIdx.x == 0) { for (u32 w = 1; w < 256 / WAVE; ++w) sum += s[w]; out[0] = sum; }
}

// one lane per output pair j < nKeys: its unit u = the last with place[u] <= j, its partner the (j - place[u])-th from srcW[u]
template <typename K>
__global__ __launch_bounds__(256) void sq_gather_kernel(const u64 *__restrict__ acc, const u64 *__restrict__ sorted, u64 i0, u32 units, const u64 *__restrict__ place,
                                                        const u32 *__restrict__ srcW, u32 q0, int lb, u64 nKeys, K *__restrict__ keys) {
  const u64 stride = (u64)gridDim.x * blockDim.x, mask = ((u64)1 << lb) - 1;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < nKeys; j += stride) {
    const u32 u = last_le(place, units, j);
    const u32 e = (u32)(acc[i0 + u] & SQ_LIST_MASK);
    const u64 f = sorted[(u64)srcW[u] + (j - place[u])] & mask;
    keys[j] = (K)(e - q0) << lb | (K)f;
  }
}

// flag[i] = 1 at the head of a run of at least T equal keys that is no sibling pair, cnt[i] = its length there (stage_l.hip's sg_run_kernel)
template <typename K>
__global__ void sq_run_kernel(const K *__restrict__ keys, u64 n, u32 T, int siblings, u32 q0, int lb, u32 *__restrict__ flag, u32 *__restrict__ cnt) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const K k = keys[i];
    u32 f = 0;
    if (!i || keys[i - 1] != k) {
      u64 l = i, step = 1;                                    // keys[l] == k; the first r > l with r == n or keys[r] != k
      u64 r = i + 1;
      while (r < n && keys[r] == k) { l = r; step <<= 1; r = l + step; }
      if (r > n) r = n;
      while (r - l > 1) { const u64 m = (l + r) >> 1; if (keys[m] == k) l = m; else r = m; }
      const u64 c = r - i;
      const u32 a = q0 + (u32)((u64)k >> lb), b = (u32)((u64)k & (((u64)1 << lb) - 1));
      if (c >= T && !(siblings && (a >> 1) == (b >> 1))) { f = 1; cnt[i] = (u32)c; }
    }
    flag[i] = f;
  }
}

// the rows of the flagged runs at oOther / oShared [pos[i]], their slot at oSlot[pos[i]], and the largest length: one atomic per workgroup
template <typename K>
__global__ __launch_bounds__(256) void sq_emit_kernel(const K *__restrict__ keys, u64 n, int lb, const u32 *__restrict__ flag, const u32 *__restrict__ cnt,
                                                      const u32 *__restrict__ pos, u64 runs, u32 *__restrict__ oOther, u32 *__restrict__ oShared,
                                                      u32 *__restrict__ oSlot, u32 *__restrict__ maxShared) {
  __shared__ u32 sMax[256 / WAVE];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u32 mx = 0;
  for (u64 i0 = (u64)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {   // wave-uniform: whole workgroups
    const u64 i = i0 + threadIdx.x;
    if (i < n && flag[i]) {
      const u64 k = (u64)keys[i]; const u32 p = pos[i], c = cnt[i];
      if (p < runs) { oOther[p] = (u32)(k & (((u64)1 << lb) - 1)); oShared[p] = c; oSlot[p] = (u32)(k >> lb); }
      mx = mx > c ? mx : c;
    }
  }
  mx = wg_max(mx, sMax);
  if (threadIdx.x == 0 && mx) atomicMax(maxShared, mx);
}

// rowCnt[q] += rows of the batch with slot q (oSlot ascends). A windowed list comes here once per window, one launch after the other
__global__ void sq_rowcount_kernel(const u32 *__restrict__ oSlot, u64 runs, u32 nq, u32 *__restrict__ rowCnt) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const u64 s = lower_bound(oSlot, (u64)0, runs, q);
  rowCnt[q] += (u32)(upper_bound(oSlot, s, runs, q) - s);
}

// ------------------------------------------------------------------------------------------------ drivers
namespace {

void release_links(Ctx *c) { c->haveRowLinks = false; c->rlLinks = 0; c->rlLists = 0; c->rlOther.release(); c->rlShared.release(); c->rlOffsets.release(); }
void release_acc(Ctx *c) { c->rqOpen = false; c->rqEntries = 0; c->rqLists = 0; c->rqBlocks = 0; c->rqKeys.release(); }

int sq_ctx_check(Ctx *c, const char *cmd) {
  if (c->sharded) return c->fail("%s: not available on a sharded context (one rank holds only its own barcodes)", cmd);
  return 0;
}
int sq_open_check(Ctx *c, const char *cmd) {
  H10X_TRY(sq_ctx_check(c, cmd));
  if (!c->rqOpen) return c->fail("%s: no accumulator is open (h10x_row_links_begin first; a new range, --clusterSplit and a new state release it)", cmd);
  return 0;
}

// dst holds at least `need` words; the first `used` are kept (grown by doubling)
template <typename T>
int sq_reserve(Ctx *c, DevBuf<T> &dst, u64 used, u64 need) {
  if (need <= dst.n && dst.p) return 0;
  DevBuf<T> b;
  H10X_HIP(c, b.alloc(hmax<u64>(need, 2 * (u64)dst.n)));
  if (used) H10X_HIP(c, hipMemcpyAsync(b.p, dst.p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
  dst.swap(b);
  H10X_HIP(c, hipStreamSynchronize(c->stream));               // the old block goes back to the cache behind the copy
  return 0;
}

// nLists rows with m entries in CSR form on the device (dOff[0] = 0) go behind the accumulator
int append(Ctx *c, const u64 *dOff, const u32 *dBlock, u64 nLists, u64 m) {
  if (c->rqLists + nLists > 0xFFFFFFFFull) return c->fail("rowLinks: %llu lists, beyond 2^32 - 1", c->rqLists + nLists);
  if (c->rqEntries + m >= 0xFFFFFFFFull) return c->fail("rowLinks: %llu row entries, beyond 2^32 - 2", c->rqEntries + m);
  if (m) {
    H10X_TRY(sq_reserve(c, c->rqKeys, c->rqEntries, c->rqEntries + m));
    sq_append_kernel<<<(unsigned)hmin<u64>(divUp(m, 256), 16384), 256, 0, c->stream>>>(dOff, dBlock, (u32)nLists, m, (u32)c->rqLists, c->rqKeys.p + c->rqEntries);
    H10X_HIP(c, hipGetLastError());
  }
  c->rqLists += nLists; c->rqEntries += m;
  return 0;
}

struct RowLinks {
  Ctx *c; u32 T, maxLists, nq; int siblings, lb; u64 n, budget;
  std::vector<u64> size, hOff;
  DevBuf<u64> packed, sorted, place, dOff, dSize, placeW, keys64, keys64s, winSize;
  DevBuf<u32> src, end, cnt, cntW, srcW, keys32, keys32s, flag, rcnt, pos, oSlot, rowCnt;
  u32 *tally = nullptr;                                     // used, skipped, maxShared
  PrimTemp pt;
  u64 rows = 0, pairs = 0; u32 batches = 0, windows = 0, wide = 0;

  template <typename K>
  int sortAndEmit(DevBuf<K> &keys, DevBuf<K> &keysS, u32 q0, u32 nl, int endBit, u64 i0, u64 units, u64 nKeys) {
    hipStream_t st = c->stream;
    if (keys.n < nKeys) { H10X_HIP(c, keys.alloc(nKeys)); H10X_HIP(c, keysS.alloc(nKeys)); }
    const unsigned gr = (unsigned)hmin<u64>(divUp(nKeys, 256), 16384);
    sq_gather_kernel<K><<<gr, 256, 0, st>>>(c->rqKeys.p, sorted.p, i0, (u32)units, placeW.p, srcW.p, q0, lb, nKeys, keys.p);
    H10X_HIP(c, hipGetLastError());
    if (sizeof(K) == 4) H10X_TRY(prim_sort_keys_u32(c, pt, (const u32 *)keys.p, (u32 *)keysS.p, nKeys, 0, endBit));
    else H10X_TRY(prim_sort_keys_u64(c, pt, (const u64 *)keys.p, (u64 *)keysS.p, nKeys, 0, endBit));
    if (flag.n < nKeys) { H10X_HIP(c, flag.alloc(nKeys)); H10X_HIP(c, rcnt.alloc(nKeys)); H10X_HIP(c, pos.alloc(nKeys)); }
    sq_run_kernel<K><<<gr, 256, 0, st>>>(keysS.p, nKeys, T, siblings, q0, lb, flag.p, rcnt.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, pos.p, nKeys));
    u32 lastPos = 0, lastFlag = 0;
    H10X_TRY(c->readback(&lastPos, pos.p + (nKeys - 1), 4)); H10X_TRY(c->readback(&lastFlag, flag.p + (nKeys - 1), 4)); H10X_TRY(c->syncReadbacks());
    const u64 runs = (u64)lastPos + lastFlag;
    if (!runs) return 0;
    H10X_TRY(sq_reserve(c, c->rlOther, rows, rows + runs)); H10X_TRY(sq_reserve(c, c->rlShared, rows, rows + runs));
    if (oSlot.n < runs) H10X_HIP(c, oSlot.alloc(runs));
    sq_emit_kernel<K><<<hmin<unsigned>(gr, SQ_EMIT_GRID), 256, 0, st>>>(keysS.p, nKeys, lb, flag.p, rcnt.p, pos.p, runs, c->rlOther.p + rows, c->rlShared.p + rows, oSlot.p,
                                                                       tally + 2);
    H10X_HIP(c, hipGetLastError());
    sq_rowcount_kernel<<<divUp(nl, 256), 256, 0, st>>>(oSlot.p, runs, nl, rowCnt.p + q0);
    H10X_HIP(c, hipGetLastError());
    rows += runs;
    return 0;
  }

  // lists [q0, q0 + nl) against the partners numbered [lo, hi); total = pairs gathered
  int batch(u32 q0, u32 nl, u32 lo, u32 hi, bool full, u64 total) {
    hipStream_t st = c->stream;
    if (!full) { c->nbStats[3] += 1; ++windows; }             // one window of a list above the budget
    c->nbStats[2] += 1; ++batches;
    if (!total) return 0;
    if (total >= 0xFFFFFFFFull) return c->fail("rowLinks: %llu pairs in one batch, beyond 2^32 (list %u alone)", total, q0);
    const u64 i0 = hOff[q0], units = hOff[q0 + nl] - i0;
    if (cntW.n < units + 1) { H10X_HIP(c, cntW.alloc(units + 1)); H10X_HIP(c, srcW.alloc(units + 1)); H10X_HIP(c, placeW.alloc(units + 1)); }
    sq_window_kernel<<<divUp(units + 1, 256), 256, 0, st>>>(c->rqKeys.p, sorted.p, src.p, end.p, i0, units, lb, lo, hi, full ? 1 : 0, cntW.p, srcW.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, cntW.p, placeW.p, units + 1));
    unsigned long long nKeys = 0;
    H10X_TRY(c->readback(&nKeys, placeW.p + units, 8)); H10X_TRY(c->syncReadbacks());
    if (nKeys != total) return c->fail("rowLinks: %llu keys of %llu pairs", nKeys, total);
    c->nbStats[0] += total; c->nbStats[1] += nKeys; pairs += total;
    const int endBit = lb + keyBits(nl - 1);
    if (endBit <= 32) return sortAndEmit<u32>(keys32, keys32s, q0, nl, endBit, i0, units, nKeys);
    ++wide;
    return sortAndEmit<u64>(keys64, keys64s, q0, nl, endBit, i0, units, nKeys);
  }

  int windowSize(u32 q, u32 lo, u32 hi, u64 *records) {
    if (!winSize.p) H10X_HIP(c, winSize.alloc(1));
    sq_window_size_kernel<<<1, 256, 0, c->stream>>>(c->rqKeys.p, sorted.p, src.p, end.p, hOff[q], hOff[q + 1] - hOff[q], lb, lo, hi, winSize.p);
    H10X_HIP(c, hipGetLastError());
    unsigned long long v = 0;
    H10X_TRY(c->readback(&v, winSize.p, 8)); H10X_TRY(c->syncReadbacks());
    *records = v;
    return 0;
  }

  int run(h10x_row_links_info *info) {
    hipStream_t st = c->stream;
    const u64 *acc = c->rqKeys.p;
    tally = c->zeros(3);
    if (!tally) return -1;
    H10X_HIP(c, rowCnt.alloc((size_t)nq + 1)); H10X_HIP(c, hipMemsetAsync(rowCnt.p, 0, ((size_t)nq + 1) * 4, st));
    H10X_HIP(c, c->rlOffsets.alloc((size_t)nq + 1));
    if (n) {
      const int endBit = lb + keyBits(c->rqBlocks ? c->rqBlocks - 1 : 0);
      const unsigned gr = (unsigned)hmin<u64>(divUp(n, 256), 16384);
      H10X_HIP(c, packed.alloc(n)); H10X_HIP(c, sorted.alloc(n));
      sq_pack_kernel<<<gr, 256, 0, st>>>(acc, n, lb, packed.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_sort_keys_u64(c, pt, packed.p, sorted.p, n, 0, endBit));
      packed.release();
      sq_blocks_kernel<<<hmin<unsigned>(gr, SQ_EMIT_GRID), 256, 0, st>>>(sorted.p, n, lb, maxLists, tally);
      H10X_HIP(c, hipGetLastError());
      H10X_HIP(c, src.alloc(n)); H10X_HIP(c, end.alloc(n)); H10X_HIP(c, cnt.alloc(n + 1)); H10X_HIP(c, place.alloc(n + 1));
      sq_unit_kernel<<<divUp(n + 1, 256), 256, 0, st>>>(acc, sorted.p, n, lb, maxLists, src.p, end.p, cnt.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, cnt.p, place.p, n + 1));
      H10X_HIP(c, dOff.alloc((size_t)nq + 1)); H10X_HIP(c, dSize.alloc(nq));
      sq_offsets_kernel<<<divUp((u64)nq + 1, 256), 256, 0, st>>>(acc, n, nq, dOff.p);
      H10X_HIP(c, hipGetLastError());
      sq_size_kernel<<<divUp(nq, 256), 256, 0, st>>>(dOff.p, place.p, nq, dSize.p);
      H10X_HIP(c, hipGetLastError());
      size.resize(nq); hOff.resize((size_t)nq + 1);
      H10X_HIP(c, hipMemcpyAsync(hOff.data(), dOff.p, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(size.data(), dSize.p, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipStreamSynchronize(st));
      cnt.release(); place.release(); dSize.release(); dOff.release();
      H10X_TRY(cut_batches(size.data(), nq, nq, budget,
                           [&](u32 q, u32 lo, u32 hi, u64 *records) { return windowSize(q, lo, hi, records); },
                           [&](u32 q0, u32 nl, u32 lo, u32 hi, bool full, u64 total) { return batch(q0, nl, lo, hi, full, total); }));
    }
    H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, rowCnt.p, c->rlOffsets.p, (size_t)nq + 1));
    u32 t[3] = {0, 0, 0};
    H10X_TRY(c->readback(t, tally, 12)); H10X_TRY(c->syncReadbacks());
    info->blocksUsed = t[0]; info->skippedBlocks = t[1]; info->maxShared = t[2];
    return 0;
  }
};
}  // namespace

void stageQ_release(Ctx *c) { release_acc(c); release_links(c); }

int stageQ_begin(Ctx *c, u32 nBlocks) {
  stageQ_release(c);
  H10X_TRY(sq_ctx_check(c, "rowLinks"));
  c->rqOpen = true; c->rqBlocks = nBlocks;
  return 0;
}

int stageQ_add(Ctx *c, const u64 *offsets, const u32 *block, u64 nLists) {
  H10X_TRY(sq_open_check(c, "rowLinks"));
  if (nLists && (!offsets || (offsets[nLists] && !block))) return c->fail("rowLinks: null argument");
  if (!nLists) return 0;
  if (offsets[0]) return c->fail("!! rowLinks offsets must start at 0");
  for (u64 q = 0; q < nLists; ++q) {
    if (offsets[q + 1] < offsets[q]) return c->fail("!! rowLinks offsets descend at list %llu", c->rqLists + q);
    for (u64 j = offsets[q]; j < offsets[q + 1]; ++j) {
      if (block[j] >= c->rqBlocks)
        return c->fail("!! rowLinks list %llu entry %llu: block %u is not below %u", c->rqLists + q, j - offsets[q], block[j], c->rqBlocks);
      if (j > offsets[q] && block[j] <= block[j - 1])
        return c->fail("!! rowLinks list %llu entry %llu: block %u is not ascending", c->rqLists + q, j - offsets[q], block[j]);
    }
  }
  hipStream_t st = c->stream;
  const u64 m = offsets[nLists];
  if (nLists > 0xFFFFFFFFull) return c->fail("rowLinks: %llu lists, beyond 2^32 - 1", nLists);
  DevBuf<u64> dOff; DevBuf<u32> dBlock;
  H10X_HIP(c, dOff.alloc((size_t)nLists + 1)); H10X_HIP(c, dBlock.alloc(hmax<u64>(m, 1)));
  H10X_HIP(c, hipMemcpyAsync(dOff.p, offsets, ((size_t)nLists + 1) * 8, hipMemcpyHostToDevice, st));
  if (m) H10X_HIP(c, hipMemcpyAsync(dBlock.p, block, (size_t)m * 4, hipMemcpyHostToDevice, st));
  const int rc = append(c, dOff.p, dBlock.p, nLists, m);
  (void)hipStreamSynchronize(st);                             // the uploads go back to the block cache behind finished work
  return rc;
}

int stageQ_addKept(Ctx *c) {
  H10X_TRY(sq_open_check(c, "rowLinks"));
  if (!c->haveState) return c->fail("no hash state loaded: use readFQB or readHash first");
  if (!c->haveRange || !c->haveGood) return c->fail("!! you must set hashDepthRange before rowLinks");
  if (!c->haveSeqBlocks) return c->fail("rowLinks: no rows are kept (run h10x_list_share_run or h10x_seq_blocks_run first)");
  if (c->nBlocks > c->rqBlocks) return c->fail("rowLinks: the kept rows are of %u blocks, the accumulator of %u", c->nBlocks, c->rqBlocks);
  return append(c, c->sbOffsets.p, c->sbBlock.p, c->sbLists, c->sbRows);
}

int stageQ_finish(Ctx *c, int64_t minBlocks, int64_t maxLists, int siblings, h10x_row_links_info *info) {
  release_links(c);
  memset(info, 0, sizeof *info);
  H10X_TRY(sq_open_check(c, "rowLinks"));
  if (minBlocks < 1) return c->fail("!! seqLinks minBlocks %lld must be >= 1", (long long)minBlocks);
  if (maxLists < 0) return c->fail("!! seqLinks maxEnds %lld must be >= 0", (long long)maxLists);
  if (c->rqLists > 0xFFFFFFFFull) return c->fail("rowLinks: %llu lists, beyond 2^32 - 1", c->rqLists);
  RowLinks g; g.c = c; g.T = (u32)hmin<int64_t>(minBlocks, 0xFFFFFFFFll); g.maxLists = (u32)hmin<int64_t>(maxLists, 0xFFFFFFFFll);
  g.nq = (u32)c->rqLists; g.siblings = siblings ? 1 : 0; g.n = c->rqEntries; g.lb = keyBits(g.nq ? g.nq - 1 : 0);
  g.budget = c->optNbBudget > 0 ? (u64)c->optNbBudget : SQ_DEFAULT_BUDGET;
  if (g.lb + keyBits(c->rqBlocks) > 63) return c->fail("rowLinks: %u lists of %u blocks do not fit a 64-bit key", g.nq, c->rqBlocks);
  info->lists = c->rqLists; info->rowEntries = c->rqEntries;
  ZeroScope zs(c);
  if (zs.rc) return zs.rc;
  const int rc = g.run(info);
  if (rc) { (void)hipStreamSynchronize(c->stream); release_links(c); return rc; }
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  if (!c->rlOther.p) { H10X_HIP(c, c->rlOther.alloc(1)); H10X_HIP(c, c->rlShared.alloc(1)); }
  c->haveRowLinks = true; c->rlLinks = g.rows; c->rlLists = g.nq;
  info->pairs = g.pairs; info->links = g.rows; info->batches = g.batches; info->windows = g.windows; info->wideBatches = g.wide;
  return 0;
}

// offsets[lists + 1] and the first min(cap, links) links of the kept result, to host (toDevice = 0) or device memory; any may be null
int stageQ_get(Ctx *c, u64 *offsets, u32 *other, u32 *shared, u64 cap, int toDevice) {
  if (!c->haveRowLinks) return c->fail("rowLinks: no links are kept (finish first; a new begin, a new range, --clusterSplit and a new state release them)");
  const hipMemcpyKind kind = toDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t m = (size_t)hmin<u64>(cap, c->rlLinks);
  if (offsets) H10X_HIP(c, hipMemcpyAsync(offsets, c->rlOffsets.p, ((size_t)c->rlLists + 1) * 8, kind, c->stream));
  if (m && other) H10X_HIP(c, hipMemcpyAsync(other, c->rlOther.p, m * 4, kind, c->stream));
  if (m && shared) H10X_HIP(c, hipMemcpyAsync(shared, c->rlShared.p, m * 4, kind, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int stageQ_getRange(Ctx *c, u64 first, u64 count, u32 *other, u32 *shared) {
  if (!c->haveRowLinks) return c->fail("rowLinks: no links are kept (finish first; a new begin, a new range, --clusterSplit and a new state release them)");
  if (first > c->rlLinks || count > c->rlLinks - first) return c->fail("rowLinks: links %llu .. %llu of %llu", first, first + count, c->rlLinks);
  if (count && other) H10X_HIP(c, hipMemcpyAsync(other, c->rlOther.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  if (count && shared) H10X_HIP(c, hipMemcpyAsync(shared, c->rlShared.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace h10x
