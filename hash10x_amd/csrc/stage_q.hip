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
//   tail     census_rows.hip: the keys sorted, a run of equal keys is one (e, f) with shared = its length, the runs of length >= M (siblings
//            (2s, 2s + 1) are none) placed by a scan as rows (f, shared) behind those of the batches before, the rows per list summed to offsets[].
// Batches are cut by list against "neighbour_budget" (pairs gathered); a list above it runs alone in windows of the other list's number (its units'
// partners ascend, so a window is a stretch of each).
#include "census_rows.hpp"
#include "runs.hpp"
#include "wave.hpp"

namespace h10x {

static constexpr u64 SQ_LIST_MASK = 0xFFFFFFFFull;         // accumulator key = block << 32 | list

// the first entry of list e in the accumulator (its list field ascends)
__device__ __forceinline__ u64 sq_list_start(const u64 *__restrict__ acc, u64 n, u64 e) {
  u64 l = 0, r = n;
  while (l < r) { const u64 m = (l + r) >> 1; if ((acc[m] & SQ_LIST_MASK) < e) l = m + 1; else r = m; }
  return l;
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
        const u64 len = run_end(sorted, n, i, [lb](u64 k) { return k >> lb; }) - i;   // the block's run
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
  const u64 at = lower_bound(sorted, (u64)0, n, d << lb | (k & SQ_LIST_MASK)), p = at + 1;   // the key itself: it is there
  const u64 re = run_end(sorted, n, at, [lb](u64 v) { return v >> lb; });   // the end of block d's run
  u64 e = re;
  if (maxLists) {                                             // the run's start matters only within maxLists of the key: a run that reaches further back is too long
    const u64 lo = at > maxLists ? at - maxLists : 0;
    if (re - lower_bound(sorted, lo, at, d << lb) > maxLists) e = p;
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
  a = lower_bound(sorted, a, b, base + lo); b = lower_bound(sorted, a, b, base + hi);
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

// ------------------------------------------------------------------------------------------------ drivers
namespace {

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

// nLists rows with m entries in CSR form on the device (dOff[0] = 0) go behind the accumulator
int append(Ctx *c, const u64 *dOff, const u32 *dBlock, u64 nLists, u64 m) {
  if (c->rqLists + nLists > 0xFFFFFFFFull) return c->fail("rowLinks: %llu lists, beyond 2^32 - 1", c->rqLists + nLists);
  if (c->rqEntries + m >= 0xFFFFFFFFull) return c->fail("rowLinks: %llu row entries, beyond 2^32 - 2", c->rqEntries + m);
  if (m) {
    H10X_TRY(reserve_keep(c, c->rqKeys, c->rqEntries, c->rqEntries + m));
    sq_append_kernel<<<(unsigned)hmin<u64>(divUp(m, 256), 16384), 256, 0, c->stream>>>(dOff, dBlock, (u32)nLists, m, (u32)c->rqLists, c->rqKeys.p + c->rqEntries);
    H10X_HIP(c, hipGetLastError());
  }
  c->rqLists += nLists; c->rqEntries += m;
  return 0;
}

struct RowLinks {
  Ctx *c; u32 maxLists, nq; int lb; u64 n, budget;
  std::vector<u64> size, hOff;
  DevBuf<u64> packed, sorted, place, dOff, dSize, placeW, winSize;
  DevBuf<u32> src, end, cnt, cntW, srcW;
  RowTail tail;

  template <typename K>
  int gather(K *keys, u32 q0, u64 i0, u64 units, u64 nKeys) {
    sq_gather_kernel<K><<<(unsigned)hmin<u64>(divUp(nKeys, 256), 16384), 256, 0, c->stream>>>(c->rqKeys.p, sorted.p, i0, (u32)units, placeW.p, srcW.p, q0, lb, nKeys, keys);
    H10X_HIP(c, hipGetLastError());
    return 0;
  }

  // lists [q0, q0 + nl) against the partners numbered [lo, hi); total = pairs gathered
  int batch(u32 q0, u32 nl, u32 lo, u32 hi, bool full, u64 total) {
    tail.batch(full);                                         // (a window: of a list above the budget)
    if (!total) return 0;
    if (total >= 0xFFFFFFFFull) return c->fail("rowLinks: %llu pairs in one batch, beyond 2^32 (list %u alone)", total, q0);
    const u64 i0 = hOff[q0], units = hOff[q0 + nl] - i0;
    if (cntW.n < units + 1) { H10X_HIP(c, cntW.alloc(units + 1)); H10X_HIP(c, srcW.alloc(units + 1)); H10X_HIP(c, placeW.alloc(units + 1)); }
    sq_window_kernel<<<divUp(units + 1, 256), 256, 0, c->stream>>>(c->rqKeys.p, sorted.p, src.p, end.p, i0, units, lb, lo, hi, full ? 1 : 0, cntW.p, srcW.p);
    H10X_HIP(c, hipGetLastError());
    u64 nKeys = 0;
    H10X_TRY(tail.places(cntW.p, placeW.p, units, &nKeys));
    if (nKeys != total) return c->fail("rowLinks: %llu keys of %llu pairs", nKeys, total);
    tail.gathered(total, nKeys);
    const int endBit = lb + keyBits(nl - 1);
    H10X_TRY(tail.keys(nKeys, endBit > 32));
    H10X_TRY(endBit > 32 ? gather(tail.keys64.p, q0, i0, units, nKeys) : gather(tail.keys32.p, q0, i0, units, nKeys));
    return tail.emit(nKeys, lb, endBit, q0, nl);
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

  int run(u32 T, bool siblings, h10x_row_links_info *info) {
    hipStream_t st = c->stream; PrimTemp &pt = tail.pt;
    const u64 *acc = c->rqKeys.p;
    u32 *tally = c->zeros(2);                                 // used, skipped
    if (!tally) return -1;
    H10X_TRY(tail.begin(c, &c->rl, T, nq, siblings));
    if (n) {
      const int endBit = lb + keyBits(c->rqBlocks ? c->rqBlocks - 1 : 0);
      const unsigned gr = (unsigned)hmin<u64>(divUp(n, 256), 16384);
      H10X_HIP(c, packed.alloc(n)); H10X_HIP(c, sorted.alloc(n));
      sq_pack_kernel<<<gr, 256, 0, st>>>(acc, n, lb, packed.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_sort_keys_u64(c, pt, packed.p, sorted.p, n, 0, endBit));
      packed.release();
      sq_blocks_kernel<<<hmin<unsigned>(gr, ROWS_EMIT_GRID), 256, 0, st>>>(sorted.p, n, lb, maxLists, tally);
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
    u32 t[2] = {0, 0}, mx = 0;
    H10X_TRY(c->readback(t, tally, 8)); H10X_TRY(tail.finish(&mx));   // (one round trip for both)
    info->blocksUsed = t[0]; info->skippedBlocks = t[1]; info->maxShared = mx;
    return 0;
  }
};
}  // namespace

void stageQ_release(Ctx *c) { release_acc(c); c->rl.release(); }

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
  if (!c->sb.have) return c->fail("rowLinks: no rows are kept (run h10x_list_share_run or h10x_seq_blocks_run first)");
  if (c->nBlocks > c->rqBlocks) return c->fail("rowLinks: the kept rows are of %u blocks, the accumulator of %u", c->nBlocks, c->rqBlocks);
  return append(c, c->sb.offsets.p, c->sb.a.p, c->sb.lists, c->sb.rows);
}

int stageQ_finish(Ctx *c, int64_t minBlocks, int64_t maxLists, int siblings, h10x_row_links_info *info) {
  c->rl.release();
  memset(info, 0, sizeof *info);
  H10X_TRY(sq_open_check(c, "rowLinks"));
  if (minBlocks < 1) return c->fail("!! seqLinks minBlocks %lld must be >= 1", (long long)minBlocks);
  if (maxLists < 0) return c->fail("!! seqLinks maxEnds %lld must be >= 0", (long long)maxLists);
  if (c->rqLists > 0xFFFFFFFFull) return c->fail("rowLinks: %llu lists, beyond 2^32 - 1", c->rqLists);
  RowLinks g; g.c = c; g.maxLists = (u32)hmin<int64_t>(maxLists, 0xFFFFFFFFll);
  g.nq = (u32)c->rqLists; g.n = c->rqEntries; g.lb = keyBits(g.nq ? g.nq - 1 : 0);
  g.budget = c->optNbBudget > 0 ? (u64)c->optNbBudget : ROWS_DEFAULT_BUDGET;
  if (g.lb + keyBits(c->rqBlocks) > 63) return c->fail("rowLinks: %u lists of %u blocks do not fit a 64-bit key", g.nq, c->rqBlocks);
  info->lists = c->rqLists; info->rowEntries = c->rqEntries;
  ZeroScope zs(c);
  if (zs.rc) return zs.rc;
  const int rc = g.run((u32)hmin<int64_t>(minBlocks, 0xFFFFFFFFll), siblings != 0, info);
  if (rc) { (void)hipStreamSynchronize(c->stream); c->rl.release(); return rc; }
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  if (!c->rl.a.p) { H10X_HIP(c, c->rl.a.alloc(1)); H10X_HIP(c, c->rl.b.alloc(1)); }
  c->rl.have = true; c->rl.rows = g.tail.rows; c->rl.lists = g.nq;
  info->pairs = g.tail.entries; info->links = g.tail.rows; info->batches = g.tail.batches; info->windows = g.tail.windows; info->wideBatches = g.tail.wide;
  return 0;
}

int stageQ_get(Ctx *c, u64 *offsets, u32 *other, u32 *shared, u64 cap, int toDevice) {
  return c->rl.get(c, offsets, other, shared, cap, toDevice, "rowLinks: no links are kept (finish first; a new begin, a new range, --clusterSplit and a new state release them)");
}

int stageQ_getRange(Ctx *c, u64 first, u64 count, u32 *other, u32 *shared) {
  if (!c->rl.have) return c->fail("rowLinks: no links are kept (finish first; a new begin, a new range, --clusterSplit and a new state release them)");
  if (first > c->rl.rows || count > c->rl.rows - first) return c->fail("rowLinks: links %llu .. %llu of %llu", first, first + count, c->rl.rows);
  if (count && other) H10X_HIP(c, hipMemcpyAsync(other, c->rl.a.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  if (count && shared) H10X_HIP(c, hipMemcpyAsync(shared, c->rl.b.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace h10x
