// stage_c_good.hip — --hashDepthRange: the depth filter and the good-hash list of every barcode block.
//
// Replaces hashWithinRangeBuild (hash10x.c:528-539) and goodHashesBuild (hash10x.c:738-766): within[] per hash, then per block the
// positions of its in-range hashes in ascending (depth, position) — one workgroup builds and sorts a block's list in LDS
// (good_block_kernel, three launch classes by block size); blocks or depths too large for that take keys + a device-wide segmented
// sort + good_pos_kernel. Either way every rank also gets its list descriptor goodRow[] (where the hash's barcode list starts in
// rows[], how long it is: good_block_kernel or good_rows_kernel), which is what the cluster kernels stream.
#include "common.hpp"
#include "prim.hpp"
#include <rocprim/block/block_radix_sort.hpp>

namespace h10x {

// ------------------------------------------------------------------------------------------ depth range
// One walk over the hashes: within[] takes the range [lo, hi) in (update; only ever set: hash10x.c:535 — ranges accumulate; `first`: within[] holds nothing
// yet and counts as zero, no memset), then per hash wd = 0 outside the range(s), depth + 1 inside (one word tells both) goes to out[] and / or into rowInfo[],
// and the workgroup's largest wd to part[blockIdx.x] — a plain store; good_totals_kernel takes the maximum of those. (An atomic maximum on one word instead, one per
// wave: 40 k of them for 2.6 M hashes made the kernel 65 us slower than the three launches it replaces; one per workgroup, and only where it raises the word, still 20 us.)
constexpr int FILTER_THREADS = 1024;
__global__ __launch_bounds__(FILTER_THREADS)
void depth_filter_kernel(const u32 *__restrict__ depth, u32 hashNumber, int lo, int hi, int update, int first, u8 *__restrict__ within,
                         u32 *__restrict__ out /* null, or wd per hash */, const u64 *__restrict__ rowStart, u32 rowShift,
                         u64 *__restrict__ rowInfo /* null, or per hash: where its barcode list starts (>> rowShift) | wd << 32 */, u32 *__restrict__ part) {
  __shared__ u32 sMax[FILTER_THREADS / WAVE];
  const u32 i = blockIdx.x * FILTER_THREADS + threadIdx.x;
  u32 m = 0;
  if (i < hashNumber) {
    const u32 d = depth[i];
    u8 w = first ? (u8)0 : within[i];
    if (update) { const int n = (int)d; if (n >= lo && n < hi) w = 1; within[i] = w; }
    m = w ? d + 1 : 0;
    if (out) out[i] = m;
    if (rowInfo) rowInfo[i] = (u64)(u32)(rowStart[i] >> rowShift) | ((u64)m << 32);
  }
  for (int s = 32; s; s >>= 1) m = max(m, (u32)__shfl_xor((int)m, s));
  if ((threadIdx.x & (WAVE - 1)) == 0) sMax[threadIdx.x / WAVE] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < FILTER_THREADS / WAVE; ++w) m = max(m, sMax[w]);
    part[blockIdx.x] = m;
  }
}
// What --cluster sizes its launches by, in one launch: tot[0] = largest wd (the maximum over depth_filter_kernel's workgroups), tot[1] = most good hashes of a
// block, tot[2..3] = their sum (64 bits). Up to TOTALS_GROUPS workgroups each reduce a slice and leave {wd, max, sum} in `slot`; the one that draws the last
// ticket (*ticket starts at zero: Ctx::zeros) folds the slots and stores tot with plain stores: tot needs no clearing and may outlive the command (Ctx::goodTotals).
constexpr int TOTALS_THREADS = 1024, TOTALS_GROUPS = 64;
__global__ __launch_bounds__(TOTALS_THREADS)
void good_totals_kernel(const u32 *__restrict__ nGood, u32 nBlocks, const u32 *__restrict__ part, u32 nPart, u32 *slot /* 4 words per workgroup */, u32 *ticket, u32 *__restrict__ tot) {
  __shared__ u32 sMax[TOTALS_THREADS / WAVE], sWd[TOTALS_THREADS / WAVE]; __shared__ unsigned long long sSum[TOTALS_THREADS / WAVE]; __shared__ u32 sLast;
  u32 m = 0, wd = 0; unsigned long long s = 0;
  const u32 stride = gridDim.x * TOTALS_THREADS;
  for (u32 c = blockIdx.x * TOTALS_THREADS + threadIdx.x; c < nBlocks; c += stride) { const u32 n = nGood[c]; m = max(m, n); s += n; }
  for (u32 p = blockIdx.x * TOTALS_THREADS + threadIdx.x; p < nPart; p += stride) wd = max(wd, part[p]);
  for (int sft = 32; sft; sft >>= 1) { m = max(m, (u32)__shfl_xor((int)m, sft)); wd = max(wd, (u32)__shfl_xor((int)wd, sft)); s += __shfl_xor(s, sft); }
  if ((threadIdx.x & (WAVE - 1)) == 0) { sMax[threadIdx.x / WAVE] = m; sWd[threadIdx.x / WAVE] = wd; sSum[threadIdx.x / WAVE] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TOTALS_THREADS / WAVE; ++w) { m = max(m, sMax[w]); wd = max(wd, sWd[w]); s += sSum[w]; }
    u32 *const mine = slot + 4 * blockIdx.x;
    __hip_atomic_store(mine + 0, wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(mine + 1, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 2, (u32)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(mine + 3, (u32)(s >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();                                         // the slot is visible before the ticket is drawn
    sLast = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!sLast || threadIdx.x != 0) return;
  __threadfence();
  m = 0; wd = 0; s = 0;
  for (u32 g = 0; g < gridDim.x; ++g) {
    const u32 *const q = slot + 4 * g;
    wd = max(wd, __hip_atomic_load(q + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); m = max(m, __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    s += (unsigned long long)__hip_atomic_load(q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | ((unsigned long long)__hip_atomic_load(q + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 32);
  }
  tot[0] = wd; tot[1] = m; tot[2] = (u32)s; tot[3] = (u32)(s >> 32);
}

// per block: keys (depth << 16 | position) of its in-range hashes, appended in any order; KT = u32 while the largest
// in-range depth fits 16 bits (the segmented sort then moves half the bytes)
template <typename KT>
__global__ __launch_bounds__(256)
void good_keys_kernel(const h10x_clushash *__restrict__ ch, const u64 *__restrict__ blockOff, const h10x_block *__restrict__ blocks,
                      u32 nBlocks, const u32 *__restrict__ wdepth /* 0 = not in range, else depth + 1 */,
                      KT *__restrict__ key, u32 *__restrict__ nGood, u32 *__restrict__ segEnd, u32 *__restrict__ entries /* sum of depths, saturating */) {
  __shared__ u32 sCount; __shared__ unsigned long long sDepth;
  for (u32 c = blockIdx.x; c < nBlocks; c += gridDim.x) {
    const u64 o = blockOff[c]; const u32 nHash = blocks[c].nHash;
    __syncthreads();
    if (threadIdx.x == 0) { sCount = 0; sDepth = 0; }
    __syncthreads();
    unsigned long long myDepth = 0;
    if (nHash <= 65535) {                                    // hash10x.c:748-753: bigger blocks are ignored
      for (u32 base = 0; base < nHash; base += blockDim.x) {
        const u32 p = base + threadIdx.x;
        u32 wd = 0; bool good = false;
        if (p < nHash) { wd = wdepth[ch[o + p].hash]; good = wd != 0; if (good) myDepth += wd - 1; }
        const u64 bal = __ballot(good);
        const int lane = threadIdx.x & (WAVE - 1);
        u32 wb = 0;
        if (lane == 0 && bal) wb = atomicAdd(&sCount, (u32)__popcll(bal));
        wb = __shfl(wb, 0);
        if (good) key[o + wb + (u32)__popcll(bal & ((1ULL << lane) - 1))] = (KT)(((KT)(wd - 1) << 16) | (KT)p);
      }
    }
    for (int sft = 32; sft; sft >>= 1) myDepth += __shfl_down(myDepth, sft);
    if ((threadIdx.x & (WAVE - 1)) == 0 && myDepth) atomicAdd(&sDepth, myDepth);
    __syncthreads();
    if (threadIdx.x == 0) { nGood[c] = sCount; segEnd[c] = (u32)o + sCount; entries[c] = sDepth > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)sDepth; }
  }
}
template <typename KT>
__global__ void good_pos_kernel(const KT *__restrict__ key, u64 n, u16 *__restrict__ pos) {
  u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (; i < n; i += stride) pos[i] = (u16)(key[i] & 0xFFFF);
}
__global__ void offsets32c_kernel(const u64 *__restrict__ off, u32 n, u32 *__restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (u32)off[i];
}

// The good list of a block in one workgroup: the in-range hashes' depths as keys, their positions as values, sorted in LDS
// (rocPRIM block radix sort, stable), positions written out — instead of key kernel + device-wide segmented sort + position
// kernel. Blocks up to BLOCK_SORT_MAX entries, depths below 2^16; three launch classes by block size like clushash_block_kernel.
// Round 5: ONE random read per entry. The chip does some 55 G independent random reads a second whatever the table's size (scratch/r5_gather_rate.hip: 64 MB .. 4 GB
// tables, 1 .. 8 byte entries, all within 15 %), and this kernel used to make two — the depth byte of every entry, then the list offset of every good one: 4.1 G look-ups
// in 72 ms on the 3 Gb set, i.e. at that wall. rowInfo[] (within_depth_kernel) holds both in a word; the offset rides through the sort as part of the value.
template <int THREADS, int IPT>
__global__ __launch_bounds__(THREADS)
void good_block_kernel(const h10x_clushash *__restrict__ ch, const u64 *__restrict__ blockOff, const h10x_block *__restrict__ blocks,
                       const u32 *__restrict__ list, const u32 *__restrict__ count /* this class's blocks: stageB_blockClassLists */,
                       const u64 *__restrict__ rowInfo /* per hash: list offset | (0 = not in range, else depth + 1) << 32 */, int sortBits,
                       u16 *__restrict__ goodPos, u32 *__restrict__ nGood, u32 *__restrict__ entries /* sum of depths, saturating */,
                       u64 *__restrict__ goodRow /* list descriptor per rank: see good_rows_kernel */) {
  using Sort = rocprim::block_radix_sort<u32, THREADS, IPT, u64>;
  __shared__ typename Sort::storage_type storage;
  __shared__ u32 sCount; __shared__ unsigned long long sDepth;
  const u32 nList = *count;
  for (u32 wi = blockIdx.x; wi < nList; wi += gridDim.x) {
    const u32 c = list[wi];
    const u32 nHash = blocks[c].nHash;                       // (the smallest class also takes the empty blocks: their counts are written too)
    const u64 o = blockOff[c];
    __syncthreads();
    if (threadIdx.x == 0) { sCount = 0; sDepth = 0; }
    __syncthreads();
    // blocked arrangement: a thread holds IPT consecutive positions, so the positions are ascending in the order the sort
    // takes as given, and a STABLE sort on the depth bits alone (one 8-bit pass for depths below 128, where depth and
    // position in one key needed three) leaves equal depths in ascending position
    u32 k[IPT]; u64 v[IPT]; u32 mine = 0; unsigned long long myDepth = 0;
#pragma unroll
    for (int j = 0; j < IPT; ++j) { k[j] = 0xFFFFFFFFu; v[j] = threadIdx.x * IPT + (u32)j; }
    if (nHash) {
      // (positions past the block's end read its last record: loads without a branch around them — written as `if (p < nHash) load` every entry was a branch, a load and a
      // wait of its own, twelve memory latencies in a row per lane — the IPT records and then the IPT look-ups are in flight together)
      u32 hs[IPT]; u64 ri[IPT];
#pragma unroll
      for (int j = 0; j < IPT; ++j) { const u32 p = threadIdx.x * IPT + (u32)j; hs[j] = ch[o + (p < nHash ? p : nHash - 1)].hash; }
#pragma unroll
      for (int j = 0; j < IPT; ++j) ri[j] = rowInfo[hs[j]];
#pragma unroll
      for (int j = 0; j < IPT; ++j) {
        const u32 p = threadIdx.x * IPT + (u32)j; const u32 wd = (u32)(ri[j] >> 32);
        if (p < nHash && wd) { k[j] = wd - 1; ++mine; myDepth += wd - 1; v[j] = (u64)p | ((ri[j] & 0xFFFFFFFFull) << 16); }   // value: position (16 bits: blocks of at most BLOCK_SORT_MAX entries) | list offset << 16
      }
    }
    for (int sft = 32; sft; sft >>= 1) { mine += (u32)__shfl_down((int)mine, sft); myDepth += __shfl_down(myDepth, sft); }
    if ((threadIdx.x & (WAVE - 1)) == 0 && mine) { atomicAdd(&sCount, mine); atomicAdd(&sDepth, myDepth); }
    Sort().sort_to_striped(k, v, storage, 0, sortBits);      // ascending (depth, position): hash10x.c:726-730,758; padding keys last
    __syncthreads();
    const u32 nG = sCount;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {                          // striped: coalesced stores
      const u32 e = (u32)j * THREADS + threadIdx.x;
      if (e < nG) {
        goodPos[o + e] = (u16)v[j];
        // where the rank's barcode list lies and how long it is (the sort key IS the depth): the cluster kernel streams these
        // instead of gathering position -> hash index -> offset, depth per barcode
        goodRow[o + e] = (u64)(u32)(v[j] >> 16) | ((u64)k[j] << 32);
      }
    }
    if (threadIdx.x == 0) { nGood[c] = nG; entries[c] = sDepth > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)sDepth; }
  }
}

// ---- list descriptors: per good hash of a block, in rank order, where its barcode list starts in rows[] and how long it is.
// Built once per --hashDepthRange (after the list exchange of a sharded run), read by every --cluster that follows: the
// cluster kernel used to fetch them per barcode through three dependent gathers (position -> hash index -> offset, depth)
// into LDS arrays of 6 bytes per rank.
__global__ __launch_bounds__(256)
void good_rows_kernel(const h10x_clushash *__restrict__ ch, const u64 *__restrict__ blockOff, const u32 *__restrict__ nGood, const u16 *__restrict__ goodPos, u32 nBlocks,
                      const u32 *__restrict__ hashDepth, const u64 *__restrict__ rowStart, u32 rowShift, u64 *__restrict__ goodRow) {
  for (u32 c = blockIdx.x; c < nBlocks; c += gridDim.x) {
    const u32 n = nGood[c]; const u64 o = blockOff[c];
    for (u32 i = threadIdx.x; i < n; i += blockDim.x) {
      const u32 x = ch[o + goodPos[o + i]].hash;
      goodRow[o + i] = (u64)(u32)(rowStart[x] >> rowShift) | ((u64)hashDepth[x] << 32);
    }
  }
}

int stageC_depthRange(Ctx *c, int lo, int hi) {
  hipStream_t st = c->stream; PrimTemp pt;
  if (!c->haveState) return c->fail("no hash state loaded: use readFQB or readHash first");
  c->haveGood = false; c->goodFiguresPending = false;        // (a call that fails half-way must not leave the lists of an earlier one standing: rows[] and the offsets are replaced below)
  ZeroScope zeroScope(c); H10X_TRY(zeroScope.rc);
  c->tstart(T_GOOD);
  const u32 U1 = c->hashNumber; const u32 nBlocks = c->nBlocks; const u64 H = c->nEntries;
  const bool newRange = !(c->haveRange && lo == c->rangeMin && hi == c->rangeMax);       // hash10x.c:530: the same range again changes nothing in within[]
  const bool firstRange = !c->haveRange;                     // within[] holds nothing yet: depth_filter_kernel starts it from zero (no clear)
  if (newRange && firstRange) H10X_HIP(c, c->within.alloc(U1));
  const unsigned filterGrid = divUp(U1, FILTER_THREADS);
  DevBuf<u32> wdPart; H10X_HIP(c, wdPart.alloc(filterGrid));  // per workgroup of the filter: largest in-range depth + 1
  if (!c->goodTotals.p) H10X_HIP(c, c->goodTotals.alloc(4));
  // the totals' launch: its workgroups, their slots, and a ticket word per launch (the device-wide sort path makes one ahead of time for the depth figure alone)
  const unsigned totalsGrid = hmax<u32>(1u, hmin<u32>((u32)TOTALS_GROUPS, divUp(hmax<u32>(nBlocks, filterGrid), TOTALS_THREADS)));
  DevBuf<u32> totSlots, earlyTot; H10X_HIP(c, totSlots.alloc(4 * (size_t)TOTALS_GROUPS));
  u32 *const tickets = c->zeros(2); if (!tickets) return -1;
  auto noteRange = [&]() { c->haveRange = true; c->rangeMin = lo; c->rangeMax = hi; if (hi > 0 && (u32)hi > c->rangeHiMax) c->rangeHiMax = (u32)hi; };
  // sharded: the barcode lists of the in-range hashes come from their owners first (they depend on the ranges alone), so that
  // the good lists below can point into them — within[] is brought up to date in a launch of its own in front of the exchange
  XGuard xGuard(c);                                          // (the lists may still be arriving on the exchange stream when this function leaves early)
  bool updated = !newRange;
  if (c->sharded) {
    if (newRange) {
      depth_filter_kernel<<<filterGrid, FILTER_THREADS, 0, st>>>(c->hashDepth.p, U1, lo, hi, 1, firstRange ? 1 : 0, c->within.p, nullptr, nullptr, 0u, nullptr, wdPart.p);
      noteRange(); updated = true;
    }
    c->tstop(T_GOOD); H10X_TRY(shard_exchangeRows(c)); c->tstart(T_GOOD);
  }
  // goodHashesBuild (hash10x.c:738-766)
  DevBuf<u64> key, keyS; DevBuf<u32> key32, keyS32, off32, segEnd, wdepth;
  H10X_HIP(c, c->nGood.alloc(nBlocks)); H10X_HIP(c, c->goodPos.alloc(H)); H10X_HIP(c, c->goodEntries.alloc(nBlocks)); H10X_HIP(c, c->goodRow.alloc(H));
  // no in-range depth exceeds this, known without a round trip: the data set's barcode count (Ctx::depthBound) or the ranges' limit
  const u32 hiMax = (!updated && hi > 0 && (u32)hi > c->rangeHiMax) ? (u32)hi : c->rangeHiMax;      // (rangeHiMax as it stands once this range is in)
  const u32 goodDepthBound = hmin<u32>(c->depthBound, hiMax ? hiMax - 1 : 0);
  const bool narrow = goodDepthBound <= 65535u;
  const bool byBlocks = narrow && c->maxBlockHashes <= BLOCK_SORT_MAX;       // every block's list is built and sorted by one workgroup
  DevBuf<u64> rowInfo;
  if (byBlocks) H10X_HIP(c, rowInfo.alloc(U1));              // (wdepth[] and off32[] serve the device-wide sort path only)
  else { H10X_HIP(c, wdepth.alloc(U1)); H10X_HIP(c, off32.alloc((size_t)nBlocks + 1)); H10X_HIP(c, segEnd.alloc(nBlocks)); }
  depth_filter_kernel<<<filterGrid, FILTER_THREADS, 0, st>>>(c->hashDepth.p, U1, lo, hi, updated ? 0 : 1, !updated && firstRange ? 1 : 0, c->within.p, wdepth.p,
                                                     c->rowStart.p, (u32)c->rowShift, rowInfo.p, wdPart.p);
  if (!updated) noteRange();
  if (byBlocks) {
    int db = 1; while (db < 16 && (goodDepthBound >> db)) ++db;
    const int sortBits = db + 1;                                              // one bit more than the largest depth: padding keys sort last
    DevBuf<u32> lists; u32 *counts = nullptr;
    H10X_TRY(stageB_blockClassLists(c, lists, counts));
    const unsigned gridBig = hmin<u32>(nBlocks, (u32)c->numCU * 8), gridSmall = hmin<u32>(nBlocks, 65535u * 4);
    const int side = c->maxBlockHashes > BLOCK_SORT_CAP1 ? 2 : (c->maxBlockHashes > BLOCK_SORT_CAP0 ? 1 : 0);
    ForkGuard forkGuard(c);
    if (side) H10X_TRY(c->forkStreams(side));
#define H10X_GOOD_LAUNCH(T, I, CLS, STREAM)                                                                                         \
    { const u32 *const L = lists.p + (size_t)CLS * nBlocks, *const N = counts + CLS; const unsigned grid = CLS == 0 ? gridSmall : gridBig; \
      good_block_kernel<T, I><<<grid, T, 0, STREAM>>>(c->clusHash.p, c->blockOff.p, c->blocks.p, L, N, rowInfo.p, sortBits, c->goodPos.p, c->nGood.p, c->goodEntries.p, c->goodRow.p); }
    H10X_GOOD_LAUNCH(H10X_BS_T0, H10X_BS_I0, 0, st)
    if (side >= 1) H10X_GOOD_LAUNCH(H10X_BS_T1, H10X_BS_I1, 1, c->aux[0])
    if (side >= 2) H10X_GOOD_LAUNCH(1024, 8, 2, c->aux[1])
#undef H10X_GOOD_LAUNCH
    H10X_TRY(c->faultAt(3));
    if (side) H10X_TRY(c->joinStreams(side));
    forkGuard.done();
  }
  else if (narrow) { H10X_HIP(c, key32.alloc(H)); H10X_HIP(c, keyS32.alloc(H)); } else { H10X_HIP(c, key.alloc(H)); H10X_HIP(c, keyS.alloc(H)); }
  if (byBlocks) {}
  else if (narrow) good_keys_kernel<u32><<<hmin<u32>(nBlocks, 16384), 256, 0, st>>>(c->clusHash.p, c->blockOff.p, c->blocks.p, nBlocks, wdepth.p,
                                                                             key32.p, c->nGood.p, segEnd.p, c->goodEntries.p);
  else good_keys_kernel<u64><<<hmin<u32>(nBlocks, 16384), 256, 0, st>>>(c->clusHash.p, c->blockOff.p, c->blocks.p, nBlocks, wdepth.p,
                                                                      key.p, c->nGood.p, segEnd.p, c->goodEntries.p);
  u32 hWd = 0;                                               // the sort below is made over the bits of the largest in-range depth: that path fetches it here
  if (H && !byBlocks) {
    H10X_HIP(c, earlyTot.alloc(4));                          // (the depth figure alone, ahead of time, into a record of its own: Ctx::goodTotals is written once, at the end)
    good_totals_kernel<<<totalsGrid, TOTALS_THREADS, 0, st>>>(c->nGood.p, 0u, wdPart.p, filterGrid, totSlots.p, tickets + 1, earlyTot.p);
    H10X_TRY(c->readback(&hWd, earlyTot.p, 4));
    H10X_TRY(c->syncReadbacks());
    offsets32c_kernel<<<divUp((u64)nBlocks + 1, 256), 256, 0, st>>>(c->blockOff.p, nBlocks + 1, off32.p);
  }
  const u32 hr[1] = {hWd ? hWd - 1 : 0};                      // (depth + 1)
  // ascending (depth, position): qsort by depth, stable => ties by position (hash10x.c:726-730,758)
  if (H && !byBlocks) {
    if (narrow) {
      H10X_TRY(prim_seg_sort_keys_u32(c, pt, key32.p, keyS32.p, (u32)H, nBlocks, off32.p, segEnd.p, 0, 16 + bitsFor(hr[0])));
      good_pos_kernel<u32><<<(unsigned)hmin<u64>(divUp(H, 256), 65535u * 2), 256, 0, st>>>(keyS32.p, H, c->goodPos.p);
    } else {
      H10X_TRY(prim_seg_sort_keys_u64(c, pt, key.p, keyS.p, (u32)H, nBlocks, off32.p, segEnd.p, 0, 16 + bitsFor(hr[0])));
      good_pos_kernel<u64><<<(unsigned)hmin<u64>(divUp(H, 256), 65535u * 2), 256, 0, st>>>(keyS.p, H, c->goodPos.p);
    }
  }
  // list descriptors per good hash, in rank order: written by good_block_kernel; the device-wide sort path adds them here
  if (!byBlocks && nBlocks) good_rows_kernel<<<hmin<u32>(nBlocks, 65535u * 4), 256, 0, st>>>(c->clusHash.p, c->blockOff.p, c->nGood.p, c->goodPos.p, nBlocks, c->hashDepth.p, c->rowStart.p,
                                                                                           (u32)c->rowShift, c->goodRow.p);
  // the figures --cluster sizes its launches by stay on the device (Ctx::goodTotals) until a command asks for them: an unsharded --hashDepthRange
  // ends without draining the queue, and the next command's launches queue up behind this one's
  good_totals_kernel<<<totalsGrid, TOTALS_THREADS, 0, st>>>(c->nGood.p, nBlocks, wdPart.p, filterGrid, totSlots.p, tickets, c->goodTotals.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(c->xJoin());                                      // sharded: the in-range lists have arrived before anything queued from here on runs (and before the next collective)
  c->goodFiguresPending = true;
  if (c->sharded) H10X_TRY(c->needGoodFigures());            // (sharded contexts keep the round trip here)
  c->haveGood = true;
  c->tstop(T_GOOD);
  return 0;
}

// maxGoodDepth, maxGood and meanGood of the last --hashDepthRange: fetched from the device the first time they are wanted
int Ctx::needGoodFigures() {
  if (!goodFiguresPending) return 0;
  u32 t[4] = {0, 0, 0, 0};
  H10X_TRY(readback(t, goodTotals.p, 16));
  H10X_TRY(syncReadbacks());
  maxGoodDepth = t[0] ? t[0] - 1 : 0;                        // goodTotals[0] holds depth + 1
  maxGood = t[1];
  const u64 sumGood = (u64)t[2] | ((u64)t[3] << 32);
  meanGood = nBlocks > 1 ? (u32)(sumGood / (nBlocks - 1)) : 0;
  goodFiguresPending = false;
  return 0;
}

__global__ void warm_stageCGood_kernel() {}
void warm_stageCGood(hipStream_t st) { warm_stageCGood_kernel<<<1, 1, 0, st>>>(); }

}  // namespace h10x
