// stage_f.hip — the neighbour census behind --hashInfo / --hashExplore / --doubleShared / --errorFix / --shareScan.
//
// For a query hash x the reference (hashNeighbours / countHashNeighbours, hash10x.c:541-586) walks every barcode block
// that holds x (hashCodes[x]) and every ClusterHash record of those blocks, keeps h != x with hashWithinRange[h], and
// counts per h the blocks it shares with x: c_x(h). Its cost is sum over x's blocks of nHash. Here a batch of queries
// runs as one gather, one device-wide sort and one pass over the runs:
//   gather   one wave per (query, block of the query): the block's records in the batch's hash window, filtered, written
//            as key = slot << hbits | h (slot = the query's position in the batch) at positions reserved once per block;
//   sort     prim_sort_keys_u64 on the bits in use (hbits + bits of the slot);
//   runs     a run of equal keys is one neighbour h of one query with c = run length. Three reductions: the list
//            (h, c, lowest barcode of h) by a scan of the run heads, per query the max of (c mod 2^16) << 32 | h and |N(x)|
//            by 64-bit atomics, or H_x[c] += 1 into the caller's per-query histogram regions.
// Batches are cut by gathered records against a budget (option "neighbour_budget"); a query larger than the budget runs
// alone in windows of hash index, found by binary search in each block's clusHash list (sorted by index).
#include "common.hpp"
#include "prim.hpp"

namespace h10x {

enum { NB_LIST = 0, NB_MAX = 1, NB_HIST = 2 };
static constexpr u64 NB_DEFAULT_BUDGET = 1ull << 26;       // gathered records per batch: 2 x 8 bytes each for the sort = 1 GiB

static int nbBits(u64 v) { int b = 1; while (b < 64 && (v >> b)) ++b; return b; }

// records [a, b) of block blk with hash index in [lo, hi); full = the window covers every index
__device__ __forceinline__ void nb_window(const h10x_clushash *__restrict__ ch, const u64 *__restrict__ blockOff, u32 blk, u32 lo, u32 hi, bool full,
                                          u64 &a, u64 &b) {
  a = blockOff[blk]; b = blockOff[blk + 1];
  if (full) return;
  u64 l = a, r = b;
  while (l < r) { const u64 m = (l + r) >> 1; if (ch[m].hash < lo) l = m + 1; else r = m; }
  const u64 s = l; r = b;
  while (l < r) { const u64 m = (l + r) >> 1; if (ch[m].hash < hi) l = m + 1; else r = m; }
  a = s; b = l;
}

// one wave per query: records of its blocks in the window (size), and its depth
__global__ void nb_size_kernel(const u32 *__restrict__ xs, u32 nq, const u32 *__restrict__ depth, const u64 *__restrict__ rowStart,
                               const u32 *__restrict__ rows, const u64 *__restrict__ blockOff, const h10x_clushash *__restrict__ ch,
                               u32 lo, u32 hi, int full, u64 *__restrict__ size, u32 *__restrict__ qDepth) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 q = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (q >= nq) return;
  const u32 x = xs[q], d = depth[x]; const u64 rs = rowStart[x];
  u64 s = 0;
  for (u32 i = lane; i < d; i += WAVE) { u64 a, b; nb_window(ch, blockOff, rows[rs + i], lo, hi, full != 0, a, b); s += b - a; }
  for (int k = 32; k; k >>= 1) s += __shfl_xor(s, k);
  if (lane == 0) { size[q] = s; qDepth[q] = d; }
}

// one wave per unit (query, i-th block of the query); unitBase[q] = first unit of query q, unitBase[nq] = units
__global__ __launch_bounds__(256) void nb_gather_kernel(const u32 *__restrict__ xs, u32 nq, const u64 *__restrict__ unitBase,
                                                        const u64 *__restrict__ rowStart, const u32 *__restrict__ rows,
                                                        const u64 *__restrict__ blockOff, const h10x_clushash *__restrict__ ch,
                                                        const u8 *__restrict__ within, u32 lo, u32 hi, int full, int hbits,
                                                        u64 cap, u64 *__restrict__ keys, unsigned long long *__restrict__ nKept) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u64 units = unitBase[nq];
  const u64 w0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE, wStride = ((u64)gridDim.x * blockDim.x) / WAVE;
  for (u64 u = w0; u < units; u += wStride) {
    u32 l = 0, r = nq;                                        // the query: last q with unitBase[q] <= u
    while (r - l > 1) { const u32 m = (l + r) >> 1; if (unitBase[m] <= u) l = m; else r = m; }
    const u32 q = l, x = xs[q];
    const u32 blk = rows[rowStart[x] + (u - unitBase[q])];
    u64 a, b; nb_window(ch, blockOff, blk, lo, hi, full != 0, a, b);
    const u64 slot = (u64)q << hbits;
    // two passes over the block's records (the second from cache): the wave reserves its output with ONE atomic per block. One per 64
    // records was the command's wall — 5.6 of 10 s on the yeast-like set, all waves on a single counter
    u64 cnt = 0;
    for (u64 e = a; e < b; e += WAVE) {                       // wave-uniform trip counts
      const u64 j = e + lane;
      bool keep = false;
      if (j < b) { const u32 h = ch[j].hash; keep = h != x && within[h]; }
      cnt += __popcll(__ballot(keep));
    }
    if (!cnt) continue;
    unsigned long long p0 = 0;
    if (lane == 0) p0 = atomicAdd(nKept, (unsigned long long)cnt);
    p0 = __shfl(p0, 0);
    for (u64 e = a; e < b; e += WAVE) {
      const u64 j = e + lane;
      u32 h = 0; bool keep = false;
      if (j < b) { h = ch[j].hash; keep = h != x && within[h]; }
      const u64 m = __ballot(keep);
      const u64 p = p0 + __popcll(m & ((1ull << lane) - 1));
      if (keep && p < cap) keys[p] = slot | h;               // p < cap always (cap = records in the window); the test keeps a miscount in bounds
      p0 += __popcll(m);
    }
  }
}

// a run of equal keys = one neighbour of one query. LIST: head[i] = 1 at a run's first key, cnt[i] = its length; MAX: per-query atomics.
template <int MODE>
__global__ void nb_run_kernel(const u64 *__restrict__ keys, u64 n, int hbits, u32 *__restrict__ head, u32 *__restrict__ cnt,
                              unsigned long long *__restrict__ maxKey, u32 *__restrict__ nNb) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u64 k = keys[i];
    if (i && keys[i - 1] == k) { if (MODE == NB_LIST) head[i] = 0; continue; }
    u64 j = i + 1; while (j < n && keys[j] == k) ++j;
    const u64 c = j - i; const u32 slot = (u32)(k >> hbits), h = (u32)(k & (((u64)1 << hbits) - 1));
    if (MODE == NB_LIST) { head[i] = 1; cnt[i] = (u32)c; }
    else if (MODE == NB_MAX) { atomicMax(&maxKey[slot], ((unsigned long long)(c & 0xFFFF) << 32) | h); atomicAdd(&nNb[slot], 1u); }
  }
}

// HIST: H_x[c] += 1 per run. Neighbouring runs mostly share the query and their count (most c are 1 .. 3), so the lanes of a wave that hit the
// same bin add once: one atomic per distinct bin of the wave instead of one per run (on the yeast-like set 37 % of the command went to
// per-run atomics on a few hot bins). The loop is wave-uniform: i0 steps by whole workgroups.
__global__ void nb_hist_kernel(const u64 *__restrict__ keys, u64 n, int hbits, const u64 *__restrict__ histOff, const u32 *__restrict__ qDepth,
                               u32 *__restrict__ hist) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const u32 lane = threadIdx.x & (WAVE - 1);
  for (u64 i0 = (u64)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
    const u64 i = i0 + threadIdx.x;
    bool act = false; u64 addr = 0;
    if (i < n) {
      const u64 k = keys[i];
      if (!i || keys[i - 1] != k) {
        u64 j = i + 1; while (j < n && keys[j] == k) ++j;
        const u64 c = j - i; const u32 slot = (u32)(k >> hbits);
        act = c <= qDepth[slot];                                // c <= depth(x) always: x is in at most depth(x) blocks
        addr = histOff[slot] + c;
      }
    }
    u64 pending = __ballot(act);
    while (pending) {
      const int leader = __ffsll((unsigned long long)pending) - 1;
      const u64 la = __shfl(addr, leader);
      const u64 same = __ballot(act && addr == la);
      if ((int)lane == leader) atomicAdd(&hist[la], (u32)__popcll(same));
      if (addr == la) act = false;
      pending &= ~same;
    }
  }
}

__global__ void nb_emit_kernel(const u64 *__restrict__ keys, u64 n, int hbits, const u32 *__restrict__ head, const u32 *__restrict__ cnt,
                               const u32 *__restrict__ pos, const u64 *__restrict__ rowStart, const u32 *__restrict__ rows,
                               u32 *__restrict__ oHash, u32 *__restrict__ oCount, u32 *__restrict__ oFirst) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (!head[i]) continue;
    const u32 h = (u32)(keys[i] & (((u64)1 << hbits) - 1)), p = pos[i];
    oHash[p] = h; oCount[p] = cnt[i]; oFirst[p] = rows[rowStart[h]];   // *arr(hashCodes, h, U32*): the lowest barcode of h
  }
}

// ---------------------------------------------------------------------------------------------------------- driver
namespace {
struct Census {
  Ctx *c; int mode; u64 budget;
  const u32 *dXs = nullptr;                 // all queries (device)
  std::vector<u64> size; std::vector<u32> depth;
  // outputs: NB_MAX per query (device, whole call), NB_HIST regions (device), NB_LIST host vectors
  unsigned long long *dMax = nullptr; u32 *dNb = nullptr; const u64 *dHistOff = nullptr; const u32 *dQDepth = nullptr; u32 *dHist = nullptr;
  std::vector<u32> lHash, lCount, lFirst;
  DevBuf<u64> keys, keys2; DevBuf<u64> unitBase; DevBuf<unsigned long long> nKept; DevBuf<u32> head, cnt, pos, oHash, oCount, oFirst;
  PrimTemp pt;

  int sizes(const u32 *dX, u32 nq, u32 lo, u32 hi, bool full, u64 *hSize, u32 *hDepth) {
    DevBuf<u64> s; DevBuf<u32> d; hipStream_t st = c->stream;
    H10X_HIP(c, s.alloc(nq)); H10X_HIP(c, d.alloc(nq));
    nb_size_kernel<<<divUp((u64)nq * WAVE, 256), 256, 0, st>>>(dX, nq, c->hashDepth.p, c->rowStart.p, c->rows.p, c->blockOff.p, c->clusHash.p,
                                                              lo, hi, full ? 1 : 0, s.p, d.p);
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(hSize, s.p, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    if (hDepth) H10X_HIP(c, hipMemcpyAsync(hDepth, d.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  // queries [q0, q0 + nq) of the call in the window [lo, hi); total = records gathered
  int batch(u32 q0, u32 nq, u32 lo, u32 hi, bool full, u64 total) {
    hipStream_t st = c->stream;
    c->nbStats[2] += 1;
    if (!total) return 0;
    std::vector<u64> ub(nq + 1); ub[0] = 0;
    for (u32 q = 0; q < nq; ++q) ub[q + 1] = ub[q] + depth[q0 + q];
    H10X_HIP(c, unitBase.alloc(nq + 1));
    H10X_HIP(c, hipMemcpyAsync(unitBase.p, ub.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    if (keys.n < total) { H10X_HIP(c, keys.alloc(total)); H10X_HIP(c, keys2.alloc(total)); }
    if (!nKept.p) H10X_HIP(c, nKept.alloc(1));
    H10X_HIP(c, hipMemsetAsync(nKept.p, 0, 8, st));
    const int hbits = nbBits(c->hashNumber), endBit = hbits + nbBits(nq - 1);
    const unsigned g = (unsigned)hmin<u64>(divUp(ub[nq], 4), 65536);
    nb_gather_kernel<<<g, 256, 0, st>>>(dXs + q0, nq, unitBase.p, c->rowStart.p, c->rows.p, c->blockOff.p, c->clusHash.p, c->within.p,
                                        lo, hi, full ? 1 : 0, hbits, total, keys.p, nKept.p);
    H10X_HIP(c, hipGetLastError());
    unsigned long long n = 0;
    H10X_TRY(c->readback(&n, nKept.p, 8)); H10X_TRY(c->syncReadbacks());
    if (n > total) return c->fail("neighbour census: %llu records kept of %llu gathered", n, (u64)total);
    c->nbStats[0] += total; c->nbStats[1] += n;
    if (!n) return 0;
    H10X_TRY(prim_sort_keys_u64(c, pt, keys.p, keys2.p, n, 0, endBit));
    const unsigned gr = (unsigned)hmin<u64>(divUp(n, 256), 16384);
    if (mode == NB_MAX) {
      nb_run_kernel<NB_MAX><<<gr, 256, 0, st>>>(keys2.p, n, hbits, nullptr, nullptr, dMax + q0, dNb + q0);
    } else if (mode == NB_HIST) {
      nb_hist_kernel<<<gr, 256, 0, st>>>(keys2.p, n, hbits, dHistOff + q0, dQDepth + q0, dHist);
    } else {
      H10X_HIP(c, head.alloc(n)); H10X_HIP(c, cnt.alloc(n)); H10X_HIP(c, pos.alloc(n));
      nb_run_kernel<NB_LIST><<<gr, 256, 0, st>>>(keys2.p, n, hbits, head.p, cnt.p, nullptr, nullptr);
      H10X_TRY(prim_exclusive_scan_u32(c, pt, head.p, pos.p, n));
      u32 lastPos = 0, lastHead = 0;
      H10X_HIP(c, hipMemcpyAsync(&lastPos, pos.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(&lastHead, head.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipStreamSynchronize(st));
      const u64 runs = (u64)lastPos + lastHead;
      H10X_HIP(c, oHash.alloc(runs)); H10X_HIP(c, oCount.alloc(runs)); H10X_HIP(c, oFirst.alloc(runs));
      nb_emit_kernel<<<gr, 256, 0, st>>>(keys2.p, n, hbits, head.p, cnt.p, pos.p, c->rowStart.p, c->rows.p, oHash.p, oCount.p, oFirst.p);
      const size_t at = lHash.size();
      lHash.resize(at + runs); lCount.resize(at + runs); lFirst.resize(at + runs);
      H10X_HIP(c, hipMemcpyAsync(lHash.data() + at, oHash.p, runs * 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(lCount.data() + at, oCount.p, runs * 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(lFirst.data() + at, oFirst.p, runs * 4, hipMemcpyDeviceToHost, st));
    }
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  // one query above the budget: windows of hash index, halved until their records fit (a window of one index always runs)
  int windowed(u32 q, u32 lo, u32 hi, u64 records) {
    if (!records) return 0;
    if (records <= budget || hi - lo <= 1) { c->nbStats[3] += 1; return batch(q, 1, lo, hi, false, records); }
    const u32 mid = lo + (hi - lo) / 2;
    u64 left = 0; H10X_TRY(sizes(dXs + q, 1, lo, mid, false, &left, nullptr));
    H10X_TRY(windowed(q, lo, mid, left));
    return windowed(q, mid, hi, records - left);
  }

  int run(u32 nq) {
    for (u32 q0 = 0; q0 < nq;) {
      if (size[q0] > budget) { H10X_TRY(windowed(q0, 0, c->hashNumber, size[q0])); ++q0; continue; }
      u32 q1 = q0; u64 sum = 0;
      while (q1 < nq && size[q1] <= budget && sum + size[q1] <= budget) sum += size[q1++];
      H10X_TRY(batch(q0, q1 - q0, 0, c->hashNumber, true, sum));
      q0 = q1;
    }
    return 0;
  }
};

int nb_check(Ctx *c, const u32 *xs, u32 nq) {
  if (!c->haveState) return c->fail("no hash state loaded: use readFQB or readHash first");
  if (c->sharded) return c->fail("neighbour census: not available on a sharded context (one rank holds only its own barcodes)");
  if (!c->haveRange) return c->fail("neighbour census called without hashDepthRange");
  for (u32 q = 0; q < nq; ++q)
    if (xs[q] >= c->hashNumber) return c->fail("neighbour census: hash %u is not below hashNumber %u", xs[q], c->hashNumber);
  return 0;
}

int nb_begin(Ctx *c, Census &k, DevBuf<u32> &dX, const u32 *xs, u32 nq) {
  k.budget = c->optNbBudget > 0 ? (u64)c->optNbBudget : NB_DEFAULT_BUDGET;
  H10X_HIP(c, dX.alloc(nq));
  H10X_HIP(c, hipMemcpyAsync(dX.p, xs, (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
  k.dXs = dX.p; k.size.resize(nq); k.depth.resize(nq);
  return k.sizes(dX.p, nq, 0, c->hashNumber, true, k.size.data(), k.depth.data());
}
}  // namespace

int stageF_neighbours(Ctx *c, u32 x, u32 *hash, u32 *count, u32 *first, u64 cap, u64 *n) {
  H10X_TRY(nb_check(c, &x, 1));
  Census k; k.c = c; k.mode = NB_LIST; DevBuf<u32> dX;
  H10X_TRY(nb_begin(c, k, dX, &x, 1));
  H10X_TRY(k.run(1));
  *n = k.lHash.size();
  const size_t m = (size_t)hmin<u64>(cap, k.lHash.size());
  if (m && hash) memcpy(hash, k.lHash.data(), m * 4);
  if (m && count) memcpy(count, k.lCount.data(), m * 4);
  if (m && first) memcpy(first, k.lFirst.data(), m * 4);
  return 0;
}

int stageF_neighbourMax(Ctx *c, const u32 *xs, u32 nq, u64 *maxKey, u32 *nNb) {
  H10X_TRY(nb_check(c, xs, nq));
  if (!nq) return 0;
  Census k; k.c = c; k.mode = NB_MAX; DevBuf<u32> dX; DevBuf<unsigned long long> dMax; DevBuf<u32> dNb;
  H10X_TRY(nb_begin(c, k, dX, xs, nq));
  H10X_HIP(c, dMax.alloc(nq)); H10X_HIP(c, dNb.alloc(nq));
  H10X_HIP(c, hipMemsetAsync(dMax.p, 0, (size_t)nq * 8, c->stream)); H10X_HIP(c, hipMemsetAsync(dNb.p, 0, (size_t)nq * 4, c->stream));
  k.dMax = dMax.p; k.dNb = dNb.p;
  H10X_TRY(k.run(nq));
  H10X_HIP(c, hipMemcpyAsync(maxKey, dMax.p, (size_t)nq * 8, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipMemcpyAsync(nNb, dNb.p, (size_t)nq * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int stageF_neighbourHist(Ctx *c, const u32 *xs, u32 nq, const u64 *offsets, u32 *hist) {
  H10X_TRY(nb_check(c, xs, nq));
  if (!nq) return 0;
  Census k; k.c = c; k.mode = NB_HIST; DevBuf<u32> dX;
  H10X_TRY(nb_begin(c, k, dX, xs, nq));
  for (u32 q = 0; q < nq; ++q)                               // region q = [offsets[q], offsets[q + 1]) holds H_x[0 .. depth(x)]
    if (offsets[q + 1] < offsets[q] || offsets[q + 1] - offsets[q] < (u64)k.depth[q] + 1)
      return c->fail("h10x_neighbour_hist: region %u holds %llu bins, hash %u needs depth + 1 = %u", q, (u64)(offsets[q + 1] - offsets[q]), xs[q], k.depth[q] + 1);
  const u64 total = offsets[nq];
  DevBuf<u64> dOff; DevBuf<u32> dHist;
  H10X_HIP(c, dOff.alloc(nq)); H10X_HIP(c, dHist.alloc(total));
  H10X_HIP(c, hipMemcpyAsync(dOff.p, offsets, (size_t)nq * 8, hipMemcpyHostToDevice, c->stream));
  H10X_HIP(c, hipMemsetAsync(dHist.p, 0, (size_t)total * 4, c->stream));
  DevBuf<u32> dDepth; H10X_HIP(c, dDepth.alloc(nq));
  H10X_HIP(c, hipMemcpyAsync(dDepth.p, k.depth.data(), (size_t)nq * 4, hipMemcpyHostToDevice, c->stream));
  k.dHistOff = dOff.p; k.dQDepth = dDepth.p; k.dHist = dHist.p;
  H10X_TRY(k.run(nq));
  H10X_HIP(c, hipMemcpyAsync(hist, dHist.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

__global__ void warm_stageF_kernel() {}
void warm_stageF(hipStream_t st) { warm_stageF_kernel<<<1, 1, 0, st>>>(); }

}  // namespace h10x
