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
//
// The same machinery runs the BARCODE census behind --codeExplore (codeExplore, hash10x.c:1351-1470): for a query barcode
// `code` with good hashes g[0 .. n) (stage_c's goodPos / goodRow, rank order), every entry cj != code of the barcode list of
// rank i gives one key slot << (cbits + 16) | cj << 16 | i. Gather = one wave per (query, rank), the list read through
// goodRow / rows; a run of equal key >> 16 is one barcode cj with countShare[cj] = run length and first[cj] = the head's rank
// (the lowest: the ranks sort along). Windows are ranges of barcode index, found by binary search in each (ascending) list.
// For the one-code clustering of --codeExplore the run pass also writes, per entry, rank << 16 | first[cj]: sorted and
// run-length counted these are minShareCount[first] of every rank i (M[i][j]), from which ce_best_kernel takes msBest /
// msMax / msTot and ce_replay_kernel replays the order-dependent part in one workgroup.
#include "common.hpp"
#include "prim.hpp"
#include "wave.hpp"

namespace h10x {

enum { NB_LIST = 0, NB_MAX = 1, NB_HIST = 2 };
enum { KIND_HASH = 0, KIND_CODE = 1 };                       // census of a hash's neighbours / of a barcode's sharing barcodes
static constexpr u64 NB_DEFAULT_BUDGET = 1ull << 26;       // gathered records per batch: 2 x 8 bytes each for the sort = 1 GiB
static constexpr int CE_RANK_BITS = 16;                      // good ranks of a block (nHash <= 65535: goodHashesBuild, hash10x.c:748)

// barcode census, one wave per query: list entries of its good ranks in the window (size), and its rank count (the gather's units)
__global__ void ce_size_kernel(const u32 *__restrict__ codes, u32 nq, const u32 *__restrict__ nGood, const u64 *__restrict__ blockOff,
                               const u64 *__restrict__ goodRow, const u32 *__restrict__ rows, u32 rowShift, u32 lo, u32 hi, int full,
                               u64 *__restrict__ size, u32 *__restrict__ qUnits) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 q = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (q >= nq) return;
  u32 n; const u64 s = good_list_entries(codes[q], nGood, blockOff, goodRow, rows, rowShift, lo, hi, full != 0, n);
  if (lane == 0) { size[q] = s; qUnits[q] = n; }
}

// one wave per unit (query, good rank of the query); unitBase[q] = first unit of query q, unitBase[nq] = units. Keys
// slot << (cbits + 16) | cj << 16 | rank for the entries cj != code, reserved once per list as nb_gather_kernel does
__global__ __launch_bounds__(256) void ce_gather_kernel(const u32 *__restrict__ codes, u32 nq, const u64 *__restrict__ unitBase,
                                                        const u64 *__restrict__ blockOff, const u64 *__restrict__ goodRow,
                                                        const u32 *__restrict__ rows, u32 rowShift, u32 lo, u32 hi, int full, int sbits,
                                                        u64 cap, u64 *__restrict__ keys, unsigned long long *__restrict__ nKept) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u64 units = unitBase[nq];
  const u64 w0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE, wStride = ((u64)gridDim.x * blockDim.x) / WAVE;
  for (u64 u = w0; u < units; u += wStride) {
    const u32 q = last_le(unitBase, nq, u), code = codes[q], rank = (u32)(u - unitBase[q]);
    u64 a, b; list_window(rows, goodRow[blockOff[code] + rank], rowShift, lo, hi, full != 0, a, b);
    const u64 tag = ((u64)q << sbits) | rank;
    u64 cnt = 0;
    for (u64 e = a; e < b; e += WAVE) {                       // wave-uniform trip counts
      const u64 j = e + lane;
      cnt += __popcll(__ballot(j < b && rows[j] != code));
    }
    if (!cnt) continue;
    unsigned long long p0 = 0;
    if (lane == 0) p0 = atomicAdd(nKept, (unsigned long long)cnt);
    p0 = __shfl(p0, 0);
    for (u64 e = a; e < b; e += WAVE) {
      const u64 j = e + lane;
      u32 cj = 0; bool keep = false;
      if (j < b) { cj = rows[j]; keep = cj != code; }
      const u64 p = wave_place(keep, p0);
      if (keep && p < cap) keys[p] = tag | ((u64)cj << CE_RANK_BITS);   // (p < cap always: cap = entries in the window)
    }
  }
}

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
  s = wave_sum(s);
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
    const u32 q = last_le(unitBase, nq, u), x = xs[q];
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
      const u64 p = wave_place(keep, p0);
      if (keep && p < cap) keys[p] = slot | h;               // p < cap always (cap = records in the window); the test keeps a miscount in bounds
    }
  }
}

// a run of equal keys >> lowBits = one neighbour of one query (lowBits = 0: hash census; 16: barcode census, the ranks below the
// barcode). LIST: head[i] = 1 at a run's first key, cnt[i] = its length, and (pairs != null, --codeExplore) pairs[e] = rank of
// entry e << 16 | rank of its run's head for every entry of the run; MAX: per-query atomics.
template <int MODE>
__global__ void nb_run_kernel(const u64 *__restrict__ keys, u64 n, int hbits, int lowBits, u32 *__restrict__ head, u32 *__restrict__ cnt,
                              unsigned long long *__restrict__ maxKey, u32 *__restrict__ nNb, u64 *__restrict__ pairs) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u64 k = keys[i], id = k >> lowBits;
    if (i && (keys[i - 1] >> lowBits) == id) { if (MODE == NB_LIST) head[i] = 0; continue; }
    u64 j = i + 1; while (j < n && (keys[j] >> lowBits) == id) ++j;
    const u64 c = j - i; const u32 slot = (u32)(k >> hbits), h = (u32)(k & (((u64)1 << hbits) - 1));
    if (MODE == NB_LIST) {
      head[i] = 1; cnt[i] = (u32)c;
      if (pairs) { const u64 lowMask = ((u64)1 << lowBits) - 1, r0 = k & lowMask; for (u64 e = i; e < j; ++e) pairs[e] = ((keys[e] & lowMask) << CE_RANK_BITS) | r0; }
    }
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

// the list rows. Hash census (lowBits = 0): (h, c, lowest barcode of h). Barcode census: (cj, countShare, first rank, the hash
// at that rank: g[first] of the query's block, hash10x.c:1462-1463) and the row's slot
__global__ void nb_emit_kernel(const u64 *__restrict__ keys, u64 n, int hbits, int lowBits, const u32 *__restrict__ head, const u32 *__restrict__ cnt,
                               const u32 *__restrict__ pos, const u64 *__restrict__ rowStart, const u32 *__restrict__ rows,
                               const u32 *__restrict__ codes, const u64 *__restrict__ blockOff, const u16 *__restrict__ goodPos, const h10x_clushash *__restrict__ ch,
                               u32 *__restrict__ oHash, u32 *__restrict__ oCount, u32 *__restrict__ oFirst, u32 *__restrict__ oSlot, u32 *__restrict__ oFirstHash) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (!head[i]) continue;
    const u64 k = keys[i];
    const u32 h = (u32)((k & (((u64)1 << hbits) - 1)) >> lowBits), p = pos[i];
    oHash[p] = h; oCount[p] = cnt[i];
    if (!lowBits) { oFirst[p] = rows[rowStart[h]]; continue; }   // *arr(hashCodes, h, U32*): the lowest barcode of h
    const u32 slot = (u32)(k >> hbits), r = (u32)(k & (((u64)1 << lowBits) - 1));
    const u64 o = blockOff[codes[slot]];
    oFirst[p] = r; oSlot[p] = slot; oFirstHash[p] = ch[o + goodPos[o + r]].hash;
  }
}

// ---- --codeExplore: the one-code clustering from the pairs (rank i << 16 | first[cj]) of every entry, sorted ----
// a run of equal pairs = M[i][j] (minShareCount[j] at rank i, hash10x.c:1376-1382); over j < i: msTot[i] = the sum, best[i] = the
// maximum of M << 16 | (0xFFFF - j) (largest count, then lowest j: the reference's strict > over ascending j). segLo / segHi:
// where rank i's pairs lie (ce_replay_kernel looks M[i][founder] up there)
__global__ void ce_best_kernel(const u64 *__restrict__ pairs, u64 n, unsigned long long *__restrict__ best, u32 *__restrict__ tot,
                               u32 *__restrict__ segLo, u32 *__restrict__ segHi) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const u64 k = pairs[e]; const u32 i = (u32)(k >> CE_RANK_BITS), j = (u32)(k & 0xFFFF);
    if (!e || (u32)(pairs[e - 1] >> CE_RANK_BITS) != i) segLo[i] = (u32)e;
    if (e + 1 == n || (u32)(pairs[e + 1] >> CE_RANK_BITS) != i) segHi[i] = (u32)(e + 1);
    if (e && pairs[e - 1] == k) continue;
    u64 f = e + 1; while (f < n && pairs[f] == k) ++f;
    if (j >= i) continue;                                    // M[i][i]: minShareCount of the rank itself, outside the j < i scan
    const u32 c = (u32)(f - e);
    atomicAdd(&tot[i], c);
    atomicMax(&best[i], ((unsigned long long)c << 16) | (0xFFFFu - j));
  }
}

// hash10x.c:1365-1405 in one workgroup: lane 0 walks the ranks in order (cluster creation, the 256th abandons the block, the fp64
// pointToMin chain), then the workgroup writes every good hash's label (the wipe of hash10x.c:1365 included) into the block's records.
// Dynamic LDS: one label byte per rank. rep: [0] clusters (0 when abandoned), [1] good hashes labelled, [2] abandoned
__global__ __launch_bounds__(256) void ce_replay_kernel(h10x_block *__restrict__ blocks, const u64 *__restrict__ blockOff, h10x_clushash *__restrict__ clusHash,
                                                        const u16 *__restrict__ goodPos, u32 code, u32 n, u32 thr,
                                                        const unsigned long long *__restrict__ best, const u32 *__restrict__ tot,
                                                        const u32 *__restrict__ segLo, const u32 *__restrict__ segHi, const u64 *__restrict__ pairs, u32 *__restrict__ rep) {
  extern __shared__ __align__(16) unsigned char lab[];
  __shared__ u16 founder[256];                               // clusterMin[] (hash10x.c:1400)
  __shared__ u32 sAbandoned;
  for (u32 i = threadIdx.x; i < n; i += blockDim.x) lab[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 nSub = 0, nClustered = 0, abandoned = 0; double p = 0.0;
    for (u32 i = 0; i < n; ++i) {
      const u64 bk = best[i]; const u32 mx = (u32)(bk >> 16);
      if (mx < thr) continue;                                // msMax < clusterThreshold (0: no j < i shares)
      const u32 b = 0xFFFFu - (u32)(bk & 0xFFFF);
      u32 L = lab[b];
      if (!L) {                                              // create a new cluster
        if (++nSub > 255) { abandoned = 1; nSub = 0; nClustered = 0; break; }   // the terms added so far stay in pointToMin
        L = nSub; lab[b] = (u8)L; founder[L] = (u16)b; ++nClustered;
      }
      lab[i] = (u8)L; ++nClustered;
      const u32 f = founder[L];
      u32 q = mx;                                            // minShareCount[clusterMin[label]]: msMax when msBest founded the cluster
      if (f != b) {                                          // else count the pair (i, f) among rank i's pairs
        const u64 key = ((u64)i << CE_RANK_BITS) | f;
        u32 l = segLo[i], r = segHi[i];
        while (l < r) { const u32 m = (l + r) >> 1; if (pairs[m] < key) l = m + 1; else r = m; }
        const u32 s = l; r = segHi[i];
        while (l < r) { const u32 m = (l + r) >> 1; if (pairs[m] <= key) l = m + 1; else r = m; }
        q = l - s;
      }
      p += (double)(int)q / (double)(int)tot[i];
    }
    blocks[code].nSubCluster = nSub; blocks[code].pointToMin = p;
    rep[0] = nSub; rep[1] = nClustered; rep[2] = abandoned;
    sAbandoned = abandoned;
  }
  __syncthreads();
  const bool wipe = sAbandoned != 0;                         // hash10x.c:1394: the labels of ranks < i go back to 0 (the others are 0 already)
  const u64 o = blockOff[code];
  for (u32 i = threadIdx.x; i < n; i += blockDim.x) clusHash[o + goodPos[o + i]].subCluster = wipe ? 0 : lab[i];
}

// --codeExplore's SHARE lines: per listed barcode the CRIB_HTA / CRIB_HTB records of its block (hash10x.c:1459-1461), one wave each
__global__ void ce_crib_kernel(const u32 *__restrict__ codes, u32 n, const u64 *__restrict__ blockOff, const h10x_clushash *__restrict__ ch,
                               const u8 *__restrict__ cribType, u32 *__restrict__ out) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 q = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (q >= n) return;
  const u64 a = blockOff[codes[q]], b = blockOff[codes[q] + 1];
  u32 nA = 0, nB = 0;
  for (u64 e = a + lane; e < b; e += WAVE) { const u32 t = cribType[ch[e].hash]; nA += t == 1; nB += t == 2; }   // CRIB_HTA, CRIB_HTB (stage_d.hip)
  for (int k = 32; k; k >>= 1) { nA += __shfl_xor(nA, k); nB += __shfl_xor(nB, k); }
  if (lane == 0) { out[2 * q] = nA; out[2 * q + 1] = nB; }
}

// ---------------------------------------------------------------------------------------------------------- driver
namespace {
struct Census {
  Ctx *c; int mode; u64 budget;
  int kind = KIND_HASH;                     // KIND_CODE: queries are barcodes, units their good ranks, windows ranges of barcode index
  const u32 *dXs = nullptr;                 // all queries (device)
  std::vector<u64> size; std::vector<u32> depth;   // per query: records in the window, units of the gather (blocks of the hash / good ranks of the barcode)
  // outputs: NB_MAX per query (device, whole call), NB_HIST regions (device), NB_LIST host vectors (+ slot and first hash: KIND_CODE)
  unsigned long long *dMax = nullptr; u32 *dNb = nullptr; const u64 *dHistOff = nullptr; const u32 *dQDepth = nullptr; u32 *dHist = nullptr;
  std::vector<u32> lHash, lCount, lFirst, lSlot, lFirstHash;
  u64 *dPairs = nullptr; u64 nPairs = 0, pairsCap = 0;       // --codeExplore: the (rank, first rank) pair of every kept entry, appended batch by batch
  DevBuf<u64> keys, keys2; DevBuf<u64> unitBase; DevBuf<unsigned long long> nKept; DevBuf<u32> head, cnt, pos, oHash, oCount, oFirst, oSlot, oFirstHash;
  PrimTemp pt;

  u32 top() const { return kind == KIND_CODE ? c->nBlocks : c->hashNumber; }   // the window that covers everything: [0, top)
  int idBits() const { return kind == KIND_CODE ? keyBits(c->nBlocks) + CE_RANK_BITS : keyBits(c->hashNumber); }   // key bits below the slot

  int sizes(const u32 *dX, u32 nq, u32 lo, u32 hi, bool full, u64 *hSize, u32 *hDepth) {
    DevBuf<u64> s; DevBuf<u32> d; hipStream_t st = c->stream;
    H10X_HIP(c, s.alloc(nq)); H10X_HIP(c, d.alloc(nq));
    if (kind == KIND_CODE)
      ce_size_kernel<<<divUp((u64)nq * WAVE, 256), 256, 0, st>>>(dX, nq, c->nGood.p, c->blockOff.p, c->goodRow.p, c->rows.p, (u32)c->rowShift,
                                                                lo, hi, full ? 1 : 0, s.p, d.p);
    else
      nb_size_kernel<<<divUp((u64)nq * WAVE, 256), 256, 0, st>>>(dX, nq, c->hashDepth.p, c->rowStart.p, c->rows.p, c->blockOff.p, c->clusHash.p,
                                                                lo, hi, full ? 1 : 0, s.p, d.p);
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(hSize, s.p, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    if (hDepth) H10X_HIP(c, hipMemcpyAsync(hDepth, d.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  // queries [q0, q0 + nq) of the call in the window [lo, hi); total = records gathered. !full: one window of a query above the budget
  int batch(u32 q0, u32 nq, u32 lo, u32 hi, bool full, u64 total) {
    hipStream_t st = c->stream;
    if (!full) c->nbStats[3] += 1;
    c->nbStats[2] += 1;
    if (!total) return 0;
    std::vector<u64> ub(nq + 1); ub[0] = 0;
    for (u32 q = 0; q < nq; ++q) ub[q + 1] = ub[q] + depth[q0 + q];
    H10X_HIP(c, unitBase.alloc(nq + 1));
    H10X_HIP(c, hipMemcpyAsync(unitBase.p, ub.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    if (keys.n < total) { H10X_HIP(c, keys.alloc(total)); H10X_HIP(c, keys2.alloc(total)); }
    if (!nKept.p) H10X_HIP(c, nKept.alloc(1));
    H10X_HIP(c, hipMemsetAsync(nKept.p, 0, 8, st));
    const int hbits = idBits(), lowBits = kind == KIND_CODE ? CE_RANK_BITS : 0, endBit = hbits + keyBits(nq - 1);
    const unsigned g = (unsigned)hmin<u64>(divUp(ub[nq], 4), 65536);
    if (kind == KIND_CODE)
      ce_gather_kernel<<<g, 256, 0, st>>>(dXs + q0, nq, unitBase.p, c->blockOff.p, c->goodRow.p, c->rows.p, (u32)c->rowShift,
                                          lo, hi, full ? 1 : 0, hbits, total, keys.p, nKept.p);
    else
      nb_gather_kernel<<<g, 256, 0, st>>>(dXs + q0, nq, unitBase.p, c->rowStart.p, c->rows.p, c->blockOff.p, c->clusHash.p, c->within.p,
                                          lo, hi, full ? 1 : 0, hbits, total, keys.p, nKept.p);
    H10X_HIP(c, hipGetLastError());
    unsigned long long n = 0;
    H10X_TRY(c->readback(&n, nKept.p, 8)); H10X_TRY(c->syncReadbacks());
    if (n > total) return c->fail("neighbour census: %llu records kept of %llu gathered", n, (u64)total);
    c->nbStats[0] += total; c->nbStats[1] += n;
    if (!n) return 0;
    if (dPairs && nPairs + n > pairsCap) return c->fail("codeExplore: %llu pairs beyond the %llu entries of the block's lists", (u64)(nPairs + n), (u64)pairsCap);
    H10X_TRY(prim_sort_keys_u64(c, pt, keys.p, keys2.p, n, 0, endBit));
    const unsigned gr = (unsigned)hmin<u64>(divUp(n, 256), 16384);
    if (mode == NB_MAX) {
      nb_run_kernel<NB_MAX><<<gr, 256, 0, st>>>(keys2.p, n, hbits, 0, nullptr, nullptr, dMax + q0, dNb + q0, nullptr);
    } else if (mode == NB_HIST) {
      nb_hist_kernel<<<gr, 256, 0, st>>>(keys2.p, n, hbits, dHistOff + q0, dQDepth + q0, dHist);
    } else {
      H10X_HIP(c, head.alloc(n)); H10X_HIP(c, cnt.alloc(n)); H10X_HIP(c, pos.alloc(n));
      nb_run_kernel<NB_LIST><<<gr, 256, 0, st>>>(keys2.p, n, hbits, lowBits, head.p, cnt.p, nullptr, nullptr, dPairs ? dPairs + nPairs : nullptr);
      if (dPairs) nPairs += n;
      H10X_TRY(prim_exclusive_scan_u32(c, pt, head.p, pos.p, n));
      u32 lastPos = 0, lastHead = 0;
      H10X_HIP(c, hipMemcpyAsync(&lastPos, pos.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(&lastHead, head.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipStreamSynchronize(st));
      const u64 runs = (u64)lastPos + lastHead;
      H10X_HIP(c, oHash.alloc(runs)); H10X_HIP(c, oCount.alloc(runs)); H10X_HIP(c, oFirst.alloc(runs));
      if (kind == KIND_CODE) { H10X_HIP(c, oSlot.alloc(runs)); H10X_HIP(c, oFirstHash.alloc(runs)); }
      nb_emit_kernel<<<gr, 256, 0, st>>>(keys2.p, n, hbits, lowBits, head.p, cnt.p, pos.p, c->rowStart.p, c->rows.p, dXs + q0, c->blockOff.p, c->goodPos.p, c->clusHash.p,
                                         oHash.p, oCount.p, oFirst.p, oSlot.p, oFirstHash.p);
      const size_t at = lHash.size();
      lHash.resize(at + runs); lCount.resize(at + runs); lFirst.resize(at + runs);
      H10X_HIP(c, hipMemcpyAsync(lHash.data() + at, oHash.p, runs * 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(lCount.data() + at, oCount.p, runs * 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(lFirst.data() + at, oFirst.p, runs * 4, hipMemcpyDeviceToHost, st));
      if (kind == KIND_CODE) {
        lSlot.resize(at + runs); lFirstHash.resize(at + runs);
        H10X_HIP(c, hipMemcpyAsync(lSlot.data() + at, oSlot.p, runs * 4, hipMemcpyDeviceToHost, st));
        H10X_HIP(c, hipMemcpyAsync(lFirstHash.data() + at, oFirstHash.p, runs * 4, hipMemcpyDeviceToHost, st));
      }
      H10X_HIP(c, hipGetLastError());
      H10X_HIP(c, hipStreamSynchronize(st));
      for (size_t r = at; r < lSlot.size(); ++r) lSlot[r] += q0;          // (the batch's slots: queries q0 ..)
      return 0;
    }
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  int run(u32 nq) {
    return cut_batches(size.data(), nq, top(), budget,
                       [&](u32 q, u32 lo, u32 hi, u64 *records) { return sizes(dXs + q, 1, lo, hi, false, records, nullptr); },
                       [&](u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 total) { return batch(q0, n, lo, hi, full, total); });
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
  return k.sizes(dX.p, nq, 0, k.top(), true, k.size.data(), k.depth.data());
}

}  // namespace

// the barcode census and what is built on it (--codeExplore, --shareGraph, --shareComponents, --hashCopies): one GPU holding the whole
// data set, good lists that belong to the current blocks, and for the share commands a threshold of at least 1
int ce_check(Ctx *c, const char *cmd, int64_t minShare) {
  if (!c->haveState) return c->fail("no hash state loaded: use readFQB or readHash first");
  if (c->sharded) return c->fail("%s: not available on a sharded context (one rank holds only its own barcodes)", cmd);
  if (!c->haveGood) return c->fail("!! you must set hashDepthRange before %s", cmd);    // hash10x.c:1230 (after --clusterSplit too: the lists are of the old blocks)
  if (minShare < 1) return c->fail("!! %s minShare %lld must be >= 1", cmd, (long long)minShare);
  return 0;
}

int stageF_codeShare(Ctx *c, const u32 *codes, u32 nq, u64 *offsets, u32 *barcode, u32 *count, u32 *firstRank, u32 *firstHash, u64 cap) {
  H10X_TRY(ce_check(c, "codeShare"));
  for (u32 q = 0; q < nq; ++q)
    if (codes[q] >= c->nBlocks) return c->fail("code share census: barcode %u is not below nBlocks %u", codes[q], c->nBlocks);
  if (!nq) { offsets[0] = 0; return 0; }
  Census k; k.c = c; k.mode = NB_LIST; k.kind = KIND_CODE; DevBuf<u32> dX;
  H10X_TRY(nb_begin(c, k, dX, codes, nq));
  H10X_TRY(k.run(nq));
  const size_t rows = k.lHash.size();
  for (u32 q = 0; q <= nq; ++q) offsets[q] = 0;
  for (size_t r = 0; r < rows; ++r) ++offsets[k.lSlot[r] + 1];   // rows come grouped by query (batches and windows in query order), barcodes ascending
  for (u32 q = 0; q < nq; ++q) offsets[q + 1] += offsets[q];
  const size_t m = (size_t)hmin<u64>(cap, rows);
  if (m && barcode) memcpy(barcode, k.lHash.data(), m * 4);
  if (m && count) memcpy(count, k.lCount.data(), m * 4);
  if (m && firstRank) memcpy(firstRank, k.lFirst.data(), m * 4);
  if (m && firstHash) memcpy(firstHash, k.lFirstHash.data(), m * 4);
  return 0;
}

// codeExplore (hash10x.c:1351-1438) up to and including the read merge: census with pairs, M[i][j] -> msBest / msMax / msTot, the
// ordered replay, codeClusterReadMerge's algorithm on [code, code + 1). out: nHash, nGood, clustered, raw, merged, abandoned, histMax, nShare
int stageF_codeExplore(Ctx *c, int code, int threshold, u32 *out) {
  H10X_TRY(ce_check(c, "codeExplore"));
  if (code < 0 || (u32)code >= c->nBlocks) return c->fail("!! codeExplore code %d outside 0 to %u", code, c->nBlocks);
  if (threshold < 1) return c->fail("!! clusterThreshold %d must be >= 1 (the reference reads an uninitialised msBest otherwise)", threshold);
  hipStream_t st = c->stream;
  const u32 x = (u32)code;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  h10x_block blk; u32 n = 0;
  H10X_TRY(c->readback(&blk, c->blocks.p + x, sizeof blk)); H10X_TRY(c->readback(&n, c->nGood.p + x, 4)); H10X_TRY(c->syncReadbacks());
  out[0] = blk.nHash; out[1] = n;
  if (!n) return 0;                                          // hash10x.c:1361: nothing changes, nothing is printed
  Census k; k.c = c; k.mode = NB_LIST; k.kind = KIND_CODE; DevBuf<u32> dX;
  H10X_TRY(nb_begin(c, k, dX, &x, 1));
  DevBuf<u64> pairs, pairs2;
  k.pairsCap = k.size[0];
  if (k.pairsCap >= 0xFFFFFFFFull) return c->fail("codeExplore: barcode %d has %llu list entries, beyond 2^32", code, (u64)k.pairsCap);
  H10X_HIP(c, pairs.alloc(k.pairsCap)); H10X_HIP(c, pairs2.alloc(k.pairsCap));
  k.dPairs = pairs.p;
  H10X_TRY(k.run(1));
  DevBuf<unsigned long long> best; DevBuf<u32> tot, segLo, segHi, rep;
  H10X_HIP(c, best.alloc(n)); H10X_HIP(c, tot.alloc(n)); H10X_HIP(c, segLo.alloc(n)); H10X_HIP(c, segHi.alloc(n)); H10X_HIP(c, rep.alloc(4));
  H10X_HIP(c, hipMemsetAsync(best.p, 0, (size_t)n * 8, st)); H10X_HIP(c, hipMemsetAsync(tot.p, 0, (size_t)n * 4, st));
  H10X_HIP(c, hipMemsetAsync(segLo.p, 0, (size_t)n * 4, st)); H10X_HIP(c, hipMemsetAsync(segHi.p, 0, (size_t)n * 4, st));
  const u64 np = k.nPairs;
  if (np) {
    H10X_TRY(prim_sort_keys_u64(c, k.pt, pairs.p, pairs2.p, np, 0, 2 * CE_RANK_BITS));
    ce_best_kernel<<<(unsigned)hmin<u64>(divUp(np, 256), 16384), 256, 0, st>>>(pairs2.p, np, best.p, tot.p, segLo.p, segHi.p);
  }
  const size_t lds = ((size_t)n + 15) & ~(size_t)15;
  H10X_HIP(c, hipFuncSetAttribute((const void *)ce_replay_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ce_replay_kernel<<<1, 256, lds, st>>>(c->blocks.p, c->blockOff.p, c->clusHash.p, c->goodPos.p, x, n, (u32)threshold, best.p, tot.p, segLo.p, segHi.p, pairs2.p, rep.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(stageC_readMerge(c, x));                          // (returns at once for a block without clusters: hash10x.c:1414)
  u32 r[4];
  H10X_TRY(c->readback(r, rep.p, 12)); H10X_TRY(c->readback(&blk, c->blocks.p + x, sizeof blk)); H10X_TRY(c->syncReadbacks());
  out[2] = r[1]; out[3] = r[0]; out[4] = blk.nSubCluster; out[5] = r[2];
  for (size_t i = 0; i < k.lCount.size(); ++i) out[6] = hmax<u32>(out[6], k.lCount[i]);
  out[7] = (u32)k.lCount.size();
  return 0;
}

// HTA / HTB records of each listed barcode's block (codeExplore's SHARE lines): out[2 q], out[2 q + 1]
int stageF_codeCrib(Ctx *c, const u32 *codes, u32 n, u32 *out) {
  if (!c->haveState) return c->fail("no hash state loaded: use readFQB or readHash first");
  if (c->sharded) return c->fail("code crib counts: not available on a sharded context (one rank holds only its own barcodes)");
  if (!c->haveCrib) return c->fail("!! codeExplore needs --cribBuild for its SHARE lines");
  for (u32 q = 0; q < n; ++q)
    if (codes[q] >= c->nBlocks) return c->fail("code crib counts: barcode %u is not below nBlocks %u", codes[q], c->nBlocks);
  if (!n) return 0;
  DevBuf<u32> dC, dOut;
  H10X_HIP(c, dC.alloc(n)); H10X_HIP(c, dOut.alloc(2 * (size_t)n));
  H10X_HIP(c, hipMemcpyAsync(dC.p, codes, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  ce_crib_kernel<<<divUp((u64)n * WAVE, 256), 256, 0, c->stream>>>(dC.p, n, c->blockOff.p, c->clusHash.p, c->cribType.p, dOut.p);
  H10X_HIP(c, hipGetLastError());
  H10X_HIP(c, hipMemcpyAsync(out, dOut.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

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
