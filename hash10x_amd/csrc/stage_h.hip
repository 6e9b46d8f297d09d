// stage_h.hip — readsets: the object behind moshasm (moshasm.c of the reference) over a mosh set of stage_g.hip.
//
// A readset is a CSR of mosh hits per read: hit[] (set index, top bit = forward), dx[] (u16 distance to the previous hit). The host
// keeps the records and the CSR (they are what -w stores and what the text reports read); the device keeps a copy with, per hit, its
// read and its position (running sum of dx), the inverse CSR (for each mosh the reads that hold it, in read order, once per
// occurrence) and x's map: the hits of every read sorted by mosh, which is where "is this mosh of y a first-occurrence copy-1 hit
// of x, and which" is answered by a binary search in x's own segment — no array as large as the set or the readset per query.
//
// The overlap table. findOverlaps' classification of a pair (x, y) reads the hits of x and y only, so it is done once for every
// directed pair that shares a first-occurrence copy-1 mosh of x, in chunks of queries:
//   expand   every (first-occurrence copy-1 hit of x, entry of that mosh's inverse list) in the order the reference walks them
//   sort     by (x, y), stable: a run is one candidate, its length nHit(x, y), its first element's walk ordinal firstMet(x, y)
//   order    runs sorted by (x, descending nHit, firstMet): the order glibc's stable qsort on nHit leaves (moshasm.c:320)
//   classify one wave per run with nHit >= 3 walks y's hits against x's map: nPlus, nMinus, order violations, and the exact integer
//            sums of z and z * z for both directions; lane 0 keeps the direction that applies
// The table stays on the device (one buffer per chunk); the host keeps 5 bytes per pair (y, isBad, nHit >= 3), which is all the
// in-order flag chain of findOverlaps / markBadReads reads (stage h).
#include "common.hpp"
#include "prim.hpp"
#include "mosh.hpp"
#include <cmath>
#include <memory>
#include <new>

namespace h10x {

constexpr u32 RS_TOP = 0x80000000u, RS_MASK = 0x7fffffffu;
constexpr u32 RS_MAX_HITS = 65534;                           // the reference's u16 map of x's hits (moshasm.c:293) holds j + 1
enum { BAD_REPEAT = 1, BAD_ORDER10 = 2, BAD_ORDER1 = 4, BAD_NOMATCH = 8, BAD_LOWHIT = 16, BAD_LOWCOPY1 = 32 };

struct RsPair {                                              // one candidate of a query, as classified on the device
  u32 iy, nHit, firstMet; int nPlus, nMinus; u8 isPlus, isBad; u16 pad; long long sumZ, sumZ2;
};
struct RsChunk { u32 x0 = 0, x1 = 0; u64 pair0 = 0, nPairs = 0; DevBuf<RsPair> pairs; };

struct ReadSet {
  Mosh *m = nullptr;
  std::vector<h10x_read_t> reads; std::vector<u64> hitStart; std::vector<u32> hit; std::vector<u16> dx;
  u64 totHit = 0; u32 dim = 1u << 16;
  // device copy + index (rsIndex)
  bool indexed = false;
  DevBuf<u32> dHit, dHitStart, dHitRead, dPos, dInv, dInvStart, dMapMosh, dMapJ; DevBuf<u8> dFirst;
  std::vector<u32> nRepeat;
  // overlap table (rsTable)
  bool tabled = false;
  std::vector<std::unique_ptr<RsChunk>> chunks;
  std::vector<u64> pairStart; std::vector<u32> cY; std::vector<u8> cBits;      // compact host copy: bit 0 isBad, bit 1 nHit >= 3
};

// ------------------------------------------------------------------------------------------------ kernels: build
// The walk of seq_scan.hpp over the plan's runs (uniform trip counts, as in mosh_scan_kernel of stage_g.hip: wave_append sees all 64 lanes). A mosh found in the
// table goes to the list as (ordinal of its k-mer in the batch, index | forward bit) and counts in acc[]; one that is not counts in nMiss of its sequence.
__global__ __launch_bounds__(256)
void rs_scan_kernel(const u8 *__restrict__ codes, const u64 *__restrict__ seqStart, const u64 *__restrict__ runStart, u32 nSeq, int k, int w, u64 factor1,
                    const u32 *__restrict__ table, const u64 *__restrict__ value, int B, u32 *__restrict__ acc, u32 *__restrict__ nMiss,
                    u32 *__restrict__ outOrd, u32 *__restrict__ outHit, u64 cap, u64 *__restrict__ listed) {
  const u64 nRuns = runStart[nSeq];
  const u64 T = (u64)gridDim.x * blockDim.x, iters = (nRuns + T - 1) / T;
  for (u64 it = 0; it < iters; ++it) {
    const u64 run = it * T + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    KmerRun r = {0, 0, 0, 0, codes}; KmerRoll roll(k, factor1); u32 miss = 0;
    if (run < nRuns) { r = KmerRun::open(codes, seqStart, runStart, nSeq, run, k, SeqSkip{0, 0}); roll.prime(r.b); }
    for (int j = 0; j < SEQ_RUN; ++j) {
      bool emit = false; u32 hv = 0;
      if (j < r.cnt) {
        const u64 h = roll.next(r.b[k - 1 + j]);
        if (h % (u64)w == 0) {
          const u32 ix = probe_find(table, value, B, h);
          if (ix) { atomicAdd(&acc[ix], 1u); hv = roll.fwd() ? (ix | RS_TOP) : ix; emit = true; }
          else ++miss;
        }
      }
      const u64 at = wave_append(emit, listed);
      if (emit && at < cap) { outOrd[at] = (u32)(r.ord0 + (u64)j); outHit[at] = hv; }
    }
    if (miss) atomicAdd(&nMiss[r.s], miss);
  }
}
// hits sorted by ordinal: dx = distance to the previous hit of the same sequence, the position itself for the first (moshasm.c:146)
__global__ void rs_dx_kernel(const u32 *__restrict__ ord, u64 n, const u64 *__restrict__ seqStart, u32 nSeq, u16 *__restrict__ dx, u32 *__restrict__ nHit) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 o = ord[i];
  const u32 s = last_le(seqStart, nSeq, o);                  // (an empty sequence never wins: the next one starts there too)
  const u64 s0 = seqStart[s];
  const u64 prev = (i > 0 && (u64)ord[i - 1] >= s0) ? (u64)ord[i - 1] - s0 : 0;
  dx[i] = (u16)(o - s0 - prev);
  atomicAdd(&nHit[s], 1u);
}

// ------------------------------------------------------------------------------------------------ kernels: index
// per read: position and read of every hit, nCopy[4] (moshasm.c:246-250)
__global__ void rs_read_kernel(const u32 *__restrict__ hitStart, u32 nReads, const u32 *__restrict__ hit, const u16 *__restrict__ dx, const u8 *__restrict__ info,
                               u32 *__restrict__ pos, u32 *__restrict__ hitRead, u32 *__restrict__ nCopy) {
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nReads) return;
  u32 p = 0, c[4] = {0, 0, 0, 0};
  for (u32 i = hitStart[r]; i < hitStart[r + 1]; ++i) {
    p += dx[i]; pos[i] = p; hitRead[i] = r;
    const u32 cc = info[hit[i] & RS_MASK] & 3;
    c[0] += cc == 0; c[1] += cc == 1; c[2] += cc == 2; c[3] += cc == 3;
  }
  for (int j = 0; j < 4; ++j) nCopy[(size_t)r * 4 + j] = c[j];
}
__global__ void rs_keys_kernel(const u32 *__restrict__ hit, const u32 *__restrict__ hitRead, const u32 *__restrict__ hitStart, const u16 *__restrict__ depth, u32 n,
                               u32 *__restrict__ invKey, u64 *__restrict__ mapKey, u32 *__restrict__ mapJ) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 y = hit[i] & RS_MASK, r = hitRead[i];
  invKey[i] = depth[y] < 65535 ? y : 0xFFFFFFFFu;            // moshasm.c:251: a saturated mosh has no inverse list
  mapKey[i] = ((u64)r << 32) | y; mapJ[i] = i - hitStart[r] + 1;
}
__global__ void rs_eff_kernel(const u16 *__restrict__ depth, u32 n1, u32 *__restrict__ eff) {  // n1 + 1 entries: the scan's last one is the total
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n1) return;
  const u32 d = (i > 0 && i < n1) ? depth[i] : 0;
  eff[i] = d < 65535 ? d : 0;
}
// the sorted occurrences fill exactly the lists that depth[] sizes: otherwise the set's depths are not this readset's
__global__ void rs_invcheck_kernel(const u32 *__restrict__ key, u32 n, const u32 *__restrict__ invStart, u32 n1, u32 *__restrict__ flag) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 y = key[i];
  const bool ok = y == 0xFFFFFFFFu ? i >= invStart[n1] : (y > 0 && y < n1 && invStart[y] <= i && i < invStart[y + 1]);
  if (!ok) *flag = 1;
}
// x's map sorted by (read, mosh), equal moshes in hit order: the first of a run is the first occurrence (moshasm.c:302)
__global__ void rs_first_kernel(const u64 *__restrict__ mapKey, const u32 *__restrict__ mapJ, const u32 *__restrict__ hitStart, const u8 *__restrict__ info, u32 n,
                                u32 *__restrict__ mapMosh, u8 *__restrict__ first, u32 *__restrict__ nRepeat) {
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const u64 key = mapKey[p];
  const u32 r = (u32)(key >> 32), y = (u32)key;
  mapMosh[p] = y;
  if ((info[y] & 3) != 1) return;
  if (p == hitStart[r] || mapKey[p - 1] != key) first[hitStart[r] + mapJ[p] - 1] = 1;
  else atomicAdd(&nRepeat[r], 1u);
}

// ------------------------------------------------------------------------------------------------ kernels: overlap table
__global__ void rs_weight_kernel(const u8 *__restrict__ first, const u32 *__restrict__ hit, const u16 *__restrict__ depth, u32 n, u32 *__restrict__ w, u32 *__restrict__ saturated) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;                                         // n + 1 entries: the scan's last one is the total
  u32 d = 0;
  if (i < n && first[i]) { d = depth[hit[i] & RS_MASK]; if (d == 65535) { atomicMin(saturated, hit[i] & RS_MASK); d = 0; } }
  w[i] = d;
}
__global__ void rs_gather_kernel(const u64 *__restrict__ off, const u32 *__restrict__ hitStart, u32 nReads1, u64 *__restrict__ out) {
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nReads1) out[r] = off[hitStart[r]];
}
// entry e of the chunk = element (g - off[p]) of the inverse list of hit p, p = the hit whose span of the scan holds g = base + e
__global__ void rs_expand_kernel(u64 base, u32 E, const u64 *__restrict__ off, u32 h0, u32 h1, const u32 *__restrict__ hit, const u32 *__restrict__ hitRead,
                                 const u32 *__restrict__ invStart, const u32 *__restrict__ inv, u32 x0, int yBits, u64 *__restrict__ key, u32 *__restrict__ val) {
  const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const u64 g = base + e;
  u32 lo = h0, hi = h1;                                      // largest p in [h0, h1) with off[p] <= g: hits of no weight share their successor's offset and lose
  while (hi - lo > 1) { const u32 mid = lo + (hi - lo) / 2; if (off[mid] <= g) lo = mid; else hi = mid; }
  const u32 y = inv[invStart[hit[lo] & RS_MASK] + (u32)(g - off[lo])];
  key[e] = ((u64)(hitRead[lo] - x0) << yBits) | y; val[e] = e;
}
__global__ void rs_heads_kernel(const u64 *__restrict__ key, u32 n, u32 *__restrict__ flag) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
__global__ void rs_runs_kernel(const u64 *__restrict__ key, const u32 *__restrict__ val, const u32 *__restrict__ flag, const u32 *__restrict__ before, u32 n,
                               u32 *__restrict__ runStart, u32 *__restrict__ runFirst) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  runStart[before[i]] = i; runFirst[before[i]] = val[i];     // the sort is stable: the first element of a run is the first met
}
__global__ void rs_order_kernel(const u64 *__restrict__ key, const u32 *__restrict__ runStart, const u32 *__restrict__ runFirst, u32 nRuns, u32 E, int yBits, u32 x0,
                                u64 *__restrict__ okey, u32 *__restrict__ oval, u32 *__restrict__ pairCount) {
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nRuns) return;
  const u32 nHit = (r + 1 < nRuns ? runStart[r + 1] : E) - runStart[r];
  const u32 xl = (u32)(key[runStart[r]] >> yBits);
  okey[r] = ((u64)xl << 48) | ((u64)(65535u - (nHit > 65535u ? 65535u : nHit)) << 32) | runFirst[r]; oval[r] = r;
  atomicAdd(&pairCount[x0 + xl], 1u);
}
// One wave per candidate in its final place s. The walk of y's hits against x's map (moshasm.c:330-353) in tiles of 64: a lane looks
// its hit up in x's segment of the map; "last" of a matched lane is the map index of the nearest matched lane below it, or the last
// match of the tiles before. Both directions are summed, since which applies is known only at the end.
__global__ __launch_bounds__(256)
void rs_classify_kernel(u32 nRuns, const u32 *__restrict__ perm, const u64 *__restrict__ key, const u32 *__restrict__ runStart, const u32 *__restrict__ runFirst, u32 E,
                        int yBits, u32 x0, const u32 *__restrict__ hitStart, const u32 *__restrict__ hit, const u32 *__restrict__ pos,
                        const u32 *__restrict__ mapMosh, const u32 *__restrict__ mapJ, const u8 *__restrict__ info,
                        RsPair *__restrict__ out, u32 *__restrict__ cY, u8 *__restrict__ cBits) {
  const u32 s = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (s >= nRuns) return;                                    // (a whole wave leaves together)
  const u32 r = perm[s];
  const u64 kk = key[runStart[r]];
  const u32 x = x0 + (u32)(kk >> yBits), y = (u32)(kk & (((u64)1 << yBits) - 1));
  const u32 nHit = (r + 1 < nRuns ? runStart[r + 1] : E) - runStart[r];
  RsPair P; P.iy = y; P.nHit = nHit; P.firstMet = runFirst[r]; P.nPlus = P.nMinus = 0; P.isPlus = P.isBad = 0; P.pad = 0; P.sumZ = P.sumZ2 = 0;
  if (nHit >= 3) {
    const u32 xs = hitStart[x], xe = hitStart[x + 1], ys = hitStart[y], ye = hitStart[y + 1];
    u32 nP = 0, nM = 0, vP = 0, vM = 0, carry = 0; bool haveCarry = false;
    long long sP = 0, sP2 = 0, sM = 0, sM2 = 0;
    for (u32 base = ys; base < ye; base += WAVE) {
      const u32 i = base + lane;
      bool matched = false; u32 ihx = 0, h = 0;
      if (i < ye) {
        h = hit[i];
        const u32 mo = h & RS_MASK;
        if ((info[mo] & 3) == 1) {
          u32 lo = xs, hi = xe;                              // first entry of x's map that is not below mo
          while (lo < hi) { const u32 mid = lo + (hi - lo) / 2; if (mapMosh[mid] < mo) lo = mid + 1; else hi = mid; }
          if (lo < xe && mapMosh[lo] == mo) { ihx = mapJ[lo]; matched = true; }
        }
      }
      const u64 mm = __ballot(matched);
      const u64 below = mm & (((u64)1 << lane) - 1);
      const u32 prevIn = __shfl(ihx, below ? 63 - __clzll((long long)below) : lane);
      if (matched) {
        const bool hasPrev = below || haveCarry;
        const u32 prev = below ? prevIn : carry;
        if (((h ^ hit[xs + ihx - 1]) & RS_TOP) == 0) ++nP; else ++nM;
        if (ihx < (hasPrev ? prev : 0u)) ++vP;               // moshasm.c:341
        if (ihx > (hasPrev ? prev : xe - xs)) ++vM;          // moshasm.c:350
        const long long xp = pos[xs + ihx - 1], yp = pos[i], zp = xp - yp, zm = xp + yp;
        sP += zp; sP2 += zp * zp; sM += zm; sM2 += zm * zm;
      }
      if (mm) { carry = __shfl(ihx, 63 - __clzll((long long)mm)); haveCarry = true; }
    }
    for (int o = 32; o; o >>= 1) {
      nP += __shfl_down(nP, o); nM += __shfl_down(nM, o); vP += __shfl_down(vP, o); vM += __shfl_down(vM, o);
      sP += __shfl_down(sP, o); sP2 += __shfl_down(sP2, o); sM += __shfl_down(sM, o); sM2 += __shfl_down(sM2, o);
    }
    if (nP && !nM) { P.isPlus = 1; P.isBad = vP > 0; P.nPlus = (int)(nP - vP); P.sumZ = sP; P.sumZ2 = sP2; }
    else if (nM && !nP) { P.isBad = vM > 0; P.nMinus = (int)(nM - vM); P.sumZ = sM; P.sumZ2 = sM2; }
    else { P.nPlus = (int)nP; P.nMinus = (int)nM; P.isBad = (nP && nM) ? 1 : 0; }           // moshasm.c:354: mixed is bad, both sums 0
  }
  if (lane == 0) { out[s] = P; cY[s] = y; cBits[s] = (u8)(P.isBad | (nHit >= 3 ? 2 : 0)); }
}

// ------------------------------------------------------------------------------------------------ drivers

static void rsInvalidate(ReadSet *rs) {
  rs->indexed = rs->tabled = false; rs->chunks.clear(); rs->pairStart.clear(); rs->cY.clear(); rs->cBits.clear(); rs->nRepeat.clear();
}

int stageH_create(ReadSet **out, Mosh *m) {
  *out = nullptr;
  if (!m) return -1;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c;
  if (m->max >= RS_TOP) return c->fail("too many entries in moshset");                        // moshasm.c:652
  ReadSet *rs = new (std::nothrow) ReadSet();
  if (!rs) return c->fail("out of host memory");
  rs->m = m;
  rs->reads.resize(1); memset(&rs->reads[0], 0, sizeof(h10x_read_t)); rs->hitStart.assign(2, 0);
  H10X_HIP(c, hipMemsetAsync(m->depth.p, 0, (size_t)m->size * 2, c->stream));                 // moshasm.c:132
  H10X_HIP(c, hipMemsetAsync(m->acc.p, 0, (size_t)m->size * 4, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  *out = rs;
  return 0;
}
void stageH_destroy(ReadSet *rs) {
  if (!rs) return;
  (void)moshEnter(rs->m);
  (void)hipStreamSynchronize(rs->m->c.stream);
  delete rs;
}
const char *stageH_error(const ReadSet *rs) { return rs ? rs->m->c.err.c_str() : "null readset"; }
// a std::bad_alloc of the host vectors, caught at the C boundary (h10x_api.hip)
int stageH_oom(Mosh *m) { return m ? m->c.fail("out of host memory") : -1; }
Mosh *stageH_set(ReadSet *rs) { return rs ? rs->m : nullptr; }

static u32 rsGrowDim(u32 dim, u32 n) {                       // arrayExtend (array.c:144-170) for 72-byte records, called with index n >= dim
  if ((u64)dim * 72 < ((u64)1 << 23)) dim *= 2; else dim += 1024 + ((1u << 23) / 72);
  if (n >= dim) dim = n + 1;
  return dim;
}

static int rsAddBatch(ReadSet *rs, const u8 *codes, const u64 *seqStart, u32 nSeq) {
  Mosh *m = rs->m; Ctx *c = &m->c; hipStream_t st = c->stream; const int k = m->k; PrimTemp pt;
  const SeqPlan plan(seqStart, nSeq, k); StreamWait wait{st};
  for (u32 s = 0; s < nSeq; ++s) if (plan.len(s) >= ((u64)1 << 31)) return c->fail("sequence of %llu bases: 2^31 or more are not supported", (unsigned long long)plan.len(s));
  if (plan.total > 0xFFFFFFFFull) return c->fail("a batch of %llu bases: at most 2^32 - 1 are supported per call", plan.total);
  std::vector<u32> nHit(nSeq, 0), nMiss(nSeq, 0); std::vector<u32> hh; std::vector<u16> dd;
  u64 n = 0;
  if (plan.nRuns) {
    SeqBatch b; DevBuf<u64> dListed; DevBuf<u32> dMiss, dNHit, oOrd, oHit, sOrd, sHit; DevBuf<u16> dDx;
    H10X_TRY(b.upload(c, plan, codes + seqStart[0])); H10X_HIP(c, dListed.alloc(1)); H10X_HIP(c, dMiss.alloc(nSeq)); H10X_HIP(c, dNHit.alloc(nSeq));
    const unsigned grid = (unsigned)hmin<u64>(divUp(plan.nRuns, 256), (u64)c->numCU * 16);
    H10X_TRY(seqScanTwice(c, plan.cap(m->w), dListed.p, &n, 1, "readset scan: the list overflowed twice", [&](u64 cap) -> int {
      H10X_HIP(c, oOrd.alloc(cap)); H10X_HIP(c, oHit.alloc(cap));
      H10X_HIP(c, hipMemsetAsync(dListed.p, 0, 8, st)); H10X_HIP(c, hipMemsetAsync(dMiss.p, 0, (size_t)nSeq * 4, st));
      rs_scan_kernel<<<grid, 256, 0, st>>>(b.codes.p, b.seq.p, b.run.p, nSeq, k, m->w, m->factor1, c->hashIndex.p, c->hashValue.p, m->B, m->acc.p, dMiss.p,
                                           oOrd.p, oHit.p, cap, dListed.p);
      return 0;
    }, [&]() -> int { H10X_HIP(c, hipMemsetAsync(m->acc.p, 0, (size_t)m->size * 4, st)); return 0; }));   // (acc[] is all zero between batches)
    H10X_HIP(c, hipMemcpyAsync(nMiss.data(), dMiss.p, (size_t)nSeq * 4, hipMemcpyDeviceToHost, st));
    if (n) {
      H10X_HIP(c, sOrd.alloc(n)); H10X_HIP(c, sHit.alloc(n)); H10X_HIP(c, dDx.alloc(n));
      H10X_TRY(prim_sort_pairs_u32_u32(c, pt, oOrd.p, sOrd.p, oHit.p, sHit.p, n, 0, bitsFor(plan.total)));
      H10X_HIP(c, hipMemsetAsync(dNHit.p, 0, (size_t)nSeq * 4, st));
      rs_dx_kernel<<<divUp(n, 256), 256, 0, st>>>(sOrd.p, n, b.seq.p, nSeq, dDx.p, dNHit.p);
      H10X_HIP(c, hipGetLastError());
      hh.resize(n); dd.resize(n);
      H10X_HIP(c, hipMemcpyAsync(hh.data(), sHit.p, n * 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(dd.data(), dDx.p, n * 2, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(nHit.data(), dNHit.p, (size_t)nSeq * 4, hipMemcpyDeviceToHost, st));
    }
    H10X_HIP(c, hipStreamSynchronize(st));
  }
  for (u32 s = 0; s < nSeq; ++s)
    if (nHit[s] > RS_MAX_HITS) return c->fail("read %llu has %u hits: more than %u are not supported", (unsigned long long)(rs->reads.size() + s), nHit[s], RS_MAX_HITS);
  if (rs->totHit + n >= RS_TOP) return c->fail("readset of %llu hits: 2^31 or more are not supported", (unsigned long long)(rs->totHit + n));
  if ((u64)rs->reads.size() + nSeq >= RS_TOP) return c->fail("readset of 2^31 reads or more is not supported");
  if (n) {                                                   // only a batch that is taken counts in the set's depths (a refused one leaves acc[] to the caller's reset)
    H10X_TRY(moshFold(m));
    H10X_HIP(c, hipStreamSynchronize(st));
  }
  for (u32 s = 0; s < nSeq; ++s) {
    h10x_read_t r; memset(&r, 0, sizeof r);
    r.len = (int32_t)plan.len(s); r.nHit = (int32_t)nHit[s]; r.nMiss = (int32_t)nMiss[s];
    const u32 ix = (u32)rs->reads.size();
    if (ix >= rs->dim) rs->dim = rsGrowDim(rs->dim, ix);
    rs->reads.push_back(r);
    rs->hitStart.push_back(rs->hitStart.back() + nHit[s]);
  }
  rs->hit.insert(rs->hit.end(), hh.begin(), hh.end()); rs->dx.insert(rs->dx.end(), dd.begin(), dd.end());
  rs->totHit += n;
  return 0;
}

int stageH_add(ReadSet *rs, const u8 *codes, const u64 *seqStart, u32 nSeq) {
  Mosh *m = rs->m;
  H10X_TRY(moshEnter(m));
  if (nSeq && (!codes || !seqStart)) return m->c.fail("h10x_readset_add: null argument");
  rsInvalidate(rs);
  const int rc = moshBatches(m, seqStart, nSeq, [&](u32 s, u32 n) { return rsAddBatch(rs, codes, seqStart + s, n); });
  if (rc) { (void)hipStreamSynchronize(m->c.stream); (void)hipMemsetAsync(m->acc.p, 0, (size_t)m->size * 4, m->c.stream); (void)hipStreamSynchronize(m->c.stream); }
  return rc;
}

int stageH_load(ReadSet **out, Mosh *m, const h10x_read_t *reads, u32 nReads, u32 dim, const u32 *hit, const u16 *dx) {
  *out = nullptr;
  if (!m) return -1;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c;
  if (m->max >= RS_TOP) return c->fail("too many entries in moshset");
  if (!reads || nReads < 1 || nReads > dim) return c->fail("readset max %u outside 1 .. dim %u", nReads, dim);
  u64 tot = 0;
  for (u32 i = 0; i < nReads; ++i) {
    if (reads[i].nHit < 0 || (u32)reads[i].nHit > RS_MAX_HITS) return c->fail("read %u has %d hits: more than %u are not supported", i, reads[i].nHit, RS_MAX_HITS);
    tot += (u32)reads[i].nHit;
  }
  if (tot >= RS_TOP) return c->fail("readset of %llu hits: 2^31 or more are not supported", (unsigned long long)tot);
  if (tot && (!hit || !dx)) return c->fail("h10x_readset_load: null argument");
  std::unique_ptr<ReadSet> rs(new (std::nothrow) ReadSet());
  if (!rs) return c->fail("out of host memory");
  rs->m = m; rs->dim = dim; rs->totHit = tot;
  rs->reads.assign(reads, reads + nReads);
  rs->hitStart.assign((size_t)nReads + 1, 0);
  for (u32 i = 0; i < nReads; ++i) { rs->hitStart[i + 1] = rs->hitStart[i] + (u32)reads[i].nHit; rs->reads[i].hitPtr = rs->reads[i].dxPtr = 0; }
  rs->hit.assign(hit, hit + tot); rs->dx.assign(dx, dx + tot);
  for (u32 i = 0; i < nReads; ++i)
    for (u64 p = rs->hitStart[i]; p < rs->hitStart[i + 1]; ++p) {
      const u32 y = rs->hit[p] & RS_MASK;
      if (y == 0 || y > m->max) return c->fail("read %u holds mosh index %u outside 1 .. %u", i, y, m->max);
    }
  *out = rs.release();
  return 0;
}

// the device copy, nCopy, the inverse CSR and x's map (invBuild, moshasm.c:232-260)
static int rsIndex(ReadSet *rs) {
  if (rs->indexed) return 0;
  Mosh *m = rs->m; Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt;
  const u32 R = (u32)rs->reads.size(), n = (u32)rs->totHit, n1 = m->max + 1;
  std::vector<u32> hs((size_t)R + 1);
  for (u32 i = 0; i <= R; ++i) hs[i] = (u32)rs->hitStart[i];
  DevBuf<u16> dDx; DevBuf<u32> dCopy, invKey, invKeyS, eff, flag; DevBuf<u64> mapKey, mapKeyS; DevBuf<u32> mapJ;
  H10X_HIP(c, rs->dHitStart.alloc((size_t)R + 1)); H10X_HIP(c, rs->dHit.alloc(n)); H10X_HIP(c, dDx.alloc(n)); H10X_HIP(c, rs->dHitRead.alloc(n)); H10X_HIP(c, rs->dPos.alloc(n));
  H10X_HIP(c, dCopy.alloc((size_t)R * 4)); H10X_HIP(c, rs->dInv.alloc(n)); H10X_HIP(c, rs->dInvStart.alloc((size_t)n1 + 1)); H10X_HIP(c, eff.alloc((size_t)n1 + 1));
  H10X_HIP(c, rs->dMapMosh.alloc(n)); H10X_HIP(c, rs->dMapJ.alloc(n)); H10X_HIP(c, rs->dFirst.alloc(n)); H10X_HIP(c, flag.alloc((size_t)R + 1));
  H10X_HIP(c, hipMemcpyAsync(rs->dHitStart.p, hs.data(), ((size_t)R + 1) * 4, hipMemcpyHostToDevice, st));
  if (n) {
    H10X_HIP(c, hipMemcpyAsync(rs->dHit.p, rs->hit.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    H10X_HIP(c, hipMemcpyAsync(dDx.p, rs->dx.data(), (size_t)n * 2, hipMemcpyHostToDevice, st));
  }
  rs_read_kernel<<<divUp(R, 256), 256, 0, st>>>(rs->dHitStart.p, R, rs->dHit.p, dDx.p, m->info.p, rs->dPos.p, rs->dHitRead.p, dCopy.p);
  H10X_HIP(c, hipGetLastError());
  std::vector<u32> copy((size_t)R * 4);
  H10X_HIP(c, hipMemcpyAsync(copy.data(), dCopy.p, (size_t)R * 16, hipMemcpyDeviceToHost, st));
  rs_eff_kernel<<<divUp((u64)n1 + 1, 256), 256, 0, st>>>(m->depth.p, n1, eff.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, eff.p, rs->dInvStart.p, (size_t)n1 + 1));
  H10X_HIP(c, hipMemsetAsync(flag.p, 0, ((size_t)R + 1) * 4, st));          // flag[0] = mismatch, flag[1 + r] = nRepeat of read r ... (R entries used)
  rs->nRepeat.assign(R, 0);
  u32 mismatch = 0;
  if (n) {
    H10X_HIP(c, invKey.alloc(n)); H10X_HIP(c, invKeyS.alloc(n)); H10X_HIP(c, mapKey.alloc(n)); H10X_HIP(c, mapKeyS.alloc(n)); H10X_HIP(c, mapJ.alloc(n));
    rs_keys_kernel<<<divUp(n, 256), 256, 0, st>>>(rs->dHit.p, rs->dHitRead.p, rs->dHitStart.p, m->depth.p, n, invKey.p, mapKey.p, mapJ.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_sort_pairs_u32_u32(c, pt, invKey.p, invKeyS.p, rs->dHitRead.p, rs->dInv.p, n, 0, 32));
    rs_invcheck_kernel<<<divUp(n, 256), 256, 0, st>>>(invKeyS.p, n, rs->dInvStart.p, n1, flag.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_sort_pairs_u64_u32(c, pt, mapKey.p, mapKeyS.p, mapJ.p, rs->dMapJ.p, n, 0, 32 + bitsFor(R)));
    H10X_HIP(c, hipMemsetAsync(rs->dFirst.p, 0, n, st));
    rs_first_kernel<<<divUp(n, 256), 256, 0, st>>>(mapKeyS.p, rs->dMapJ.p, rs->dHitStart.p, m->info.p, n, rs->dMapMosh.p, rs->dFirst.p, flag.p + 1);
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(&mismatch, flag.p, 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipMemcpyAsync(rs->nRepeat.data(), flag.p + 1, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  }
  u32 invTotal = 0;
  H10X_HIP(c, hipMemcpyAsync(&invTotal, rs->dInvStart.p + n1, 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  if (mismatch || invTotal > n) return c->fail("the readset does not match the depths of its mosh set");
  for (u32 i = 1; i < R; ++i) for (int j = 0; j < 4; ++j) rs->reads[i].nCopy[j] = (int32_t)copy[(size_t)i * 4 + j];
  rs->indexed = true;
  return 0;
}

static int rsTable(ReadSet *rs) {
  if (rs->tabled) return 0;
  H10X_TRY(rsIndex(rs));
  Mosh *m = rs->m; Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt;
  const u32 R = (u32)rs->reads.size(), n = (u32)rs->totHit;
  rs->chunks.clear(); rs->cY.clear(); rs->cBits.clear(); rs->pairStart.assign((size_t)R + 1, 0);
  DevBuf<u32> w, sat, pairCount; DevBuf<u64> off, offRead;
  H10X_HIP(c, w.alloc((size_t)n + 1)); H10X_HIP(c, off.alloc((size_t)n + 1)); H10X_HIP(c, offRead.alloc((size_t)R + 1)); H10X_HIP(c, sat.alloc(1)); H10X_HIP(c, pairCount.alloc(R));
  H10X_HIP(c, hipMemsetAsync(sat.p, 0xFF, 4, st)); H10X_HIP(c, hipMemsetAsync(pairCount.p, 0, (size_t)R * 4, st));
  rs_weight_kernel<<<divUp((u64)n + 1, 256), 256, 0, st>>>(rs->dFirst.p, rs->dHit.p, m->depth.p, n, w.p, sat.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, w.p, off.p, (size_t)n + 1));
  rs_gather_kernel<<<divUp((u64)R + 1, 256), 256, 0, st>>>(off.p, rs->dHitStart.p, R + 1, offRead.p);
  H10X_HIP(c, hipGetLastError());
  std::vector<u64> offR((size_t)R + 1); u32 satMosh = 0;
  H10X_HIP(c, hipMemcpyAsync(offR.data(), offRead.p, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(&satMosh, sat.p, 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  if (satMosh != 0xFFFFFFFFu) {
    u64 v = 0; H10X_HIP(c, hipMemcpy(&v, c->hashValue.p + satMosh, 8, hipMemcpyDeviceToHost));
    return c->fail("copy-1 mosh %llx has depth 65535: it has no inverse list", (unsigned long long)v);
  }
  const int yBits = bitsFor(R);
  const u64 chunkEntries = m->overlapChunk; const u32 chunkReads = m->overlapChunkReads;      // (at most RS_CHUNK_READS_MAX: stageG_setOption)
  u64 pairBase = 0;
  for (u32 x0 = 0; x0 < R; ) {
    u32 x1 = x0 + 1;
    while (x1 < R && x1 - x0 < chunkReads && offR[x1 + 1] - offR[x0] <= chunkEntries) ++x1;
    const u64 E64 = offR[x1] - offR[x0];
    if (E64 >= RS_TOP) return c->fail("read %u meets %llu inverse-list entries: 2^31 or more are not supported", x0, (unsigned long long)E64);
    const u32 E = (u32)E64;
    if (E) {
      DevBuf<u64> key, keyS, okey, okeyS; DevBuf<u32> val, valS, flag, before, runStart, runFirst, oval, perm, dY; DevBuf<u8> dBits;
      H10X_HIP(c, key.alloc(E)); H10X_HIP(c, keyS.alloc(E)); H10X_HIP(c, val.alloc(E)); H10X_HIP(c, valS.alloc(E)); H10X_HIP(c, flag.alloc(E)); H10X_HIP(c, before.alloc(E));
      rs_expand_kernel<<<divUp(E, 256), 256, 0, st>>>(offR[x0], E, off.p, (u32)rs->hitStart[x0], (u32)rs->hitStart[x1], rs->dHit.p, rs->dHitRead.p, rs->dInvStart.p, rs->dInv.p,
                                                      x0, yBits, key.p, val.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_sort_pairs_u64_u32(c, pt, key.p, keyS.p, val.p, valS.p, E, 0, yBits + bitsFor(x1 - x0 - 1)));
      rs_heads_kernel<<<divUp(E, 256), 256, 0, st>>>(keyS.p, E, flag.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, before.p, E));
      u32 tail[2];
      H10X_HIP(c, hipMemcpyAsync(&tail[0], before.p + (E - 1), 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(&tail[1], flag.p + (E - 1), 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipStreamSynchronize(st));
      const u32 nRuns = tail[0] + tail[1];
      std::unique_ptr<RsChunk> ch(new RsChunk());
      ch->x0 = x0; ch->x1 = x1; ch->pair0 = pairBase; ch->nPairs = nRuns;
      H10X_HIP(c, runStart.alloc(nRuns)); H10X_HIP(c, runFirst.alloc(nRuns)); H10X_HIP(c, okey.alloc(nRuns)); H10X_HIP(c, okeyS.alloc(nRuns)); H10X_HIP(c, oval.alloc(nRuns));
      H10X_HIP(c, perm.alloc(nRuns)); H10X_HIP(c, dY.alloc(nRuns)); H10X_HIP(c, dBits.alloc(nRuns)); H10X_HIP(c, ch->pairs.alloc(nRuns));
      rs_runs_kernel<<<divUp(E, 256), 256, 0, st>>>(keyS.p, valS.p, flag.p, before.p, E, runStart.p, runFirst.p);
      H10X_HIP(c, hipGetLastError());
      rs_order_kernel<<<divUp(nRuns, 256), 256, 0, st>>>(keyS.p, runStart.p, runFirst.p, nRuns, E, yBits, x0, okey.p, oval.p, pairCount.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_sort_pairs_u64_u32(c, pt, okey.p, okeyS.p, oval.p, perm.p, nRuns, 0, 48 + bitsFor(x1 - x0 - 1)));
      rs_classify_kernel<<<divUp(nRuns, 256 / WAVE), 256, 0, st>>>(nRuns, perm.p, keyS.p, runStart.p, runFirst.p, E, yBits, x0, rs->dHitStart.p, rs->dHit.p, rs->dPos.p,
                                                                   rs->dMapMosh.p, rs->dMapJ.p, m->info.p, ch->pairs.p, dY.p, dBits.p);
      H10X_HIP(c, hipGetLastError());
      rs->cY.resize(pairBase + nRuns); rs->cBits.resize(pairBase + nRuns);
      H10X_HIP(c, hipMemcpyAsync(rs->cY.data() + pairBase, dY.p, (size_t)nRuns * 4, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(rs->cBits.data() + pairBase, dBits.p, nRuns, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipStreamSynchronize(st));
      pairBase += nRuns;
      rs->chunks.push_back(std::move(ch));
    }
    x0 = x1;
  }
  std::vector<u32> cnt(R);
  H10X_HIP(c, hipMemcpyAsync(cnt.data(), pairCount.p, (size_t)R * 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  for (u32 i = 0; i < R; ++i) rs->pairStart[i + 1] = rs->pairStart[i] + cnt[i];
  if (rs->pairStart[R] != pairBase) return c->fail("overlap table: %llu pairs counted, %llu written", (unsigned long long)rs->pairStart[R], (unsigned long long)pairBase);
  rs->tabled = true;
  return 0;
}

// the side effects of findOverlaps on x and its counts (moshasm.c:302, 322-325, 357, 367-371), from the compact copy
static void rsResolve(ReadSet *rs, u32 x, int *nGood, int *nBad) {
  h10x_read_t &X = rs->reads[x];
  if (rs->nRepeat[x]) X.bad |= BAD_REPEAT;
  int g = 0, b = 0;
  for (u64 p = rs->pairStart[x]; p < rs->pairStart[x + 1]; ++p) {
    const u8 bits = rs->cBits[p];
    if (!(bits & 2)) break;
    if (rs->reads[rs->cY[p]].bad) continue;
    if (bits & 1) ++b; else ++g;
  }
  if (!g && !b) {
    X.bad |= BAD_NOMATCH;
    if (X.nHit < 10) X.bad |= BAD_LOWHIT; else if (X.nCopy[1] < 10) X.bad |= BAD_LOWCOPY1;
  }
  *nGood = g; *nBad = b;
}

// the Overlap array of findOverlaps for x from its rows of the table (fetched by the caller), flags as they are NOW for the y's
static u32 rsOverlapArray(ReadSet *rs, u32 x, const RsPair *rows, u32 nRows, const std::vector<u8> &yBad, h10x_overlap_t *out) {
  u32 k = 0;
  for (u32 i = 0; i <= nRows; ++i) {                         // the array ends with its first entry below 3 hits — or the burned entry 0 (moshasm.c:321-323, 365)
    h10x_overlap_t o; memset(&o, 0, sizeof o);
    if (i < nRows) { o.iy = rows[i].iy; o.nHit = (int32_t)rows[i].nHit; }
    if (i < nRows && rows[i].nHit >= 3) {
      const RsPair &P = rows[i];
      if (!yBad[i]) {
        o.visited = 1; o.isPlus = P.isPlus; o.isBad = P.isBad; o.nPlus = P.nPlus; o.nMinus = P.nMinus; o.sumZ = P.sumZ; o.sumZ2 = P.sumZ2;
        double d = (double)P.sumZ, d2 = (double)P.sumZ2;
        d /= o.nHit; d2 = sqrt(d2 / o.nHit - d * d);         // moshasm.c:355
        o.d = d; o.sd = d2; o.offset = (int32_t)d;
      }
      out[k++] = o;
      continue;
    }
    out[k++] = o;
    break;
  }
  (void)x;
  return k;
}

static int rsFetchRows(ReadSet *rs, u32 x, std::vector<RsPair> &rows) {
  Ctx *c = &rs->m->c;
  const u64 p0 = rs->pairStart[x], cnt = rs->pairStart[x + 1] - p0;
  rows.resize(cnt);
  if (!cnt) return 0;
  for (auto &ch : rs->chunks)
    if (x >= ch->x0 && x < ch->x1) {
      H10X_HIP(c, hipMemcpyAsync(rows.data(), ch->pairs.p + (p0 - ch->pair0), cnt * sizeof(RsPair), hipMemcpyDeviceToHost, c->stream));
      H10X_HIP(c, hipStreamSynchronize(c->stream));
      return 0;
    }
  return c->fail("overlap table: read %u is in no chunk", x);
}

int stageH_overlapCap(ReadSet *rs, u32 ix, u32 *cap) {
  H10X_TRY(moshEnter(rs->m));
  if (ix >= rs->reads.size()) return rs->m->c.fail("read %u is outside the readset of %u reads", ix, (u32)rs->reads.size() - 1);
  H10X_TRY(rsTable(rs));
  *cap = (u32)(rs->pairStart[ix + 1] - rs->pairStart[ix]) + 1;
  return 0;
}

int stageH_overlaps(ReadSet *rs, u32 ix, h10x_overlap_t *out, u32 cap, u32 *nOut, int32_t counts[3]) {
  H10X_TRY(moshEnter(rs->m));
  Ctx *c = &rs->m->c;
  if (ix >= rs->reads.size()) return c->fail("read %u is outside the readset of %u reads", ix, (u32)rs->reads.size() - 1);
  H10X_TRY(rsTable(rs));
  std::vector<RsPair> rows;
  if (out) {
    H10X_TRY(rsFetchRows(rs, ix, rows));
    if (cap < rows.size() + 1) return c->fail("h10x_readset_overlaps: room for %u entries, %u needed", cap, (u32)rows.size() + 1);
  }
  int g = 0, b = 0;
  rsResolve(rs, ix, &g, &b);                                 // first: x's own row sees x's flags as this call leaves badRepeat (moshasm.c:302)
  if (out) {
    // y's flags as the walk saw them. x's own row: no_match is set only when nothing was visited, so x's row was not, and stays so
    std::vector<u8> yBad(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) yBad[i] = rs->reads[rows[i].iy].bad != 0;
    const u32 k = rsOverlapArray(rs, ix, rows.data(), (u32)rows.size(), yBad, out);
    if (nOut) *nOut = k;
  }
  if (counts) { counts[0] = (int32_t)rs->nRepeat[ix]; counts[1] = g; counts[2] = b; }
  return 0;
}

int stageH_markBad(ReadSet *rs, int32_t found[3]) {
  H10X_TRY(moshEnter(rs->m));
  H10X_TRY(rsTable(rs));
  const u32 R = (u32)rs->reads.size();
  for (u32 i = 0; i < R; ++i) rs->reads[i].bad = 0;
  for (int pass = 0; pass < 3; ++pass) {                     // moshasm.c:444-460
    int n = 0, g, b;
    for (u32 x = 0; x < R; ++x) {
      rsResolve(rs, x, &g, &b);
      h10x_read_t &X = rs->reads[x];
      if (pass == 0) { if (b >= 10) { X.bad |= BAD_ORDER10; ++n; } }
      else if (b > (pass == 1 ? 1 : 0) && !(X.bad & BAD_ORDER10)) { X.bad |= BAD_ORDER1; ++n; }
    }
    if (found) found[pass] = n;
  }
  return 0;
}

int stageH_markContained(ReadSet *rs, int32_t *nContained, int32_t *nNot, u64 *totLen) {
  H10X_TRY(moshEnter(rs->m));
  H10X_TRY(rsTable(rs));
  Ctx *c = &rs->m->c;
  const u32 R = (u32)rs->reads.size();
  int nC = 0, nN = 0; u64 tot = 0; size_t ci = 0;
  std::vector<RsPair> rows;                                  // one chunk of the table at a time
  for (u32 x = 0; x < R; ++x) {
    while (ci < rs->chunks.size() && x >= rs->chunks[ci]->x1) ++ci;
    if (ci < rs->chunks.size() && x == rs->chunks[ci]->x0) {
      rows.resize(rs->chunks[ci]->nPairs);
      H10X_HIP(c, hipMemcpyAsync(rows.data(), rs->chunks[ci]->pairs.p, rows.size() * sizeof(RsPair), hipMemcpyDeviceToHost, c->stream));
      H10X_HIP(c, hipStreamSynchronize(c->stream));
    }
    h10x_read_t &X = rs->reads[x];
    if (X.bad) continue;
    int g, b;
    rsResolve(rs, x, &g, &b);
    if (g || b) {                                            // (otherwise nothing was visited: every entry has offset 0 and is passed over, moshasm.c:490)
      const RsPair *row = rows.data() + (rs->pairStart[x] - rs->chunks[ci]->pair0);
      int maxHit = 0;
      for (u64 i = 0, cnt = rs->pairStart[x + 1] - rs->pairStart[x]; i < cnt && row[i].nHit >= 3; ++i) {
        const RsPair &P = row[i];
        const h10x_read_t &Y = rs->reads[P.iy];
        if (P.iy == x || Y.bad) continue;                    // a bad y was not visited: isPlus 0, offset 0 < x->len
        if (Y.len < X.len || (int)P.nHit <= maxHit) continue;
        double d = (double)P.sumZ; d /= (int)P.nHit;
        const int offset = (int)d;
        if (P.isPlus && (offset > 0 || offset + Y.len < X.len)) continue;
        if (!P.isPlus && (offset < X.len || offset - Y.len > 0)) continue;
        X.contained = (int32_t)P.iy; maxHit = (int)P.nHit;
      }
    }
    if (X.contained) ++nC; else { ++nN; tot += (u64)X.len; }
  }
  if (nContained) *nContained = nC; if (nNot) *nNot = nN; if (totLen) *totLen = tot;
  return 0;
}

int stageH_info(ReadSet *rs, h10x_readset_info_t *out) {
  out->nReads = (u32)rs->reads.size(); out->dim = rs->dim; out->totHit = rs->totHit;
  return 0;
}
int stageH_chunks(ReadSet *rs, u32 *out) { *out = rs->tabled ? (u32)rs->chunks.size() : 0; return 0; }
int stageH_export(ReadSet *rs, const h10x_read_t **reads, const u64 **hitStart, const u32 **hit, const u16 **dx) {
  H10X_TRY(moshEnter(rs->m));
  H10X_TRY(rsIndex(rs));                                     // nCopy is invBuild's
  if (reads) *reads = rs->reads.data(); if (hitStart) *hitStart = rs->hitStart.data();
  if (hit) *hit = rs->hit.data(); if (dx) *dx = rs->dx.data();
  return 0;
}
int stageH_statsSums(ReadSet *rs, u64 out[16]) {
  Mosh *m = rs->m;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c;
  const size_t n1 = (size_t)m->max + 1;
  std::vector<u16> d(n1); std::vector<u8> f(n1);
  H10X_HIP(c, hipMemcpyAsync(d.data(), m->depth.p, n1 * 2, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipMemcpyAsync(f.data(), m->info.p, n1, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 16; ++i) out[i] = 0;
  for (size_t i = 1; i < n1; ++i) {
    const int j = f[i] & 3;
    ++out[j];
    if (d[i] > 0) ++out[4 + j];
    if (d[i] > 1) { ++out[8 + j]; out[12 + j] += d[i]; }
  }
  return 0;
}

}  // namespace h10x
