// stage_j.hip — the barcode step between fq2b and the record sort, on packed records: a census of the barcode words (which occur at
// least T times?), a whitelist as a set on the device, and the correction of a batch of records to that whitelist with the statistics
// fq2b -10x prints (fq2b.c:71-104, 157; the README's goodcodes pipeline, README.md:44). The records of a file pass through in batches:
// only the census keys (4 bytes per record) and the whitelist stay on the device between them.
//
//   census   word 0 of every record as it is packed (no byte swap: whitelist order is the order of the packed value) -> radix sort ->
//            run heads by a scan -> (code, count) per distinct barcode -> count >= T selected by a second scan, ascending.
//   set      open addressing over 64-bit slots, barcode << 32 | line with line >= 1, 0 = empty: every 32-bit value is a barcode (all-A is
//            0x00000000, all-T 0xFFFFFFFF), so no key can mean "empty", but no line is 0. Insert = compare-and-swap into an empty slot or
//            a 64-bit max into the slot that holds the barcode already, which is "a repeated line keeps its latest number" without a host
//            pass. At most half the slots are used.
//   fix      one lane per record: 49 look-ups (the barcode and its 48 one-substitution neighbours), the candidate of the latest line
//            wins; keep flags -> exclusive scan -> output offsets; kept records copied one lane per dword with word 0 replaced on the way;
//            the statistics as per-workgroup partial counts in LDS, then one atomic per workgroup and counter.
// The mapping could be computed once per distinct barcode where a census of the same file exists; the per-record form is the one built,
// because --fixFQB has no census and reads its file once, and one form keeps the two commands identical by construction.
#include "prim.hpp"

namespace h10x {

constexpr u64 FQB_SLAB_DEFAULT = (u64)1 << 20;            // records per batch of the host forms: 120 MiB in, 120 MiB out
u64 stageJ_slab(const Ctx *c) { return c->optFqbSlab > 0 ? (u64)c->optFqbSlab : FQB_SLAB_DEFAULT; }

static inline unsigned gridFor(u64 items, unsigned cap) { return (unsigned)hmax<u64>(1, hmin<u64>(divUp(items, 256), cap)); }

// ------------------------------------------------------------------------------------------ census
__global__ void census_keys_kernel(const u32 *__restrict__ rec, u64 n, u32 *__restrict__ key) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) key[i] = rec[i * 30];
}
// flag[i] = key i starts a run (i < n); flag[n] = 0, so that the exclusive scan over n + 1 entries ends in the number of runs
__global__ void census_heads_kernel(const u32 *__restrict__ key, u64 n, u32 *__restrict__ flag) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) flag[i] = (i < n && (i == 0 || key[i] != key[i - 1])) ? 1u : 0u;
}
// run r: its barcode and where it starts; start[D] = n
__global__ void census_runs_kernel(const u32 *__restrict__ key, const u32 *__restrict__ flag, const u32 *__restrict__ ord, u64 n,
                                   u32 *__restrict__ codes, u32 *__restrict__ start) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
    if (i == n) start[ord[n]] = (u32)n;
    else if (flag[i]) { codes[ord[i]] = key[i]; start[ord[i]] = (u32)i; }
  }
}
__global__ void census_counts_kernel(const u32 *__restrict__ start, u64 D, u64 thresh, u32 *__restrict__ counts, u32 *__restrict__ good) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r <= D; r += stride) {
    if (r == D) { good[D] = 0; continue; }
    const u32 cnt = start[r + 1] - start[r];
    counts[r] = cnt; good[r] = (u64)cnt >= thresh ? 1u : 0u;
  }
}
__global__ void census_select_kernel(const u32 *__restrict__ codes, const u32 *__restrict__ counts, const u32 *__restrict__ good, const u32 *__restrict__ pos,
                                     u64 D, u32 *__restrict__ goodCodes, u32 *__restrict__ goodCounts) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < D; r += stride)
    if (good[r]) { goodCodes[pos[r]] = codes[r]; goodCounts[pos[r]] = counts[r]; }
}

int stageJ_censusBegin(Ctx *c, u64 hint) {
  if (hint >= ((u64)1 << 32)) return c->fail("barcode census: %llu records exceed this build's 2^32 limit", hint);
  c->censusN = 0; c->censusOpen = true; c->censusClosed = false; c->censusDistinct = c->censusGood = 0;
  c->censusCodes.release(); c->censusCounts.release(); c->censusGoodCodes.release(); c->censusGoodCounts.release();   // the last census's results go with it
  if (hint > c->censusKeys.n) H10X_HIP(c, c->censusKeys.alloc(hint));
  return 0;
}
int stageJ_censusAdd(Ctx *c, const u32 *dRec, u64 n) {
  if (!c->censusOpen) return c->fail("barcode census: no census is open");
  if (c->censusN + n >= ((u64)1 << 32)) { c->censusOpen = false; return c->fail("barcode census: %llu records exceed this build's 2^32 limit", c->censusN + n); }
  if (!n) return 0;
  if (c->censusN + n > c->censusKeys.n || !c->censusKeys.p) {                      // grow geometrically, keeping the keys so far
    DevBuf<u32> bigger;
    H10X_HIP(c, bigger.alloc(hmax<u64>(c->censusN + n, 2 * (u64)c->censusKeys.n)));
    if (c->censusN) H10X_HIP(c, hipMemcpyAsync(bigger.p, c->censusKeys.p, c->censusN * 4, hipMemcpyDeviceToDevice, c->stream));
    c->censusKeys.swap(bigger);
  }
  census_keys_kernel<<<gridFor(n, 65535u * 4), 256, 0, c->stream>>>(dRec, n, c->censusKeys.p + c->censusN);
  H10X_HIP(c, hipGetLastError());
  c->censusN += n;
  return 0;
}

// ------------------------------------------------------------------------------------------ the whitelist set
__device__ __forceinline__ u64 wl_home(u32 k, u64 mask) { return (((u64)k * 0x9E3779B97F4A7C15ull) >> 24) & mask; }
// codes[i] stands on line i + 1. The walk is bounded by the table size (it ends far earlier: half the slots stay empty).
__global__ void wl_insert_kernel(const u32 *__restrict__ codes, u64 n, u64 *slots, u64 mask) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u32 k = codes[i]; const u64 v = (u64)k << 32 | (u64)(i + 1);
    u64 p = wl_home(k, mask);
    for (u64 t = 0; t <= mask; ++t, p = (p + 1) & mask) {
      u64 cur = __hip_atomic_load(&slots[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!cur) { cur = atomicCAS(&slots[p], 0ull, v); if (!cur) break; }            // taken: ours now; lost the race: look at the winner
      if ((u32)(cur >> 32) == k) { atomicMax(&slots[p], v); break; }                 // the same barcode from another line: the later line stays
    }
  }
}
__device__ __forceinline__ u32 wl_line(const u64 *__restrict__ slots, u64 mask, u32 k) {
  u64 p = wl_home(k, mask);
  for (u64 t = 0; t <= mask; ++t, p = (p + 1) & mask) {
    const u64 cur = slots[p];
    if (!cur) return 0;
    if ((u32)(cur >> 32) == k) return (u32)cur;
  }
  return 0;
}
static int wl_build(Ctx *c, const u32 *dCodes, u64 n) {
  c->haveWhitelist = false; c->wlCodes = 0;
  if (n > ((u64)1 << 31)) return c->fail("whitelist: %llu barcodes exceed this build's 2^31 limit", n);
  if (!n) return 0;
  u64 slots = 1024; while (slots < 2 * n + 2) slots *= 2;
  H10X_HIP(c, c->wlSlots.alloc(slots));
  H10X_HIP(c, hipMemsetAsync(c->wlSlots.p, 0, slots * 8, c->stream));
  wl_insert_kernel<<<gridFor(n, 65535u), 256, 0, c->stream>>>(dCodes, n, c->wlSlots.p, slots - 1);
  H10X_HIP(c, hipGetLastError());
  c->wlMask = slots - 1; c->wlCodes = n; c->haveWhitelist = true;
  return 0;
}
int stageJ_whitelistSet(Ctx *c, const u32 *hostCodes, u64 n) {
  DevBuf<u32> d;
  if (n) { H10X_HIP(c, d.alloc(n)); H10X_HIP(c, hipMemcpyAsync(d.p, hostCodes, n * 4, hipMemcpyHostToDevice, c->stream)); }
  H10X_TRY(wl_build(c, d.p, n));
  H10X_HIP(c, hipStreamSynchronize(c->stream));                                       // the caller's array is its own again
  return 0;
}

int stageJ_censusClose(Ctx *c, int64_t thresh, h10x_census_t *out) {
  if (!c->censusOpen) return c->fail("barcode census: no census is open");
  c->censusOpen = false;
  if (thresh < 1) return c->fail("barcode threshold %lld must be at least 1", (long long)thresh);
  hipStream_t st = c->stream; PrimTemp pt;
  const u64 n = c->censusN;
  u32 D = 0, G = 0; u64 goodRecords = 0;
  c->haveWhitelist = false; c->wlCodes = 0; c->wlSlots.release();                       // the whitelist is replaced: its table goes back before the sort asks for memory
  if (n) {
    DevBuf<u32> sorted, flag, ord, start;
    H10X_HIP(c, sorted.alloc(n));
    H10X_TRY(prim_sort_keys_u32(c, pt, c->censusKeys.p, sorted.p, n, 0, 32));
    H10X_HIP(c, flag.alloc(n + 1)); H10X_HIP(c, ord.alloc(n + 1));
    census_heads_kernel<<<gridFor(n + 1, 65535u * 4), 256, 0, st>>>(sorted.p, n, flag.p);
    H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, ord.p, n + 1));
    H10X_TRY(c->readback(&D, ord.p + n, 4)); H10X_TRY(c->syncReadbacks());
    H10X_HIP(c, c->censusCodes.alloc(D)); H10X_HIP(c, c->censusCounts.alloc(D)); H10X_HIP(c, start.alloc((size_t)D + 1));
    census_runs_kernel<<<gridFor(n + 1, 65535u * 4), 256, 0, st>>>(sorted.p, flag.p, ord.p, n, c->censusCodes.p, start.p);
    flag.release(); ord.release();
    DevBuf<u32> good, pos;
    H10X_HIP(c, good.alloc((size_t)D + 1)); H10X_HIP(c, pos.alloc((size_t)D + 1));
    census_counts_kernel<<<gridFor((u64)D + 1, 65535u), 256, 0, st>>>(start.p, D, (u64)thresh, c->censusCounts.p, good.p);
    H10X_TRY(prim_exclusive_scan_u32(c, pt, good.p, pos.p, (size_t)D + 1));
    H10X_TRY(c->readback(&G, pos.p + D, 4)); H10X_TRY(c->syncReadbacks());
    H10X_HIP(c, c->censusGoodCodes.alloc(G)); H10X_HIP(c, c->censusGoodCounts.alloc(G));
    if (G) {
      census_select_kernel<<<gridFor(D, 65535u), 256, 0, st>>>(c->censusCodes.p, c->censusCounts.p, good.p, pos.p, D, c->censusGoodCodes.p, c->censusGoodCounts.p);
      DevBuf<u64> sum; H10X_HIP(c, sum.alloc(1));
      H10X_TRY(prim_reduce_sum_u32_u64(c, pt, c->censusGoodCounts.p, sum.p, G));
      H10X_TRY(c->readback(&goodRecords, sum.p, 8)); H10X_TRY(c->syncReadbacks());
      H10X_TRY(wl_build(c, c->censusGoodCodes.p, G));
    }
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipStreamSynchronize(st));
  }
  c->censusKeys.release(); c->censusN = 0;                                             // the keys are spent: a new census starts from nothing
  c->censusDistinct = D; c->censusGood = G; c->censusClosed = true;
  if (out) { out->nRecords = n; out->nDistinct = D; out->nGood = G; out->nGoodRecords = goodRecords; }
  return 0;
}
int stageJ_censusExport(Ctx *c, int goodOnly, u32 *codes, u32 *counts, u64 cap) {
  if (!c->censusClosed) return c->fail("barcode census: no closed census to export");
  const u64 m = hmin<u64>(cap, goodOnly ? c->censusGood : c->censusDistinct);
  if (!m) return 0;
  if (codes) H10X_HIP(c, hipMemcpyAsync(codes, goodOnly ? c->censusGoodCodes.p : c->censusCodes.p, m * 4, hipMemcpyDeviceToHost, c->stream));
  if (counts) H10X_HIP(c, hipMemcpyAsync(counts, goodOnly ? c->censusGoodCounts.p : c->censusCounts.p, m * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------ fix
enum { FIX_COUNTERS = 18 };                                 // dropped, corrected, correctedAt[16]
__global__ void __launch_bounds__(256) fix_match_kernel(const u32 *__restrict__ rec, u64 n, const u64 *__restrict__ slots, u64 mask,
                                                        u32 *__restrict__ newCode, u32 *__restrict__ keep /* n + 1 */, u64 *stats) {
  __shared__ u32 part[FIX_COUNTERS];
  if (threadIdx.x < FIX_COUNTERS) part[threadIdx.x] = 0;
  __syncthreads();
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
    if (i == n) { keep[n] = 0; continue; }
    const u32 v = rec[i * 30];
    u32 bestLine = wl_line(slots, mask, v), best = v; int bestBase = -1;
    for (int b = 0; b < 16; ++b) {                          // base b counted from the first base = bits 2 (15 - b)
      const int sh = 2 * (15 - b);
      for (u32 x = 1; x < 4; ++x) {                         // the three other letters at this base
        const u32 u = v ^ (x << sh);
        const u32 ln = wl_line(slots, mask, u);
        if (ln > bestLine) { bestLine = ln; best = u; bestBase = b; }
      }
    }
    keep[i] = bestLine ? 1u : 0u; newCode[i] = best;
    if (!bestLine) atomicAdd(&part[0], 1u);
    else if (bestBase >= 0) { atomicAdd(&part[1], 1u); atomicAdd(&part[2 + bestBase], 1u); }
  }
  __syncthreads();
  if (threadIdx.x < FIX_COUNTERS && part[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (u64)part[threadIdx.x]);
}
// one lane per dword of the input: a kept record's 30 dwords go to its output slot, word 0 replaced
__global__ void fix_copy_kernel(const u32 *__restrict__ rec, const u32 *__restrict__ keep, const u32 *__restrict__ pos, const u32 *__restrict__ newCode,
                                u64 n, u32 *__restrict__ out) {
  const u64 stride = (u64)gridDim.x * blockDim.x, total = n * 30;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const u64 j = t / 30; const u32 w = (u32)(t - j * 30);
    if (keep[j]) out[(u64)pos[j] * 30 + w] = w ? rec[t] : newCode[j];
  }
}
int stageJ_fix(Ctx *c, const u32 *dIn, u64 n, u32 *dOut, u64 *nKept, h10x_fix_stats *acc) {
  static_assert(sizeof(h10x_fix_stats) == FIX_COUNTERS * 8, "h10x_fix_stats: 18 counters");
  if (!c->haveWhitelist) return c->fail("no whitelist: close a census with a good barcode or set one first");
  if (n >= ((u64)1 << 32)) return c->fail("whitelist correction: %llu records in one batch exceed this build's 2^32 limit", n);
  if (nKept) *nKept = 0;
  if (!n) return 0;
  hipStream_t st = c->stream; PrimTemp pt;
  DevBuf<u32> newCode, keep, pos;
  H10X_HIP(c, newCode.alloc(n)); H10X_HIP(c, keep.alloc(n + 1)); H10X_HIP(c, pos.alloc(n + 1));
  DevBuf<u64> stats; H10X_HIP(c, stats.alloc(FIX_COUNTERS));
  H10X_HIP(c, hipMemsetAsync(stats.p, 0, FIX_COUNTERS * 8, st));
  fix_match_kernel<<<gridFor(n + 1, 65535u), 256, 0, st>>>(dIn, n, c->wlSlots.p, c->wlMask, newCode.p, keep.p, stats.p);
  H10X_TRY(prim_exclusive_scan_u32(c, pt, keep.p, pos.p, n + 1));
  fix_copy_kernel<<<gridFor(n * 30, 65535u * 16), 256, 0, st>>>(dIn, keep.p, pos.p, newCode.p, n, dOut);
  H10X_HIP(c, hipGetLastError());
  u32 kept = 0; u64 s[FIX_COUNTERS];
  H10X_TRY(c->readback(&kept, pos.p + n, 4)); H10X_TRY(c->readback(s, stats.p, sizeof s));
  H10X_TRY(c->syncReadbacks());                                                       // behind the copy kernel on the stream: dOut is complete
  if (nKept) *nKept = kept;
  if (acc) { acc->dropped += s[0]; acc->corrected += s[1]; for (int i = 0; i < 16; ++i) acc->correctedAt[i] += s[2 + i]; }
  return 0;
}

}  // namespace h10x
