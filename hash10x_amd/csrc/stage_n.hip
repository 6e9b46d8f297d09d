// stage_n.hip — the per-hash linkage groups behind --hashCopies: for every hash x in the depth range, the connected components of the share
// graph at a threshold T restricted to the blocks that hold x.
//
// L(x) is x's barcode list (ascending, a block as often as it holds x), D(x) its distinct blocks, m = |D(x)|. a and b of D(x) are joined when
// b stands in a's row of the share graph (stage_l.hip) or a in b's. Per x: distinct = m, groups, largest, second (include/h10x.h).
//   census   stageL_run over all blocks at T: offsets / block stay on the device and are the graph;
//   flag     flag[x] = x in range (x >= 1), the deepest in-range list by one atomicMax per workgroup; a scan of the flags numbers the hashes,
//            compact writes their indices back to back;
//   groups   ONE WAVE per in-range hash, nothing in it waits for another wave. The list is deduped into LDS (D) with the labels beside it
//            (lab[i] = i). For each member a the wave streams a's row in coalesced 64-wide steps; each entry is looked up in D by binary search
//            in LDS; a hit is an edge and is hooked with the union by smaller label of unionfind.hpp, on LDS words (lab[i] <= i always,
//            so every loop is bounded by m). After a pass the labels are flattened and the roots counted:
//            the passes end when a pass hooked nothing or one root is left (sets only merge); running out of m passes is an error word.
//            Then the members per root are counted in LDS (D's words, no longer wanted), groups / largest / second reduced across the
//            wave, and the 8 bytes written by one store.
//   tally    per crib type the in-range hashes, those in one group, those with second >= 2, and the deepest list: one atomic per workgroup
//            and counter.
// This reads 4 B per list entry and 4 B per row entry of every member, contiguously. The other form, a look-up of each of the m^2 pairs in
// the rows in global memory, would make m^2 log2(row) dependent 4-byte reads per hash and was not built.
// The lanes of a wave run in lockstep and its LDS operations complete in order, so inside a wave a fence for the compiler is all the
// synchronisation there is; labels that other lanes rewrite are read with atomic loads.
#include "common.hpp"
#include "prim.hpp"
#include "unionfind.hpp"
#include "wave.hpp"

namespace h10x {

static constexpr u32 HC_MAX_DEPTH = 4096;                     // a deeper in-range list is refused: the working set of a wave is 2 x 4096 words of LDS at most
static constexpr unsigned HC_GRID = 2048;                     // workgroups of the kernels that end in one atomic per counter
static constexpr size_t HC_LDS_BYTES = 65536;                 // dynamic LDS of a workgroup of the groups kernel, at most

__device__ __forceinline__ void hc_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ u32 hc_load(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
typedef UfDevice<__HIP_MEMORY_SCOPE_WAVEFRONT> HcWords;      // lab[]: LDS words of one wave (indices into D)

// flag[x] = 1 for the in-range hashes x >= 1 (flag[U1] = 0: the scan's last entry is their number); *deepest = the longest of their lists
__global__ __launch_bounds__(256) void hc_flag_kernel(const u8 *__restrict__ within, const u32 *__restrict__ hashDepth, u32 U1, u32 *__restrict__ flag,
                                                      u32 *__restrict__ deepest) {
  __shared__ u32 sMax[256 / WAVE];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u32 mx = 0;
  for (u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; x <= U1; x += stride) {
    u32 f = 0;
    if (x >= 1 && x < U1 && within[x]) { f = 1; const u32 d = hashDepth[x]; mx = mx > d ? mx : d; }
    flag[x] = f;
  }
  mx = wg_max(mx, sMax);
  if (threadIdx.x == 0 && mx) atomicMax(deepest, mx);
}

__global__ void hc_compact_kernel(const u32 *__restrict__ flag, const u32 *__restrict__ pos, u32 U1, u32 nx, u32 *__restrict__ xs) {
  const u32 x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < U1 && flag[x] && pos[x] < nx) xs[pos[x]] = x;
}

// one wave per in-range hash xs[w]. LDS: per wave D[cap] and lab[cap], cap >= the deepest in-range list. offsets[] / block[] are the share graph
// of blocks 1 .. nBlocks-1 (the row of block a at offsets[a - 1]); out[x] = {distinct | groups << 16, largest | second << 16}
__global__ __launch_bounds__(256) void hc_groups_kernel(const u32 *__restrict__ xs, u32 nx, const u32 *__restrict__ hashDepth, const u64 *__restrict__ rowStart,
                                                        const u32 *__restrict__ rows, const u64 *__restrict__ offsets, const u32 *__restrict__ block,
                                                        u32 nBlocks, u32 cap, uint2 *__restrict__ out, u32 *__restrict__ err) {
  extern __shared__ u32 hcLds[];
  const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, wpw = blockDim.x / WAVE;
  u32 *D = hcLds + (size_t)wave * 2 * cap, *lab = D + cap;
  for (u64 w = (u64)blockIdx.x * wpw + wave; w < nx; w += (u64)gridDim.x * wpw) {   // wave-uniform throughout
    const u32 x = xs[w];
    const u32 depth = hashDepth[x], len = depth < cap ? depth : cap;                // (depth <= cap: the driver sized cap from the deepest list)
    const u64 rs = rowStart[x];
    u32 m = 0;
    for (u32 j0 = 0; j0 < len; j0 += WAVE) {                  // dedupe: the list ascends
      const u32 j = j0 + lane;
      u32 v = 0; bool keep = false;
      if (j < len) { v = rows[rs + j]; keep = j == 0 || rows[rs + j - 1] != v; }
      const u32 p = wave_place(keep, m);
      if (keep) { D[p] = v; lab[p] = p; }                     // p < len <= cap
    }
    hc_sync();
    if (m > 1) {
      for (u32 pass = 0;; ++pass) {
        if (pass == m) { if (lane == 0) err[0] = x; break; }
        bool changed = false;
        for (u32 ia = 0; ia < m; ++ia) {
          const u32 a = (u32)__builtin_amdgcn_readfirstlane((int)D[ia]);
          if (!a || a >= nBlocks) continue;                   // block 0 stands in no list; a number out of range is never followed
          const u64 r0 = offsets[a - 1], r1 = offsets[a];
          for (u64 r = r0; r < r1; r += WAVE) {
            const u64 j = r + lane;
            if (j < r1) {
              const u32 b = block[j];
              const u32 l = lower_bound(D, 0u, m, b);
              if (l < m && l != ia && D[l] == b) changed |= uf_union<HcWords>(lab, ia, l, m);
            }
          }
        }
        hc_sync();
        u32 roots = 0;
        for (u32 i0 = 0; i0 < m; i0 += WAVE) {                // flatten, count the roots
          const u32 i = i0 + lane;
          bool isRoot = false;
          if (i < m) { const u32 r = uf_find<HcWords>(lab, i, m); isRoot = r == i; if (!isRoot) atomicMin(lab + i, r); }
          roots += (u32)__popcll(__ballot(isRoot));
        }
        hc_sync();
        if (!__ballot(changed) || roots == 1) break;          // sets only merge: one set, or a pass that found every edge inside a set
      }
    }
    u32 *cnt = D;                                             // members per root, in D's words
    for (u32 i = lane; i < m; i += WAVE) cnt[i] = 0;
    hc_sync();
    for (u32 i = lane; i < m; i += WAVE) { const u32 r = hc_load(lab + i); if (r < m) atomicAdd(cnt + r, 1u); }
    hc_sync();
    u32 groups = 0, first = 0, second = 0;
    for (u32 i = lane; i < m; i += WAVE) {
      const u32 n = hc_load(cnt + i);
      if (!n) continue;
      ++groups;
      if (n > first) { second = first; first = n; } else if (n > second) second = n;
    }
    for (int k = 32; k; k >>= 1) {                            // the two largest of two disjoint sets of counts
      groups += (u32)__shfl_xor((int)groups, k);
      const u32 of = (u32)__shfl_xor((int)first, k), os = (u32)__shfl_xor((int)second, k);
      const u32 lo = first < of ? first : of, s2 = second > os ? second : os;
      first = first > of ? first : of; second = lo > s2 ? lo : s2;
    }
    if (lane == 0) out[x] = make_uint2(m | groups << 16, first | second << 16);
    hc_sync();                                                // the next hash rewrites D and lab
  }
}

// counts[3 * t + k] for crib type t (0 without a crib): k = 0 in-range hashes, 1 those with groups == 1, 2 those with second >= 2; counts[15] =
// the deepest list (atomicMax). One atomic per workgroup and counter
__global__ __launch_bounds__(256) void hc_tally_kernel(const u32 *__restrict__ xs, u32 nx, const uint2 *__restrict__ out, const u8 *__restrict__ cribType /* null: no crib */,
                                                       const u32 *__restrict__ hashDepth, unsigned long long *__restrict__ counts) {
  __shared__ u32 sCnt[256 / WAVE][16];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  u32 n[15], mx = 0;
  for (int k = 0; k < 15; ++k) n[k] = 0;
  for (u64 w0 = (u64)blockIdx.x * blockDim.x; w0 < nx; w0 += stride) {   // wave-uniform: whole workgroups
    const u64 w = w0 + threadIdx.x;
    u32 t = 5; bool one = false, split = false;
    if (w < nx) {
      const u32 x = xs[w]; const uint2 r = out[x];
      t = cribType ? cribType[x] : 0; if (t > 4) t = 0;
      one = (r.x >> 16) == 1; split = (r.y >> 16) >= 2;
      const u32 d = hashDepth[x]; mx = mx > d ? mx : d;
    }
#pragma unroll
    for (u32 k = 0; k < 5; ++k) {
      n[3 * k] += (u32)__popcll(__ballot(t == k)); n[3 * k + 1] += (u32)__popcll(__ballot(t == k && one)); n[3 * k + 2] += (u32)__popcll(__ballot(t == k && split));
    }
  }
  mx = wave_max(mx);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 15; ++k) sCnt[wave][k] = n[k];
    sCnt[wave][15] = mx;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const u32 k = threadIdx.x;
    u32 v = sCnt[0][k];
    for (u32 q = 1; q < blockDim.x / WAVE; ++q) v = k == 15 ? (v > sCnt[q][k] ? v : sCnt[q][k]) : v + sCnt[q][k];
    if (v) { if (k == 15) atomicMax(counts + k, (unsigned long long)v); else atomicAdd(counts + k, (unsigned long long)v); }
  }
}

// ---------------------------------------------------------------------------------------------------------- driver
void stageN_release(Ctx *c) {
  c->haveHashCopies = false; c->hcHashes = 0; c->hcOut.release();
  memset(c->hcTally, 0, sizeof c->hcTally); memset(&c->hcInfo, 0, sizeof c->hcInfo);
}

int stageN_run(Ctx *c, int64_t minShare, h10x_hash_copies_info *info) {
  release_share_results(c);                                   // the census below uses the share graph's arrays
  H10X_TRY(ce_check(c, "hashCopies", minShare));
  hipStream_t st = c->stream;
  const u32 U1 = c->hashNumber;
  PrimTemp pt; DevBuf<u32> flag, pos, small;
  H10X_HIP(c, flag.alloc((size_t)U1 + 1)); H10X_HIP(c, pos.alloc((size_t)U1 + 1)); H10X_HIP(c, small.alloc(2));
  H10X_HIP(c, hipMemsetAsync(small.p, 0, 8, st));             // [0] the deepest in-range list, [1] the error word of the groups kernel
  hc_flag_kernel<<<(unsigned)hmin<u64>(divUp((u64)U1 + 1, 256), HC_GRID), 256, 0, st>>>(c->within.p, c->hashDepth.p, U1, flag.p, small.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, pos.p, (size_t)U1 + 1));
  u32 nx = 0, deepest = 0;
  H10X_TRY(c->readback(&nx, pos.p + U1, 4)); H10X_TRY(c->readback(&deepest, small.p, 4)); H10X_TRY(c->syncReadbacks());
  if (deepest > HC_MAX_DEPTH) return c->fail("!! hashCopies needs every hash in range to have depth <= %u (deepest %u)", HC_MAX_DEPTH, deepest);
  h10x_share_graph_info g;
  H10X_TRY(stageL_run(c, minShare, 1, 0, &g));
  struct DropGraph { Ctx *c; ~DropGraph() { stageL_release(c); } } drop{c};   // the rows are wanted until the groups kernel is done, and by nobody after
  h10x_hash_copies_info &z = c->hcInfo;
  z.hashNumber = U1; z.minShare = (u32)hmin<int64_t>(minShare, 0xFFFFFFFFll); z.inRange = nx; z.rows = g.rows; z.listEntries = g.listEntries;
  z.deepest = deepest; z.batches = g.batches; z.windows = g.windows;
  H10X_HIP(c, c->hcOut.alloc((size_t)2 * hmax<u32>(U1, 1)));
  H10X_HIP(c, hipMemsetAsync(c->hcOut.p, 0, (size_t)8 * hmax<u32>(U1, 1), st));
  DevBuf<unsigned long long> counts; H10X_HIP(c, counts.alloc(16));
  H10X_HIP(c, hipMemsetAsync(counts.p, 0, 16 * 8, st));
  if (nx) {
    DevBuf<u32> xs; H10X_HIP(c, xs.alloc(nx));
    hc_compact_kernel<<<divUp(U1, 256), 256, 0, st>>>(flag.p, pos.p, U1, nx, xs.p);
    const u32 cap = hmax<u32>((deepest + WAVE - 1) / WAVE * WAVE, WAVE);          // LDS words per array and wave: from the state's deepest list, not from the limit
    const u32 wpw = (u32)hmin<size_t>(4, HC_LDS_BYTES / ((size_t)cap * 8));       // cap <= 4096: at least two waves
    const unsigned grid = (unsigned)hmin<u64>(divUp(nx, wpw), 65536);
    hc_groups_kernel<<<grid, wpw * WAVE, (size_t)wpw * cap * 8, st>>>(xs.p, nx, c->hashDepth.p, c->rowStart.p, c->rows.p, c->sg.offsets.p, c->sg.a.p, c->nBlocks, cap,
                                                                       (uint2 *)c->hcOut.p, small.p + 1);
    H10X_HIP(c, hipGetLastError());
    hc_tally_kernel<<<(unsigned)hmin<u64>(divUp(nx, 256), HC_GRID), 256, 0, st>>>(xs.p, nx, (const uint2 *)c->hcOut.p, c->haveCrib ? c->cribType.p : nullptr, c->hashDepth.p,
                                                                                  counts.p);
    H10X_HIP(c, hipGetLastError());
    u32 bad = 0;
    H10X_TRY(c->readback(&bad, small.p + 1, 4)); H10X_TRY(c->readback(c->hcTally, counts.p, 16 * 8)); H10X_TRY(c->syncReadbacks());
    H10X_HIP(c, hipStreamSynchronize(st));                    // xs goes back to the block cache
    if (bad) { stageN_release(c); return c->fail("hashCopies: the blocks of hash %u were not all joined after as many hook passes as it has blocks", bad); }
    if (c->hcTally[15] != deepest) { stageN_release(c); return c->fail("hashCopies: the deepest list is %u at the flags and %llu at the tally", deepest, (unsigned long long)c->hcTally[15]); }
  }
  H10X_HIP(c, hipStreamSynchronize(st));
  for (int t = 0; t < 5; ++t) { z.oneGroup += c->hcTally[3 * t + 1]; z.split += c->hcTally[3 * t + 2]; }
  c->hcHashes = U1; c->haveHashCopies = true;
  if (info) *info = z;
  return 0;
}

// records [first, first + count) of the kept result (4 x u16 each) to host (toDevice = 0) or device memory; out = null only asks whether one is kept
int stageN_get(Ctx *c, uint16_t *out, u64 first, u64 count, int toDevice) {
  if (!c->haveHashCopies) return c->fail("hashCopies: no result is kept (run it first; a new range, --clusterSplit and a new state release it)");
  if (!out) return 0;
  if (first > c->hcHashes || count > c->hcHashes - first) return c->fail("hashCopies: records [%llu, %llu) beyond the %u hashes", (unsigned long long)first, (unsigned long long)(first + count), c->hcHashes);
  if (count) H10X_HIP(c, hipMemcpyAsync(out, c->hcOut.p + 2 * first, (size_t)count * 8, toDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int stageN_tally(Ctx *c, u64 *counts15) {
  if (!c->haveHashCopies) return c->fail("hashCopies: no result is kept (run it first; a new range, --clusterSplit and a new state release it)");
  for (int k = 0; k < 15; ++k) counts15[k] = c->hcTally[k];
  return 0;
}

}  // namespace h10x
