// stage_m.hip — the linkage groups behind --shareComponents: the connected components of the share graph at a threshold T over all blocks.
//
// Every row entry (c, d) of the share graph (stage_l.hip) is an undirected edge {c, d}. The rows of a block range are born on the device and stay
// there: a label per block, parent[nBlocks], lives in the context, and each range's rows are folded into it as soon as the census has made them.
//   hook     one thread per row of the range (the source block by binary search in the range's offsets): lock-free union by smaller root
//            (unionfind.hpp: every loop is bounded by nBlocks, nothing waits for another wave).
//   check    the same rows: how many still have ends with different roots. While that is non-zero the hook runs again over the range (sets
//            only merge: a satisfied range stays satisfied, whatever later ranges do). Bounded rounds; running out of them is an error.
//   finish   root[c] by a find per block; the roots c >= 1 flagged, scanned, numbered in ascending order; comp[c] = number(root[c]) + 1; member
//            counts and record sums by integer atomics (exact, order-free); the largest component and the singletons with one atomic per
//            workgroup.
// parent[] is rewritten by other CUs and XCDs while hook runs, so inside these kernels every read of it is a relaxed agent-scope atomic load (it
// bypasses the CU's L1, which no other CU's store refreshes) and every write an agent-scope atomic. Between kernels the launch boundary orders.
#include "common.hpp"
#include "prim.hpp"
#include "unionfind.hpp"
#include "wave.hpp"

namespace h10x {

static constexpr u32 SM_MAX_ROUNDS = 64;                     // hook rounds per range (one is the rule: the hook leaves nothing undone by itself)
static constexpr unsigned SM_GRID = 2048;                    // workgroups of the kernels that end in one atomic each

typedef UfDevice<__HIP_MEMORY_SCOPE_AGENT> SmWords;          // parent[]: global memory, rewritten by every CU

__global__ void sm_init_kernel(u32 *__restrict__ parent, u32 nB) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nB) parent[c] = c;
}

// one thread per row: union of the row's block (c0 + its slot: the last q with offsets[q] <= i; offsets[0] = 0, offsets[nq] = rows) and its
// entry. Block 0 holds no records and stands in no list; an entry outside [1, nB) is skipped, never followed
__global__ __launch_bounds__(256) void sm_hook_kernel(const u64 *__restrict__ offsets, const u32 *__restrict__ block, u64 rows, u32 c0, u32 nq,
                                                      u32 *parent, u32 nB) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    const u32 a = c0 + last_le(offsets, nq, i), b = block[i];
    if (!a || !b || a >= nB || b >= nB) continue;
    uf_union<SmWords>(parent, a, b, nB);
  }
}

// *open += rows of the range whose two ends have different roots (one atomic per workgroup)
__global__ __launch_bounds__(256) void sm_check_kernel(const u64 *__restrict__ offsets, const u32 *__restrict__ block, u64 rows, u32 c0, u32 nq,
                                                       u32 *parent, u32 nB, u32 *__restrict__ open) {
  __shared__ u32 sOpen[256 / WAVE];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u32 n = 0;
  for (u64 i0 = (u64)blockIdx.x * blockDim.x; i0 < rows; i0 += stride) {
    const u64 i = i0 + threadIdx.x;
    if (i < rows) {
      const u32 a = c0 + last_le(offsets, nq, i), b = block[i];
      if (a && b && a < nB && b < nB && uf_find<SmWords>(parent, a, nB) != uf_find<SmWords>(parent, b, nB)) ++n;
    }
  }
  n = wg_sum(n, sOpen);
  if (threadIdx.x == 0 && n) atomicAdd(open, n);
}

// root[c] for every block, and flag[c] = 1 for the roots c >= 1 (flag[nB] = 0: the scan's last entry is the number of components)
__global__ void sm_root_kernel(u32 *parent, u32 nB, u32 *__restrict__ root, u32 *__restrict__ flag) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > nB) return;
  if (c == nB) { flag[c] = 0; return; }
  const u32 r = uf_find<SmWords>(parent, c, nB);
  root[c] = r; flag[c] = (c >= 1 && r == c) ? 1u : 0u;
}

// comp[c] = number(root[c]) + 1, the component's member count and record sum, and the root of every component. The lanes of a wave that hold the
// same component add up first and send one atomic for all of them: with one atomic a block, the 479 062 members of the largest component of the
// yeast-like molecule graph all met on two words, 6.4 ms of a 45 ms request. Integer sums: exact whatever the grouping
__global__ __launch_bounds__(256) void sm_label_kernel(const u32 *__restrict__ root, const u32 *__restrict__ num, const h10x_block *__restrict__ blocks, u32 nB,
                                                       u32 nComp, u32 *__restrict__ comp, u32 *__restrict__ rootOf, u32 *__restrict__ nMember,
                                                       unsigned long long *__restrict__ records) {
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;       // (no early return: the ballots below want every lane of the wave)
  const u32 lane = threadIdx.x & (WAVE - 1);
  u32 k = 0, nh = 0;
  if (c >= 1 && c < nB) {
    const u32 r = root[c];
    k = r < nB ? num[r] + 1 : 0;
    if (k > nComp) k = 0;                                     // (cannot be: a root is flagged)
    comp[c] = k;
    if (k && r == c) rootOf[k] = c;
    if (k) nh = blocks[c].nHash;
  } else if (c == 0 && nB) comp[0] = 0;
  u64 todo = __ballot(k != 0);
  while (todo) {                                              // wave-uniform: one turn per distinct component among the lanes
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const u32 kl = (u32)__shfl((int)k, lead);
    const bool mine = k == kl;
    const u64 m = __ballot(mine);
    const u64 sum = wave_sum((u64)(mine ? nh : 0));
    if (lane == (u32)lead) { atomicAdd(nMember + kl, (u32)__popcll(m)); if (sum) atomicAdd(records + kl, (unsigned long long)sum); }
    todo &= ~m;
  }
}

// out[0] = the largest member count (atomicMax), out[1] = components of one block (atomicAdd): one atomic each per workgroup
__global__ __launch_bounds__(256) void sm_summary_kernel(const u32 *__restrict__ nMember, u32 nComp, u32 *__restrict__ out) {
  __shared__ u32 sMax[256 / WAVE], sOne[256 / WAVE];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const u32 lane = threadIdx.x & (WAVE - 1);
  u32 mx = 0, one = 0;
  for (u64 k = 1 + (u64)blockIdx.x * blockDim.x + threadIdx.x; k <= nComp; k += stride) {
    const u32 m = nMember[k];
    mx = mx > m ? mx : m; one += m == 1;
  }
  // two values through one butterfly and one barrier: wave.hpp's folds take one value each and would make two of both
  for (int k = 32; k; k >>= 1) { const u32 o = (u32)__shfl_xor((int)mx, k); mx = mx > o ? mx : o; one += (u32)__shfl_xor((int)one, k); }
  if (lane == 0) { sMax[threadIdx.x / WAVE] = mx; sOne[threadIdx.x / WAVE] = one; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (u32 w = 1; w < blockDim.x / WAVE; ++w) { mx = mx > sMax[w] ? mx : sMax[w]; one += sOne[w]; }
    if (mx) atomicMax(out, mx);
    if (one) atomicAdd(out + 1, one);
  }
}

// ---------------------------------------------------------------------------------------------------------- driver
void stageM_release(Ctx *c) {
  c->scOpen = false; c->haveShareComp = false; c->scComps = 0; c->scBlocks = 0;
  c->scParent.release(); c->scComp.release(); c->scRoot.release(); c->scRootOf.release(); c->scMembers.release(); c->scRecords.release();
}

int stageM_begin(Ctx *c, int64_t minShare) {
  stageM_release(c);
  H10X_TRY(ce_check(c, "shareComponents", minShare));
  const u32 nB = c->nBlocks;
  H10X_HIP(c, c->scParent.alloc(nB));
  if (nB) sm_init_kernel<<<divUp(nB, 256), 256, 0, c->stream>>>(c->scParent.p, nB);
  H10X_HIP(c, hipGetLastError());
  memset(&c->scInfo, 0, sizeof c->scInfo);
  c->scInfo.nBlocks = nB; c->scInfo.minShare = (u32)hmin<int64_t>(minShare, 0xFFFFFFFFll);
  c->scMinShare = minShare; c->scBlocks = nB; c->scOpen = true;
  return 0;
}

// census of blocks [codeMin, codeMax) (stage_l.hip: the rows stay on the device), then hook and check until no row of the range is open
int stageM_add(Ctx *c, u32 codeMin, u32 codeMax) {
  if (!c->scOpen) return c->fail("shareComponents: add without begin (a new range, --clusterSplit and a new state end a run)");
  h10x_share_graph_info g;
  int rc = stageL_run(c, c->scMinShare, codeMin, codeMax, &g);
  if (rc) { stageM_release(c); return rc; }
  h10x_share_components_info &z = c->scInfo;
  z.rows += g.rows; z.listEntries += g.listEntries; z.batches += g.batches; z.windows += g.windows;
  const u32 nq = g.codeMax - g.codeMin, nB = c->scBlocks;
  if (!g.rows || !nq) return 0;
  hipStream_t st = c->stream;
  DevBuf<u32> open; H10X_HIP(c, open.alloc(1));
  const unsigned grid = (unsigned)hmin<u64>(divUp(g.rows, 256), SM_GRID);
  for (u32 round = 0;; ++round) {
    if (round == SM_MAX_ROUNDS) {
      stageM_release(c);
      return c->fail("shareComponents: blocks [%u, %u) still have rows across two components after %u hook rounds", g.codeMin, g.codeMax, SM_MAX_ROUNDS);
    }
    sm_hook_kernel<<<(unsigned)hmin<u64>(divUp(g.rows, 256), 65536), 256, 0, st>>>(c->sg.offsets.p, c->sg.a.p, g.rows, g.codeMin, nq, c->scParent.p, nB);
    H10X_HIP(c, hipGetLastError());
    ++z.hookRounds;
    H10X_HIP(c, hipMemsetAsync(open.p, 0, 4, st));
    sm_check_kernel<<<grid, 256, 0, st>>>(c->sg.offsets.p, c->sg.a.p, g.rows, g.codeMin, nq, c->scParent.p, nB, open.p);
    H10X_HIP(c, hipGetLastError());
    u32 left = 0;
    H10X_TRY(c->readback(&left, open.p, 4)); H10X_TRY(c->syncReadbacks());
    if (!left) break;
  }
  return 0;
}

int stageM_finish(Ctx *c, h10x_share_components_info *info) {
  if (!c->scOpen) return c->fail("shareComponents: finish without begin (a new range, --clusterSplit and a new state end a run)");
  c->scOpen = false;
  stageL_release(c);                                          // the last range's rows: folded in, no longer wanted
  hipStream_t st = c->stream;
  const u32 nB = c->scBlocks;
  h10x_share_components_info &z = c->scInfo;
  PrimTemp pt; DevBuf<u32> flag, num, sum;
  H10X_HIP(c, c->scRoot.alloc(nB)); H10X_HIP(c, c->scComp.alloc(nB));
  H10X_HIP(c, flag.alloc((size_t)nB + 1)); H10X_HIP(c, num.alloc((size_t)nB + 1)); H10X_HIP(c, sum.alloc(2));
  sm_root_kernel<<<divUp((u64)nB + 1, 256), 256, 0, st>>>(c->scParent.p, nB, c->scRoot.p, flag.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, num.p, (size_t)nB + 1));
  u32 nComp = 0;
  H10X_TRY(c->readback(&nComp, num.p + nB, 4)); H10X_TRY(c->syncReadbacks());
  H10X_HIP(c, c->scRootOf.alloc((size_t)nComp + 1)); H10X_HIP(c, c->scMembers.alloc((size_t)nComp + 1)); H10X_HIP(c, c->scRecords.alloc((size_t)nComp + 1));
  H10X_HIP(c, hipMemsetAsync(c->scRootOf.p, 0, ((size_t)nComp + 1) * 4, st));
  H10X_HIP(c, hipMemsetAsync(c->scMembers.p, 0, ((size_t)nComp + 1) * 4, st));
  H10X_HIP(c, hipMemsetAsync(c->scRecords.p, 0, ((size_t)nComp + 1) * 8, st));
  H10X_HIP(c, hipMemsetAsync(sum.p, 0, 8, st));
  if (nB) sm_label_kernel<<<divUp(nB, 256), 256, 0, st>>>(c->scRoot.p, num.p, c->blocks.p, nB, nComp, c->scComp.p, c->scRootOf.p, c->scMembers.p,
                                                          (unsigned long long *)c->scRecords.p);
  if (nComp) sm_summary_kernel<<<(unsigned)hmin<u64>(divUp(nComp, 256), SM_GRID), 256, 0, st>>>(c->scMembers.p, nComp, sum.p);
  H10X_HIP(c, hipGetLastError());
  u32 s2[2] = {0, 0};
  H10X_TRY(c->readback(s2, sum.p, 8)); H10X_TRY(c->syncReadbacks());
  H10X_HIP(c, hipStreamSynchronize(st));
  c->scParent.release();
  z.nComponents = nComp; z.largest = s2[0]; z.singletons = s2[1];
  c->scComps = nComp; c->haveShareComp = true;
  if (info) *info = z;
  return 0;
}

// comp[nBlocks], root[nBlocks] (the first min(capBlocks, nBlocks)) and rootOf / blocks / records [nComponents + 1] (the first min(capComps, that)); any may be null
int stageM_get(Ctx *c, u32 *comp, u32 *root, u32 *rootOf, u32 *nMember, u64 *records, u64 capBlocks, u64 capComps) {
  if (!c->haveShareComp) return c->fail("shareComponents: no result is kept (run begin, add and finish first; a new range, --clusterSplit and a new state release it)");
  const size_t nb = (size_t)hmin<u64>(capBlocks, c->scBlocks), nc = (size_t)hmin<u64>(capComps, (u64)c->scComps + 1);
  if (nb && comp) H10X_HIP(c, hipMemcpyAsync(comp, c->scComp.p, nb * 4, hipMemcpyDeviceToHost, c->stream));
  if (nb && root) H10X_HIP(c, hipMemcpyAsync(root, c->scRoot.p, nb * 4, hipMemcpyDeviceToHost, c->stream));
  if (nc && rootOf) H10X_HIP(c, hipMemcpyAsync(rootOf, c->scRootOf.p, nc * 4, hipMemcpyDeviceToHost, c->stream));
  if (nc && nMember) H10X_HIP(c, hipMemcpyAsync(nMember, c->scMembers.p, nc * 4, hipMemcpyDeviceToHost, c->stream));
  if (nc && records) H10X_HIP(c, hipMemcpyAsync(records, c->scRecords.p, nc * 8, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace h10x
