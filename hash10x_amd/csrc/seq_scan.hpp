// seq_scan.hpp — the device and driver side of the sequence scans over a SeqPlan: a lane's run, the uploaded batch and the two attempts of a scan whose list is
// sized by an estimate. The three scan kernels (stage_d.hip, stage_g.hip, stage_h.hip) are their own per-mosh action over these and KmerRoll.
#pragma once
#include "seq_plan.hpp"
#include "common.hpp"
#include "wave.hpp"

namespace h10x {

// Run `run` of the plan: sequence s, p0 = its first k-mer start in s behind the skip, cnt <= SEQ_RUN starts, ord0 = the ordinal of the k-mer at p0 in the batch,
// b = its first base. A run that starts inside a sequence primes from the k - 1 bases at b like any other
struct KmerRun {
  u32 s; int cnt; u64 p0, ord0; const u8 *b;
  __device__ __forceinline__ static KmerRun open(const u8 *codes, const u64 *seqStart, const u64 *runStart, u32 nSeq, u64 run, int k, SeqSkip skip) {
    KmerRun r; r.s = last_le(runStart, nSeq, run);
    const u64 off = skip.of(r.s), nK = seqStart[r.s + 1] - seqStart[r.s] - off - (u64)k + 1;
    r.p0 = (run - runStart[r.s]) * SEQ_RUN;
    r.cnt = (int)(nK - r.p0 < (u64)SEQ_RUN ? nK - r.p0 : (u64)SEQ_RUN);
    r.ord0 = seqStart[r.s] + off + r.p0; r.b = codes + r.ord0;
    return r;
  }
};

// every way out of a driver waits for the copies that read its plan's vectors: declare it behind the plan
struct StreamWait { hipStream_t s; ~StreamWait() { (void)hipStreamSynchronize(s); } };

// the device side of a plan: the batch's bases (hostCodes = its first), rel[] and runStart[]
struct SeqBatch {
  DevBuf<u8> codes; DevBuf<u64> seq, run;
  int upload(Ctx *c, const SeqPlan &p, const u8 *hostCodes) {
    const size_t n1 = p.rel.size();
    H10X_HIP(c, codes.alloc(p.total + 1)); H10X_HIP(c, seq.alloc(n1)); H10X_HIP(c, run.alloc(n1));
    H10X_HIP(c, hipMemcpyAsync(codes.p, hostCodes, p.total, hipMemcpyHostToDevice, c->stream));
    H10X_HIP(c, hipMemcpyAsync(seq.p, p.rel.data(), n1 * 8, hipMemcpyHostToDevice, c->stream));
    H10X_HIP(c, hipMemcpyAsync(run.p, p.runStart.data(), n1 * 8, hipMemcpyHostToDevice, c->stream));
    return 0;
  }
};

// The list is sized by the plan's estimate and the scan repeated at the exact size if it listed more. launch(cap) sizes the list, clears the tally and launches;
// tally[0 .. nTally) comes back from dTally, tally[0] = entries listed; onRetry() clears what the first attempt counted; overflow = the error text
template <typename Launch, typename Retry>
static int seqScanTwice(Ctx *c, u64 cap, const u64 *dTally, u64 *tally, int nTally, const char *overflow, Launch &&launch, Retry &&onRetry) {
  for (int attempt = 0; attempt < 2; ++attempt) {
    H10X_TRY(launch(cap)); H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(tally, dTally, (size_t)nTally * 8, hipMemcpyDeviceToHost, c->stream));
    H10X_HIP(c, hipStreamSynchronize(c->stream));            // (the plan's vectors are free to go from here)
    if (tally[0] <= cap) return 0;
    if (attempt) break;
    cap = tally[0]; ++c->scanRetries;                        // the estimate was too small: once more with the exact size
    H10X_TRY(onRetry());
  }
  return c->fail("%s", overflow);
}

}  // namespace h10x
