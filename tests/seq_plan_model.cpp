// The k-mer walk and the batch plan of hash10x_amd/csrc/seq_plan.hpp (the text the three sequence scan kernels and their drivers run) against the plain
// definitions, as a stand-alone host program under AddressSanitizer:
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 tests/seq_plan_model.cpp -o seq_plan_model && ./seq_plan_model
// KmerRoll: every k-mer hashed from scratch, forward and reverse complement, k = 1, 16, 19, 31, walks that start inside a sequence, and palindromic k-mers (a tie
// must report reverse). SeqPlan: sequence lengths around the run of 64 starts, the 23-base skip on odd file ordinals, a sequence too short for it, a batch that
// starts inside a larger seqStart[]. cap(w) is printed for tests/test_seq_plan_cpu.py to compare with gap_cases.scan_cap. Every array is allocated at exactly
// its length: a read beyond it is an ASan report.
#include <cstdio>
#include <cstdlib>
#include "../hash10x_amd/csrc/seq_plan.hpp"

using namespace h10x;

static long bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 10) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static u64 rnd() { static u64 x = 88172645463325252ull; x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }

// the hash of the k-mer at b from scratch (seqhash.c:58-67): fwd = the forward strand is strictly smaller
static u64 scratch_hash(const u8 *b, int k, u64 factor1, bool &fwd) {
  u64 f = 0, rc = 0;
  for (int i = 0; i < k; ++i) f = (f << 2) | (u64)(b[i] & 3);
  for (int i = k - 1; i >= 0; --i) rc = (rc << 2) | (u64)(3 - (b[i] & 3));
  const u64 hf = (f * factor1) >> (64 - 2 * k), hr = (rc * factor1) >> (64 - 2 * k);
  fwd = hf < hr;
  return fwd ? hf : hr;
}

static long check_roll(int k, bool palindromes) {
  long cases = 0;
  const u64 factor1 = rnd() | 1;
  for (int len : {k, k + 1, k + 63, k + 64, k + 200}) {
    u8 *b = new u8[len];                                        // exactly len: no slack behind the last base
    for (int i = 0; i < len; ++i) b[i] = (u8)(rnd() & 3) | (u8)(rnd() & 0x0c);   // the walk reads the low two bits only
    if (palindromes)                                            // every k-th window is its own reverse complement
      for (int p = 0; p + k <= len; p += k) for (int i = 0; i < k / 2; ++i) b[p + k - 1 - i] = (u8)(3 - (b[p + i] & 3));
    for (int p0 : {0, 1, 64, len - k}) {                        // a walk from p0 primes from the bases at p0, wherever that is
      if (p0 < 0 || p0 + k > len) continue;
      KmerRoll roll(k, factor1);
      roll.prime(b + p0);
      for (int j = 0; p0 + j + k <= len; ++j, ++cases) {
        bool fwd; const u64 exp = scratch_hash(b + p0 + j, k, factor1, fwd);
        const u64 got = roll.next(b[p0 + j + k - 1]);
        CHECK(got == exp && roll.fwd() == fwd, "KmerRoll k %d len %d from %d at %d: %llx %d, from scratch %llx %d", k, len, p0, j, got, (int)roll.fwd(), exp, (int)fwd);
        if (palindromes && (p0 + j) % k == 0) CHECK(!roll.fwd() && roll.hf == roll.hr, "KmerRoll k %d: the palindrome at %d reports forward", k, p0 + j);
      }
    }
    delete[] b;
  }
  printf("roll k %d%s: %ld cases\n", k, palindromes ? " palindromes" : "", cases);
  return cases;
}

// one batch: sequences [s0, s0 + nSeq) of all[], under the skip rule or not
static void check_plan(const std::vector<u64> &lens, u32 s0, u32 nSeq, int k, SeqSkip skip, long expectShort) {
  u64 *all = new u64[lens.size() + 1];
  all[0] = 1000;                                                // (the file's first base is not base 0 of the codes either)
  for (size_t i = 0; i < lens.size(); ++i) all[i + 1] = all[i] + lens[i];
  u64 *seqStart = new u64[nSeq + 1];                            // exactly the batch's entries
  for (u32 s = 0; s <= nSeq; ++s) seqStart[s] = all[s0 + s];
  const SeqPlan p(seqStart, nSeq, k, skip);
  CHECK(p.rel.size() == (size_t)nSeq + 1 && p.runStart.size() == (size_t)nSeq + 1, "SeqPlan: vector sizes");
  u64 nK = 0, runs = 0; long firstShort = nSeq;
  for (u32 s = 0; s < nSeq; ++s) {
    const u64 len = lens[s0 + s], off = (skip.odd && ((skip.base + s + 1) % 2 == 1)) ? 23 : 0;
    if (len < off && firstShort == (long)nSeq) firstShort = s;
    const u64 n = len >= off + (u64)k ? len - off - (u64)k + 1 : 0;
    CHECK(p.rel[s] == all[s0 + s] - all[s0] && p.len(s) == len && skip.of(s) == off, "SeqPlan k %d sequence %u: rel %llu len %llu off %llu", k, s, p.rel[s], p.len(s), skip.of(s));
    CHECK(p.runStart[s] == runs, "SeqPlan k %d sequence %u of %llu bases: runStart %llu, expected %llu", k, s, len, p.runStart[s], runs);
    const u64 r = p.runStart[s + 1] - p.runStart[s];
    CHECK(r == (n + 63) / 64 && (n == 0 ? r == 0 : (r - 1) * SEQ_RUN < n && n <= r * SEQ_RUN), "SeqPlan k %d sequence %u: %llu k-mers in %llu runs", k, s, n, r);
    nK += n; runs += r;
  }
  CHECK(p.nK == nK && p.nRuns == runs && p.total == all[s0 + nSeq] - all[s0] && p.rel[nSeq] == p.total, "SeqPlan k %d: nK %llu nRuns %llu total %llu", k, p.nK, p.nRuns, p.total);
  CHECK((long)p.tooShort == firstShort && firstShort == (expectShort < 0 ? (long)nSeq : expectShort), "SeqPlan k %d: tooShort %u, expected %ld", k, p.tooShort, firstShort);
  delete[] seqStart; delete[] all;
}

int main() {
  long cases = 0;
  for (int k : {1, 16, 19, 31}) cases += check_roll(k, false);
  for (int k : {2, 16, 30}) cases += check_roll(k, true);       // (a k-mer of odd length is never its own reverse complement)
  long plans = 0;
  for (int k : {16, 19, 31}) {
    std::vector<u64> lens;
    for (int rep = 0; rep < 2; ++rep)                           // twice: every length falls on an odd and on an even file ordinal
      for (u64 n : {(u64)0, (u64)1, (u64)k - 1, (u64)k, (u64)k + 62, (u64)k + 63, (u64)k + 64, (u64)k + 127, (u64)k + 128, (u64)5}) lens.push_back(n);
    const u32 N = (u32)lens.size();
    check_plan(lens, 0, N, k, SeqSkip{0, 0}, -1); ++plans;
    check_plan(lens, 7, N - 9, k, SeqSkip{0, 0}, -1); ++plans; // a batch from the middle of seqStart[]: the rebasing
    for (u64 base : {(u64)0, (u64)1, (u64)6, (u64)7}) {
      std::vector<u64> skipped(lens);                           // the same lengths behind the skip on the odd ordinals
      for (u32 s = 0; s < N; ++s) if ((base + s + 1) & 1) skipped[s] += 23;
      check_plan(skipped, 0, N, k, SeqSkip{1, base}, -1); ++plans;
      check_plan(skipped, 4, N - 4, k, SeqSkip{1, base + 4}, -1); ++plans;
      std::vector<u64> tooShort(skipped);                       // 22 bases under the skip: reported, and no run
      const u32 at = ((base + 1) & 1) ? 2 : 3;
      tooShort[at] = 22; tooShort[at + 2] = 0;
      check_plan(tooShort, 0, N, k, SeqSkip{1, base}, at); ++plans;
    }
  }
  printf("plan: %ld batches\n", plans);
  struct { int k, w; std::vector<u64> lens; } caps[] = {        // "cap k w value : lens": the estimate of the drivers, for gap_cases.scan_cap
    {19, 31, {140000}}, {19, 31, {140000, 20000, 5000}}, {16, 32, {140000, 20000}}, {16, 1, {0, 1, 15, 16, 78, 79, 80, 143, 144, 145}},
    {16, 3, {0, 1, 15, 16, 78, 79, 80, 143, 144, 145}}, {19, 31, {1000, 1000, 18, 19}}, {31, 7, {3000000}}, {19, 1, {70000}}, {19, 2, {200000}}, {19, 31, {}}};
  for (auto &c : caps) {
    std::vector<u64> st(c.lens.size() + 1, 0);
    for (size_t i = 0; i < c.lens.size(); ++i) st[i + 1] = st[i] + c.lens[i];
    printf("cap %d %d %llu :", c.k, c.w, SeqPlan(st.data(), (u32)c.lens.size(), c.k).cap(c.w));
    for (u64 n : c.lens) printf(" %llu", n);
    printf("\n");
  }
  if (bad) { fprintf(stderr, "%ld mismatches in %ld cases\n", bad, cases); return 1; }
  printf("ok\n");
  return 0;
}
