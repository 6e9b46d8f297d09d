// The galloping run search of hash10x_amd/csrc/runs.hpp (the text the run kernel of census_rows.hip and stage_q.hip's block-run kernels run on
// the device) against a linear walk, as a stand-alone host program under AddressSanitizer:
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 tests/runs_model.cpp -o runs_model && ./runs_model
// Every run length 1 .. 300 (the probes fall at i + 2^j - 1: every 2^j - 1, 2^j and 2^j + 1 is inside), the run ending the array and followed by
// another key, at the array's start and behind other keys, identity and shift projection, 32- and 64-bit keys. Every array is allocated at exactly
// its length: a probe at or beyond n is an ASan report.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../hash10x_amd/csrc/runs.hpp"

typedef unsigned long long u64;

template <typename K, typename Proj>
static u64 walk(const K *keys, u64 n, u64 i, Proj proj) {
  u64 r = i + 1;
  while (r < n && proj(keys[r]) == proj(keys[i])) ++r;
  return r;
}

// keys: `before` keys of one value, `len` of the next, `after` of a third; the low `shift` bits differ inside a run where they are projected away
template <typename K>
static long check(int shift) {
  long bad = 0, cases = 0;
  for (u64 len = 1; len <= 300; ++len)
    for (u64 before : {0ull, 1ull, 5ull})
      for (u64 after : {0ull, 1ull, 3ull}) {
        const u64 n = before + len + after;
        K *keys = new K[n];                                     // exactly n: no slack behind the last key
        for (u64 j = 0; j < n; ++j) {
          const K hi = j < before ? 7 : j < before + len ? 8 : 9;
          keys[j] = shift ? (K)(hi << shift | (j & (((K)1 << shift) - 1))) : hi;
        }
        for (u64 i = before; i < before + len; i += (i - before < 3 || before + len - i < 4) ? 1 : 37) {   // from the head, near it, inside, at the end
          u64 got, exp;
          if (shift) {
            auto proj = [shift](K k) { return (K)(k >> shift); };
            got = run_end(keys, n, i, proj); exp = walk(keys, n, i, proj);
          } else {
            auto proj = [](K k) { return k; };
            got = run_end(keys, n, i, proj); exp = walk(keys, n, i, proj);
          }
          ++cases;
          if (got != exp || exp != before + len) {
            if (++bad <= 10) fprintf(stderr, "run_end: %u-bit keys, shift %d, before %llu len %llu after %llu from %llu: %llu, the walk gives %llu\n",
                                     (unsigned)sizeof(K) * 8, shift, before, len, after, i, got, exp);
          }
        }
        delete[] keys;
      }
  printf("%u-bit keys, shift %d: %ld cases\n", (unsigned)sizeof(K) * 8, shift, cases);
  return bad;
}

int main() {
  long bad = check<uint32_t>(0) + check<uint32_t>(5) + check<u64>(0) + check<u64>(5) + check<u64>(40);
  if (bad) { fprintf(stderr, "%ld mismatches\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
