// runs.hpp — the end of a run of equal keys in a sorted array, the one text behind the run kernel of census_rows.hip (whole keys), stage_q.hip's
// sq_blocks_kernel and sq_unit_kernel (keys >> lb: a block's run) and the host model of tests/runs_model.cpp (the same loops under
// AddressSanitizer against a linear walk). The header needs no HIP header.
#pragma once

#ifdef __HIPCC__
#define RUNS_FN __device__ __forceinline__
#else
#define RUNS_FN static inline
#endif

// the first r > i with r == n or proj(keys[r]) != proj(keys[i]); i < n, and equal projections stand together. The end is searched for in
// doubling steps (the probes fall at i + 2^j - 1) and then by bisection: most runs are a few keys long, some thousands, and a walk would leave
// 63 lanes waiting for the longest. No probe is made at or beyond n
template <typename K, typename Proj>
RUNS_FN unsigned long long run_end(const K *keys, unsigned long long n, unsigned long long i, Proj proj) {
  const auto k = proj(keys[i]);
  unsigned long long l = i, step = 1, r = i + 1;               // proj(keys[l]) == k
  while (r < n && proj(keys[r]) == k) { l = r; step <<= 1; r = l + step; }
  if (r > n) r = n;
  while (r - l > 1) { const unsigned long long m = (l + r) >> 1; if (proj(keys[m]) == k) l = m; else r = m; }
  return r;
}
