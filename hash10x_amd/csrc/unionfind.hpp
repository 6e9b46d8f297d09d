// unionfind.hpp — lock-free union by smaller label, the one text behind stage_m.hip's hook over parent[] in global memory, stage_n.hip's hook
// over a wave's labels in LDS, and the host model of tests/uf_model.cpp (the same loops on std::atomic under ThreadSanitizer: DESIGN.md §17).
//
// lab[v] <= v at all times: a label only ever goes down, by fetch_min. So a find strictly descends, and the larger end of a retried union
// strictly descends: every loop is bounded by n, and nothing waits for another thread.
// A is the policy of the label words: A::word (what lab points to), A::load(p) (a relaxed atomic load) and A::fetch_min(p, v) (a relaxed
// atomic minimum that returns what the word held). The header needs no HIP header: under a plain C++ compiler the caller brings its own policy.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define UF_FN __device__ __forceinline__
#else
#define UF_FN static inline
#endif

// the root of x: at most n steps down (a value out of range would be a corrupted array: the walk stops at it). On the way every visited
// word is lowered to its grandparent (fetch_min: stays inside the set, keeps lab[v] <= v).
template <typename A>
UF_FN uint32_t uf_find(typename A::word *lab, uint32_t x, uint32_t n) {
  for (uint32_t step = 0; step < n; ++step) {
    const uint32_t p = A::load(lab + x);
    if (p >= x) return x;
    const uint32_t g = A::load(lab + p);
    if (g < p) A::fetch_min(lab + x, g);
    x = p;
  }
  return x;
}

// union of the sets of a and b; true if their roots differed. Find both roots; fetch_min the larger root's word towards the smaller. If the
// word no longer held the larger root itself, another thread hooked it first: go on with (what it held, the smaller root).
template <typename A>
UF_FN bool uf_union(typename A::word *lab, uint32_t a, uint32_t b, uint32_t n) {
  bool did = false;
  for (uint32_t t = 0; t < n; ++t) {                          // max(a, b) descends with every retry
    a = uf_find<A>(lab, a, n); b = uf_find<A>(lab, b, n);
    if (a == b) break;
    did = true;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = A::fetch_min(lab + hi, lo);
    if (old == hi) break;                                     // hi was a root, and hangs below lo now
    a = old; b = lo;                                          // hi had been hooked to old < hi meanwhile: old and lo are still to be joined
  }
  return did;
}

#ifdef __HIPCC__
// device words. SCOPE is the scope of the load: agent for an array that other CUs and XCDs rewrite (it bypasses the CU's L1, which no other
// CU's store refreshes), wavefront for LDS words that only the wave's own lanes rewrite. fetch_min is what atomicMin is.
template <int SCOPE>
struct UfDevice {
  typedef uint32_t word;
  static __device__ __forceinline__ uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
  static __device__ __forceinline__ uint32_t fetch_min(uint32_t *p, uint32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
#endif
