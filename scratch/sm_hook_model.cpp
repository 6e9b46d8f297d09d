// a host model of stage_m.hip's find and hook, the same loops on std::atomic with 16 threads, against a sequential union-find, over
// random graphs, permuted chains and stars; ONE pass over the edges must give the same roots.
//   g++ -O1 -g -fsanitize=thread -std=c++17 -pthread scratch/sm_hook_model.cpp -o scratch/bin/sm_hook_model && scratch/bin/sm_hook_model
#include <atomic>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdint>
#include <random>
#include <algorithm>
typedef uint32_t u32;
static std::vector<std::atomic<u32>> *P;
static u32 fmin_(u32 i, u32 v) { auto &a = (*P)[i]; u32 o = a.load(std::memory_order_relaxed); while (o > v && !a.compare_exchange_weak(o, v, std::memory_order_relaxed)) {} return o; }
static u32 find(u32 x, u32 nB) {
  for (u32 s = 0; s < nB; ++s) { u32 p = (*P)[x].load(std::memory_order_relaxed); if (p >= x) return x; u32 g = (*P)[p].load(std::memory_order_relaxed); if (g < p) fmin_(x, g); x = p; }
  return x;
}
static void hook(u32 a, u32 b, u32 nB) {
  for (u32 t = 0; t < nB; ++t) { a = find(a, nB); b = find(b, nB); if (a == b) break; u32 hi = std::max(a, b), lo = std::min(a, b); u32 old = fmin_(hi, lo); if (old == hi) break; a = old; b = lo; }
}
int main() {
  std::mt19937 rng(5);
  for (int trial = 0; trial < 300; ++trial) {
    u32 nB = 50 + rng() % 3000; u32 nE = rng() % (2 * nB);
    std::vector<std::pair<u32,u32>> E;
    int kind = trial % 3;
    if (kind == 0) for (u32 i = 0; i < nE; ++i) E.push_back({1 + rng() % (nB - 1), 1 + rng() % (nB - 1)});
    else if (kind == 1) { std::vector<u32> perm(nB - 1); for (u32 i = 0; i < nB - 1; ++i) perm[i] = i + 1; std::shuffle(perm.begin(), perm.end(), rng); for (u32 i = 0; i + 1 < nB - 1; ++i) E.push_back({perm[i], perm[i + 1]}); }
    else { u32 hub = 1 + rng() % (nB - 1); for (u32 i = 1; i < nB; ++i) if (i != hub) E.push_back({hub, i}); }
    std::shuffle(E.begin(), E.end(), rng);
    std::vector<std::atomic<u32>> par(nB); for (u32 i = 0; i < nB; ++i) par[i] = i; P = &par;
    const int T = 16; std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back([&, t] { for (size_t i = t; i < E.size(); i += T) hook(E[i].first, E[i].second, nB); });
    for (auto &x : th) x.join();
    std::vector<u32> ref(nB); for (u32 i = 0; i < nB; ++i) ref[i] = i;
    auto rf = [&](u32 x) { while (ref[x] != x) x = ref[x] = ref[ref[x]]; return x; };
    for (auto &e : E) { u32 a = rf(e.first), b = rf(e.second); if (a != b) ref[std::max(a, b)] = std::min(a, b); }
    for (u32 i = 0; i < nB; ++i) { if (find(i, nB) != rf(i)) { printf("MISMATCH trial %d block %u\n", trial, i); return 1; } if (par[i] > i) { printf("parent above\n"); return 1; } }
  }
  printf("ok\n");
}
