// the host model of the lock-free union by smaller label. It includes hash10x_amd/csrc/unionfind.hpp, the text the kernels of
// stage_m.hip and stage_n.hip run, with a std::atomic policy, and runs it with 16 threads against a sequential union-find over random graphs,
// permuted chains and stars: ONE pass over the edges must give the same roots, and a second pass must find nothing left to do.
//   g++ -O1 -g -fsanitize=thread -std=c++17 -pthread tests/uf_model.cpp -o uf_model && ./uf_model [trials]
#include "../hash10x_amd/csrc/unionfind.hpp"
#include <atomic>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <algorithm>
typedef uint32_t u32;
struct HostWords {
  typedef std::atomic<u32> word;
  static u32 load(const word *p) { return p->load(std::memory_order_relaxed); }
  static u32 fetch_min(word *p, u32 v) { u32 o = p->load(std::memory_order_relaxed); while (o > v && !p->compare_exchange_weak(o, v, std::memory_order_relaxed)) {} return o; }
};
int main(int argc, char **argv) {
  const int trials = argc > 1 ? atoi(argv[1]) : 60, T = 16;
  std::mt19937 rng(5);
  for (int trial = 0; trial < trials; ++trial) {
    u32 nB = 50 + rng() % 3000; u32 nE = rng() % (2 * nB);
    std::vector<std::pair<u32,u32>> E;
    int kind = trial % 3;
    if (kind == 0) for (u32 i = 0; i < nE; ++i) E.push_back({1 + rng() % (nB - 1), 1 + rng() % (nB - 1)});
    else if (kind == 1) { std::vector<u32> perm(nB - 1); for (u32 i = 0; i < nB - 1; ++i) perm[i] = i + 1; std::shuffle(perm.begin(), perm.end(), rng); for (u32 i = 0; i + 1 < nB - 1; ++i) E.push_back({perm[i], perm[i + 1]}); }
    else { u32 hub = 1 + rng() % (nB - 1); for (u32 i = 1; i < nB; ++i) if (i != hub) E.push_back({hub, i}); }
    std::shuffle(E.begin(), E.end(), rng);
    std::vector<std::atomic<u32>> par(nB); for (u32 i = 0; i < nB; ++i) par[i] = i;
    std::atomic<u32> joined{0};
    auto pass = [&] {
      std::vector<std::thread> th;
      for (int t = 0; t < T; ++t) th.emplace_back([&, t] { for (size_t i = t; i < E.size(); i += T) if (uf_union<HostWords>(par.data(), E[i].first, E[i].second, nB)) joined.fetch_add(1, std::memory_order_relaxed); });
      for (auto &x : th) x.join();
    };
    pass();
    std::vector<u32> ref(nB); for (u32 i = 0; i < nB; ++i) ref[i] = i;
    auto rf = [&](u32 x) { while (ref[x] != x) x = ref[x] = ref[ref[x]]; return x; };
    for (auto &e : E) { u32 a = rf(e.first), b = rf(e.second); if (a != b) ref[std::max(a, b)] = std::min(a, b); }
    for (u32 i = 0; i < nB; ++i) { if (uf_find<HostWords>(par.data(), i, nB) != rf(i)) { printf("MISMATCH trial %d block %u\n", trial, i); return 1; } if (par[i] > i) { printf("parent above\n"); return 1; } }
    // the second pass over the same edges: every union finds its ends in one set. Every word holds its root by now (the finds above went up
    // the blocks in order: the word below a block held its root already, so the block's word was lowered to it), so no find lowers one either
    std::vector<u32> before(nB); for (u32 i = 0; i < nB; ++i) before[i] = par[i];
    joined = 0; pass();
    if (joined) { printf("SECOND PASS trial %d: %u unions of different roots\n", trial, joined.load()); return 1; }
    for (u32 i = 0; i < nB; ++i) if (par[i] != before[i]) { printf("SECOND PASS trial %d: word %u changed\n", trial, i); return 1; }
  }
  printf("ok\n");
}
