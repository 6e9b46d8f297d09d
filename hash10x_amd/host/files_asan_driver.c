/* The writers of files_host.c that have no driver of their own — .mm, .idx, .sg and the whitelist text — behind one main, for the AddressSanitizer + UBSan
   build (tests/test_output_files_cpu.py): they need no device.   files_asan_driver <dir>
   Good files, left in <dir> for the Python readers:
     mm_<n>.mm   n = 0, 1, 65539 records (the writer works in runs of 65536): mol[i] = 7 i + 1, slot[i] = i % 5; 11 blocks, 23 molecules, n / 2 clustered
     idx_<n>.idx n = 0 (0 blocks, 0 molecules) and 7 (3 blocks, 4 molecules): start[m] = 10 m
     sg_<r>.sg   10 blocks in ranges of r = 1, 3, 8192 blocks; the row of block c has c % 3 pairs {block c + 1 + k, count 2 c + k + 1}: blocks 0, 3, 6, 9 are
                 empty, so ranges without rows occur at r = 1 and r = 3; minShare 4
   The whitelist goes through write, read and whitelist_lines with 0, 1 and 70000 codes (the reader starts with room for 65536; the last code repeats the
   first, and the last line wins), and a word of 15 characters is refused. Then every writer fails in three ways — a path that cannot be opened (a missing
   directory, and a name whose .part is too long for the file system), a failing callback where it has one, and a disk that is full after 4096 bytes
   (RLIMIT_FSIZE) — and each time nothing new is left, neither the file nor a .part, and a file that stood at the path keeps its bytes. */
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include "h10x_host.h"

static char err[512];
static int exists(const char *p) { struct stat st; return stat(p, &st) == 0; }
static void put_file(const char *p, const char *text) { FILE *f = fopen(p, "wb"); if (!f || fputs(text, f) < 0 || fclose(f)) { fprintf(stderr, "cannot place %s\n", p); exit(3); } }
static int holds(const char *p, const char *text) { char buf[64] = ""; FILE *f = fopen(p, "rb"); if (!f) return 0; const size_t n = fread(buf, 1, sizeof buf - 1, f); fclose(f); return n == strlen(text) && !memcmp(buf, text, n); }
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "files_asan_driver.c:%d: %s fails (err: %s)\n", __LINE__, #cond, err); exit(10); } } while (0)

/* the share graph above */
typedef struct { uint32_t nBlocks; uint64_t calls, failAt; int bad; uint32_t next; uint64_t *part; uint32_t *blk, *cnt; } Graph;
static int graph_range(void *user, uint32_t c0, uint32_t c1, h10x_share_graph_range *r) {
  Graph *g = (Graph *)user;
  if (g->calls++ == g->failAt) return -1;
  if (c0 != g->next || c1 <= c0 || c1 > g->nBlocks) g->bad = 1;
  g->next = c1;
  free(g->part); free(g->blk); free(g->cnt);
  const size_t n = c1 - c0;
  g->part = (uint64_t *)calloc(n + 1, 8); g->blk = (uint32_t *)calloc(2 * n + 1, 4); g->cnt = (uint32_t *)calloc(2 * n + 1, 4);
  if (!g->part || !g->blk || !g->cnt) return -1;
  uint64_t rows = 0;
  for (uint32_t c = c0; c < c1; ++c) {
    for (uint32_t k = 0; k < c % 3; ++k, ++rows) { g->blk[rows] = c + 1 + k; g->cnt[rows] = 2 * c + k + 1; }
    g->part[c - c0 + 1] = rows;
  }
  r->part = g->part; r->blk = g->blk; r->cnt = g->cnt; r->rows = rows;
  return 0;
}
static void graph_free(Graph *g) { free(g->part); free(g->blk); free(g->cnt); g->part = 0; g->blk = g->cnt = 0; }

/* one call of each writer on a payload of more than 4096 bytes; failAt: the share graph's callback fails in that call */
enum { MM, IDX, SG, WL, N_WRITERS };
static const char *const writerName[N_WRITERS] = {"mm", "idx", "sg", "wl"};
static uint32_t big[70000];
static uint64_t bigStart[1001];
static int write_big(int which, const char *path, uint64_t failAt) {
  if (which == MM) { h10x_molmap_info info = {70000, 35000, 11, 23}; return h10x_host_write_molmap(path, big, big, &info, err, (int)sizeof err); }
  if (which == IDX) return h10x_host_write_split_index(path, bigStart, 400, 600, err, (int)sizeof err);
  if (which == WL) return h10x_host_whitelist_write(path, big, 70000, err, (int)sizeof err);
  Graph g; memset(&g, 0, sizeof g); g.nBlocks = 2000; g.failAt = failAt;
  const int rc = h10x_host_write_share_graph(path, 2000, 4, 300, graph_range, &g, 0, err, (int)sizeof err);
  graph_free(&g);
  return rc;
}
/* path holds "old" before the call: the call must fail with rc, say what it should, and leave path as it was and no .part */
static void fails(int which, const char *path, int placed, uint64_t failAt, int rc, const char *says) {
  char part[1400]; snprintf(part, sizeof part, "%s.part", path);
  if (placed) put_file(path, "old");
  strcpy(err, "untouched");
  CHECK(write_big(which, path, failAt) == rc);
  CHECK(!strncmp(err, says, strlen(says)));
  CHECK(!exists(part));
  CHECK(placed ? holds(path, "old") : !exists(path));
  if (placed) remove(path);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: files_asan_driver <dir>\n"); return 2; }
  const char *dir = argv[1]; char p[1200], part[1300];
  for (uint32_t i = 0; i < 70000; ++i) big[i] = i * 2654435761u;
  for (uint32_t i = 0; i <= 1000; ++i) bigStart[i] = 10ull * i;

  /* ---- the good files ---- */
  const uint64_t mmSizes[3] = {0, 1, (1 << 16) + 3};
  for (int k = 0; k < 3; ++k) {
    const uint64_t n = mmSizes[k];
    uint32_t *mol = (uint32_t *)malloc((n + 1) * 4), *slot = (uint32_t *)malloc((n + 1) * 4);
    CHECK(mol && slot);
    for (uint64_t i = 0; i < n; ++i) { mol[i] = (uint32_t)(7 * i + 1); slot[i] = (uint32_t)(i % 5); }
    h10x_molmap_info info = {n, n / 2, 11, 23};
    snprintf(p, sizeof p, "%s/mm_%llu.mm", dir, (unsigned long long)n); snprintf(part, sizeof part, "%s.part", p);
    CHECK(h10x_host_write_molmap(p, n ? mol : 0, n ? slot : 0, &info, err, (int)sizeof err) == 0 && exists(p) && !exists(part));
    free(mol); free(slot);
  }
  for (int k = 0; k < 2; ++k) {
    const uint32_t nBlocks = k ? 3 : 0, nMol = k ? 4 : 0;
    snprintf(p, sizeof p, "%s/idx_%u.idx", dir, nBlocks + nMol); snprintf(part, sizeof part, "%s.part", p);
    CHECK(h10x_host_write_split_index(p, bigStart, nBlocks, nMol, err, (int)sizeof err) == 0 && exists(p) && !exists(part));
  }
  const uint32_t steps[3] = {1, 3, 8192}; const uint64_t wantCalls[3] = {10, 4, 1};
  for (int k = 0; k < 3; ++k) {
    Graph g; memset(&g, 0, sizeof g); g.nBlocks = 10; g.failAt = UINT64_MAX; uint64_t rows = 0;
    snprintf(p, sizeof p, "%s/sg_%u.sg", dir, steps[k]); snprintf(part, sizeof part, "%s.part", p);
    CHECK(h10x_host_write_share_graph(p, 10, 4, steps[k], graph_range, &g, &rows, err, (int)sizeof err) == 0 && exists(p) && !exists(part));
    CHECK(!g.bad && g.next == 10 && g.calls == wantCalls[k] && rows == 9);
    graph_free(&g);
  }
  { Graph g; memset(&g, 0, sizeof g); g.failAt = UINT64_MAX; uint64_t rows = 1;                     /* no blocks at all: a header and one offset */
    snprintf(p, sizeof p, "%s/sg_none.sg", dir);
    CHECK(h10x_host_write_share_graph(p, 0, 4, 0, graph_range, &g, &rows, err, (int)sizeof err) == 0 && !g.calls && rows == 0); }

  /* ---- the whitelist: write, read, look up ---- */
  const uint64_t wlSizes[3] = {0, 1, 70000};
  snprintf(p, sizeof p, "%s/wl.txt", dir); snprintf(part, sizeof part, "%s.part", p);
  for (int k = 0; k < 3; ++k) {
    const uint64_t n = wlSizes[k];
    if (n > 1) big[n - 1] = big[0];                                                                  /* a barcode on two lines */
    uint32_t *back = 0; uint64_t nBack = 0;
    CHECK(h10x_host_whitelist_write(p, big, n, err, (int)sizeof err) == 0 && exists(p) && !exists(part));
    CHECK(h10x_host_whitelist_read(p, &back, &nBack, err, (int)sizeof err) == 0 && nBack == n && (!n || !memcmp(back, big, n * 4)));
    const uint32_t query[3] = {big[0], big[1], 0x12345678u}; uint32_t lines[3] = {9, 9, 9};        /* (0x12345678 is none of i * 2654435761 below 70000) */
    CHECK(h10x_host_whitelist_lines(back, nBack, query, 3, lines) == 0);
    CHECK(lines[0] == (uint32_t)n && lines[1] == (n > 1 ? 2u : 0u) && lines[2] == 0);
    h10x_host_whitelist_free(back);
  }
  big[69999] = 69999u * 2654435761u;
  { uint32_t *back = 0; uint64_t nBack = 0;
    put_file(p, "ACGTACGTACGTACGT\nACGTACGTACGTACG\n");
    CHECK(h10x_host_whitelist_read(p, &back, &nBack, err, (int)sizeof err) == -1 && !back && !strncmp(err, "bad barcode line 2 in ", 22) && strstr(err, ": ACGTACGTACGTACG"));
    remove(p); }

  /* ---- the failures ---- */
  struct rlimit keep, small; CHECK(getrlimit(RLIMIT_FSIZE, &keep) == 0);
  signal(SIGXFSZ, SIG_IGN);
  for (int w = 0; w < N_WRITERS; ++w) {
    snprintf(p, sizeof p, "%s/missing/x.%s", dir, writerName[w]);
    fails(w, p, 0, UINT64_MAX, -1, "failed to open output file");
    char name[256]; memset(name, 'n', 252); name[252] = 0;                                           /* 252 characters fit a file name, 5 more do not */
    snprintf(p, sizeof p, "%s/%s", dir, name);
    fails(w, p, 1, UINT64_MAX, -1, "failed to open output file");
    snprintf(p, sizeof p, "%s/fail.%s", dir, writerName[w]);
    if (w == SG) { fails(w, p, 1, 0, -2, "untouched"); fails(w, p, 1, 3, -2, "untouched"); }
    small = keep; small.rlim_cur = 4096;                                                             /* (the 3 bytes placed beforehand fit under it) */
    CHECK(setrlimit(RLIMIT_FSIZE, &small) == 0);
    fails(w, p, 0, UINT64_MAX, -1, "failed to write");
    fails(w, p, 1, UINT64_MAX, -1, "failed to write");
    CHECK(setrlimit(RLIMIT_FSIZE, &keep) == 0);
  }
  printf("4 writers, 3 failures each: nothing left behind\n");
  return 0;
}
