/* The .sl writer of files_host.c (h10x_host_write_seq_links) behind a main of its own, for the AddressSanitizer + UBSan build
   (tests/test_seq_links_cpu.py): it needs no device.   sl_asan_driver <out.sl> <nSeq> <linksPerPiece>
   Sequence q is called "s<q>", has q % 5 + 1 bases, q % 4 head rows and q % 3 tail rows. End e has e % 3 links, to ends e + 2 + k (k < e % 3) where those
   exist, with shared = e + k + 1. The links come in pieces of linksPerPiece (0: the writer's default). Then the callback fails in its last piece, and a
   path that cannot be opened is tried: neither may leave a .part behind. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include "h10x_host.h"

typedef struct { const uint32_t *other, *shared; uint64_t links, calls, failAt; } Feed;

static int feed(void *user, uint64_t first, uint64_t count, uint32_t *other, uint32_t *shared) {
  Feed *f = (Feed *)user;
  if (f->calls == f->failAt) return -1;
  if (first + count > f->links) return -1;
  memcpy(other, f->other + first, (size_t)count * 4); memcpy(shared, f->shared + first, (size_t)count * 4);
  ++f->calls;
  return 0;
}

static int exists(const char *p) { struct stat st; return stat(p, &st) == 0; }

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: sl_asan_driver <out.sl> <nSeq> <linksPerPiece>\n"); return 2; }
  const uint64_t n = strtoull(argv[2], 0, 10), per = strtoull(argv[3], 0, 10), nEnds = 2 * n;
  char err[256] = "", part[1200]; snprintf(part, sizeof part, "%s.part", argv[1]);
  h10x_seq_links_rec *table = (h10x_seq_links_rec *)calloc(n + 1, sizeof *table);
  uint64_t *offsets = (uint64_t *)calloc(nEnds + 1, 8), *nameOff = (uint64_t *)calloc(n + 1, 8);
  uint32_t *other = (uint32_t *)calloc(2 * nEnds + 1, 4), *shared = (uint32_t *)calloc(2 * nEnds + 1, 4);
  char *names = (char *)calloc(n + 1, 24);
  if (!table || !offsets || !nameOff || !other || !shared || !names) return 3;
  uint64_t links = 0, nameAt = 0;
  for (uint64_t q = 0; q < n; ++q) {
    table[q].len = q % 5 + 1; table[q].headRows = (uint32_t)(q % 4); table[q].tailRows = (uint32_t)(q % 3);
    nameOff[q] = nameAt; nameAt += (uint64_t)snprintf(names + nameAt, 24, "s%llu", (unsigned long long)q) + 1;
  }
  nameOff[n] = nameAt;
  for (uint64_t e = 0; e < nEnds; ++e) {
    for (uint64_t k = 0; k < e % 3; ++k)
      if (e + 2 + k < nEnds) { other[links] = (uint32_t)(e + 2 + k); shared[links] = (uint32_t)(e + k + 1); ++links; }
    offsets[e + 1] = links;
  }
  h10x_seq_links_head head = {1000000, 3, 2, 2500, 8, n, links, 5, table, offsets, names, nameOff};
  h10x_seq_links_totals t;
  Feed f = {other, shared, links, 0, UINT64_MAX};
  int rc = h10x_host_write_seq_links(argv[1], &head, feed, &f, per, 0, &t, err, (int)sizeof err);
  if (rc) { fprintf(stderr, "%s\n", err); return 4; }
  if (t.nSeq != n || t.links != links || t.pieces != f.calls || exists(part) || !exists(argv[1])) { fprintf(stderr, "the pieces do not tile the %llu links\n", (unsigned long long)links); return 5; }
  printf("%llu pieces, %llu links, %llu with links, max shared %u\n", (unsigned long long)f.calls, (unsigned long long)t.links, (unsigned long long)t.withLinks, t.maxShared);
  if (links) {                                                /* a failing callback: -2, err untouched, nothing left behind */
    char fl[1200], flPart[1300]; snprintf(fl, sizeof fl, "%s.fail", argv[1]); snprintf(flPart, sizeof flPart, "%s.part", fl);
    Feed g = {other, shared, links, 0, f.calls - 1};
    strcpy(err, "untouched");
    rc = h10x_host_write_seq_links(fl, &head, feed, &g, per, 0, &t, err, (int)sizeof err);
    if (rc != -2 || strcmp(err, "untouched") || exists(fl) || exists(flPart)) return 6;
  }
  char bad[1200]; snprintf(bad, sizeof bad, "%s.dir/does/not/exist.sl", argv[1]);
  Feed h = {other, shared, links, 0, UINT64_MAX};
  rc = h10x_host_write_seq_links(bad, &head, feed, &h, per, 0, &t, err, (int)sizeof err);
  if (rc != -1 || strncmp(err, "failed to open output file", 26) || h.calls) return 7;
  printf("%s\n", err);
  free(table); free(offsets); free(nameOff); free(other); free(shared); free(names);
  return 0;
}
