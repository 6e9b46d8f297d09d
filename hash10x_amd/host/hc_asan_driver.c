/* The .hc writer of files_host.c (h10x_host_write_hash_copies) behind a main of its own, for the AddressSanitizer + UBSan build
   (tests/test_hash_copies_cpu.py): it needs no device.   hc_asan_driver <out.hc> <hashNumber> <slabHashes>
   Writes a table whose record x is {x % 7, x % 3, x % 5, x % 2} (index 0 all zero) in slabs of slabHashes (0: the default), checks that the
   slabs asked for tile [0, hashNumber) in order, then lets the callback fail, and tries a path that cannot be opened: neither may leave a file or a
   .part behind. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include "h10x_host.h"

typedef struct { uint64_t next, calls, cap, failAt; int bad; } Feed;

static int feed(void *user, uint16_t *out, uint64_t first, uint64_t count) {
  Feed *f = (Feed *)user;
  if (f->calls == f->failAt) return -1;
  if (first != f->next || !count || (f->cap && count > f->cap)) f->bad = 1;
  for (uint64_t i = 0; i < count; ++i) {
    const uint64_t x = first + i;
    out[4 * i] = (uint16_t)(x % 7); out[4 * i + 1] = (uint16_t)(x % 3); out[4 * i + 2] = (uint16_t)(x % 5); out[4 * i + 3] = (uint16_t)(x % 2);
  }
  f->next = first + count; ++f->calls;
  return 0;
}

static int exists(const char *p) { struct stat st; return stat(p, &st) == 0; }

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: hc_asan_driver <out.hc> <hashNumber> <slabHashes>\n"); return 2; }
  const uint32_t n = (uint32_t)strtoul(argv[2], 0, 10); const uint64_t slab = strtoull(argv[3], 0, 10);
  h10x_hash_copies_info info; memset(&info, 0, sizeof info);
  info.hashNumber = n; info.minShare = 5; info.inRange = n ? n - 1 : 0; info.rows = 3ull * n;
  char err[256] = "";
  Feed f = {0, 0, slab, UINT64_MAX, 0};
  int rc = h10x_host_write_hash_copies(argv[1], &info, feed, &f, slab, err, (int)sizeof err);
  if (rc) { fprintf(stderr, "%s\n", err); return 4; }
  if (f.bad || f.next != n) { fprintf(stderr, "the slabs do not tile the %u hashes\n", n); return 5; }
  printf("%llu slabs\n", (unsigned long long)f.calls);
  if (n) {                                                    /* a failing callback: -2, err untouched, nothing left behind */
    char other[1200], otherPart[1300]; snprintf(other, sizeof other, "%s.fail", argv[1]); snprintf(otherPart, sizeof otherPart, "%s.part", other);
    Feed g = {0, 0, slab, f.calls - 1, 0};
    strcpy(err, "untouched");
    if (h10x_host_write_hash_copies(other, &info, feed, &g, slab, err, (int)sizeof err) != -2 || strcmp(err, "untouched") || exists(other) || exists(otherPart)) return 6;
  }
  char bad[1200]; snprintf(bad, sizeof bad, "%s.dir/does/not/exist.hc", argv[1]);
  Feed h = {0, 0, slab, UINT64_MAX, 0};
  if (h10x_host_write_hash_copies(bad, &info, feed, &h, slab, err, (int)sizeof err) != -1 || strncmp(err, "failed to open output file", 26)) return 7;
  printf("%s\n", err);
  return 0;
}
