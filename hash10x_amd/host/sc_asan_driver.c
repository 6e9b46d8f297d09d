/* The .sc writer of files_host.c (h10x_host_write_share_components) behind a main of its own, for the AddressSanitizer + UBSan build
   (tests/test_share_components_asan.py): it needs no device.   sc_asan_driver <out.sc> <nBlocks>
   Writes the components of a chain 1 - 2, 3 - 4, ... (blocks 1 .. nBlocks-1 in pairs, a last odd one alone), then tries a path that cannot be opened and a
   disk that is full after 4096 bytes (RLIMIT_FSIZE, 5000 blocks in no component): each fails with -1 and its message, leaves no .part, and a file that
   stood at the path keeps its bytes. */
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include "h10x_host.h"

static int exists(const char *p) { struct stat st; return stat(p, &st) == 0; }
static int holds_old(const char *p) { char b[8] = ""; FILE *f = fopen(p, "rb"); if (!f) return 0; const size_t n = fread(b, 1, sizeof b, f); fclose(f); return n == 3 && !memcmp(b, "old", 3); }

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: sc_asan_driver <out.sc> <nBlocks>\n"); return 2; }
  const uint32_t nBlocks = (uint32_t)atoi(argv[2]), members = nBlocks ? nBlocks - 1 : 0, nComp = (members + 1) / 2;
  h10x_share_components_info info; memset(&info, 0, sizeof info);
  info.nBlocks = nBlocks; info.minShare = 5; info.nComponents = nComp; info.largest = members >= 2 ? 2 : members; info.rows = 2ull * (members / 2);
  info.singletons = members & 1;
  uint32_t *comp = (uint32_t *)calloc(nBlocks ? nBlocks : 1, 4), *rootOf = (uint32_t *)calloc((size_t)nComp + 1, 4), *blocks = (uint32_t *)calloc((size_t)nComp + 1, 4);
  uint64_t *records = (uint64_t *)calloc((size_t)nComp + 1, 8);
  if (!comp || !rootOf || !blocks || !records) return 3;
  for (uint32_t c = 1; c < nBlocks; ++c) {
    const uint32_t k = (c + 1) / 2;
    comp[c] = k; if (c & 1) rootOf[k] = c; blocks[k] += 1; records[k] += 1000ull * c;
  }
  char err[256] = "";
  int rc = h10x_host_write_share_components(argv[1], &info, comp, rootOf, blocks, records, err, (int)sizeof err);
  if (rc) { fprintf(stderr, "%s\n", err); rc = 4; }
  if (!rc) {
    char bad[1200]; snprintf(bad, sizeof bad, "%s.dir/does/not/exist.sc", argv[1]);
    char badPart[1300]; snprintf(badPart, sizeof badPart, "%s.part", bad);
    if (h10x_host_write_share_components(bad, &info, comp, rootOf, blocks, records, err, (int)sizeof err) != -1 || strncmp(err, "failed to open output file", 26) ||
        exists(bad) || exists(badPart)) rc = 5;
    else printf("%s\n", err);
  }
  if (!rc) {                                                  /* a name whose .part is too long for the file system cannot be opened either; then the full disk */
    char name[256], dir[1200], at[1500], atPart[1600]; memset(name, 'n', 252); name[252] = 0;
    snprintf(dir, sizeof dir, "%s", argv[1]); char *slash = strrchr(dir, '/'); if (slash) slash[1] = 0; else dir[0] = 0;
    snprintf(at, sizeof at, "%s%s", dir, name); snprintf(atPart, sizeof atPart, "%s.part", at);
    FILE *f = fopen(at, "wb"); if (!f || fputs("old", f) < 0 || fclose(f)) rc = 3;
    if (!rc && (h10x_host_write_share_components(at, &info, comp, rootOf, blocks, records, err, (int)sizeof err) != -1 || strncmp(err, "failed to open output file", 26) ||
                !holds_old(at) || exists(atPart))) rc = 6;
    remove(at);
    h10x_share_components_info big; memset(&big, 0, sizeof big); big.nBlocks = 5000; big.minShare = 5;
    uint32_t *none = (uint32_t *)calloc(5000, 4);
    snprintf(at, sizeof at, "%s.full", argv[1]); snprintf(atPart, sizeof atPart, "%s.part", at);
    f = fopen(at, "wb"); if (!none || !f || fputs("old", f) < 0 || fclose(f)) rc = 3;
    struct rlimit keep, small;
    if (!rc && !getrlimit(RLIMIT_FSIZE, &keep)) {
      signal(SIGXFSZ, SIG_IGN);
      small = keep; small.rlim_cur = 4096; setrlimit(RLIMIT_FSIZE, &small);
      const int w = h10x_host_write_share_components(at, &big, none, rootOf, blocks, records, err, (int)sizeof err);
      setrlimit(RLIMIT_FSIZE, &keep);
      if (w != -1 || strncmp(err, "failed to write", 15) || !holds_old(at) || exists(atPart)) rc = 7;
    } else if (!rc) rc = 3;
    remove(at); free(none);
  }
  free(comp); free(rootOf); free(blocks); free(records);
  return rc;
}
