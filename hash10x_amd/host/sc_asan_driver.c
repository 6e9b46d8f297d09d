/* The .sc writer of h10x_host.c (h10x_host_write_share_components) behind a main of its own, for the AddressSanitizer + UBSan build
   (tests/test_share_components_asan.py): it needs no device.   sc_asan_driver <out.sc> <nBlocks>
   Writes the components of a chain 1 - 2, 3 - 4, ... (blocks 1 .. nBlocks-1 in pairs, a last odd one alone), then tries a path that cannot be opened. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h10x_host.h"

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
    if (!h10x_host_write_share_components(bad, &info, comp, rootOf, blocks, records, err, (int)sizeof err) || strncmp(err, "failed to open output file", 26)) rc = 5;
    else printf("%s\n", err);
  }
  free(comp); free(rootOf); free(blocks); free(records);
  return rc;
}
