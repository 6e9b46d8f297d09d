/* map_asan_driver.c — a stand-alone program over the device-free parts of map_host.c (compiled with -DH10X_MAP_NO_DEVICE: no device library is linked) (the RFMSHv1 reader and writer, the name
 * dictionary, the Q / M / -v formatters), built with -fsanitize=address,undefined by `make asan` for tests/test_moshmap_sanitizers.py.
 *   map_asan_driver ref <in.ref> <setMax> <out.ref>   parse and write back: status 0, or 3 with the reader's message on stderr
 *   map_asan_driver dict <n>                          n names through the dictionary (doublings included), dim / max / a checksum of the table
 *   map_asan_driver fmt                               the three formatters over edge values (0 / 0, x / 0)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "h10x_host.h"

int main(int argc, char *argv[]) {
  char err[512];
  if (argc == 5 && !strcmp(argv[1], "ref")) {
    h10x_reffile rf;
    if (h10x_reffile_read(argv[2], (uint32_t)strtoul(argv[3], 0, 10), &rf, err, (int)sizeof err)) { fprintf(stderr, "%s\n", err); return 3; }
    for (uint32_t i = 0; i < (uint32_t)rf.dict->max; ++i) {
      int ip = -1;
      if (!h10x_namedict_find(rf.dict, h10x_namedict_name(rf.dict, i), &ip)) { fprintf(stderr, "name %u is not found through the table\n", i); return 4; }
    }
    printf("max %u names %d lenDim %d lenMax %d dim %d\n", rf.max, rf.dict->max, rf.lenDim, rf.lenMax, rf.dict->dim);
    const int rc = h10x_reffile_write(argv[4], &rf, err, (int)sizeof err);
    if (rc) fprintf(stderr, "%s\n", err);
    h10x_reffile_free(&rf);
    return rc ? 5 : 0;
  }
  if (argc == 3 && !strcmp(argv[1], "dict")) {
    h10x_namedict *d = h10x_namedict_create(1024);
    h10x_reffile lens; memset(&lens, 0, sizeof lens);
    const int n = atoi(argv[2]);
    if (!d) return 2;
    for (int i = 0; i < n; ++i) {
      char name[32]; int ip = -1;
      snprintf(name, sizeof name, "s%d", i);
      if (h10x_namedict_add(d, name, &ip) != 1 || ip != i) return 6;
      if (h10x_namedict_add(d, name, &ip) != 0 || ip != i) return 7;
      if (h10x_reffile_set_len(&lens, (uint32_t)i, (uint32_t)i)) return 8;
    }
    uint64_t sum = 0;
    for (int i = 0; i < d->size; ++i) sum = sum * 1000003u + (uint64_t)d->table[i];
    printf("dim %d max %d table %llx lenDim %d lenMax %d\n", d->dim, d->max, (unsigned long long)sum, lens.lenDim, lens.lenMax);
    h10x_namedict_destroy(d); h10x_reffile_free(&lens);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "fmt")) {
    const uint32_t none[4] = {0, 0, 0, 0}, some[4] = {3, 150, 2, 1};
    const h10x_maprec_t dup = {92, 2947, 341, 437, 0, 96, 0}, flat = {5, 5, 7, 7, 3, 0, 0};
    h10x_map_print_q(stdout, "short", 12, none);
    h10x_map_print_q(stdout, "q", 4000, some);
    h10x_map_print_m(stdout, "dup", 3000, &dup, "chrA", 10592, 13447, 0);
    h10x_map_print_m(stdout, "flat", 100, &flat, "chrB", 1, 1, 3);
    h10x_map_print_seed(stdout, 17, 1, "chrA", 5, "", 0);
    h10x_map_print_seed(stdout, 18, 2, "chrA", 5, "chrB", 6);
    return 0;
  }
  fprintf(stderr, "usage: map_asan_driver ref <in.ref> <setMax> <out.ref> | dict <n> | fmt\n");
  return 1;
}
