/* files_host.h — internal to libh10x_host.so: what h10x_host.c uses of files_host.c beside the writers that h10x_host.h declares. Not part of the API
   that Python or the command-line programs see (the symbols are hidden in the shared library). */
#ifndef H10X_FILES_HOST_H
#define H10X_FILES_HOST_H
#include "h10x_host.h"
#define H10X_INTERNAL __attribute__((visibility("hidden")))

/* One output file. The bytes go to <path>.part, which takes the file's name when it is whole: a run that fails leaves neither the file nor a .part,
   and a file that stood at the path before keeps its bytes. err (may be NULL) gets "failed to open output file <path>" / "failed to write <path>".
   Start from a zeroed struct, or from open / probe: then abort is always safe, also after commit. */
typedef struct { FILE *f; char *tmp; const char *path; char *err; int errlen; } OutFile;
H10X_INTERNAL int  h10x_out_open(OutFile *o, const char *path, char *err, int errlen);
H10X_INTERNAL int  h10x_out_probe(OutFile *o, const char *path, char *err, int errlen);   /* open and close: the path is known to be writable before long work, and
                                                                                             a writer that takes a path (not an OutFile) may fill o->tmp; commit or abort ends it */
H10X_INTERNAL int  h10x_out_write(OutFile *o, const void *p, size_t size, size_t n);
H10X_INTERNAL int  h10x_out_rewrite(OutFile *o, const void *p, size_t n);                 /* the first n bytes again (headers filled in at the end) */
H10X_INTERNAL int  h10x_out_commit(OutFile *o);                                           /* close, rename; a failure aborts */
H10X_INTERNAL void h10x_out_abort(OutFile *o);                                            /* close, remove the .part */

/* room for `need` elements of `elt` bytes in a malloc'ed array that doubles */
H10X_INTERNAL int  h10x_grow(void **p, size_t *cap, size_t need, size_t elt);
/* the names of sequences 0 .. n-1 back to back, NUL-terminated: sequence q is called bytes + off[q], off[n] = nBytes (off is NULL until the first add) */
typedef struct { char *bytes; uint64_t *off; uint64_t n, nBytes; size_t capBytes, capOff; } NameTable;
H10X_INTERNAL int  h10x_names_add(NameTable *t, const char *name);                        /* -1 without memory */
H10X_INTERNAL void h10x_names_free(NameTable *t);

H10X_INTERNAL extern const char *const cribTypeName[5];                                   /* hash10x.c:417 */
#endif
