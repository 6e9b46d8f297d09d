# oracle/ref_moshutils.mk — the reference's moshutils into oracle/_ref/, beside the binaries oracle/Makefile's `ref` makes.
#   make -C oracle -f ref_moshutils.mk
# TEST INFRASTRUCTURE ONLY (tests/test_write_mosh_gpu.py reads a --writeMosh file back with it). Compiled from the reference's own sources
# where they lie, never copied here; without them a prebuilt oracle/_ref/moshutils is used if there is one.

REF      ?= /root/reference
CC       ?= gcc
MU_SRCS   = moshutils.c seqio.c seqhash.c moshset.c hash.c dict.c array.c utils.c
MU_PATHS  = $(addprefix $(REF)/,$(MU_SRCS))

ref:
	@if [ -d $(REF) ]; then $(MAKE) --no-print-directory -f ref_moshutils.mk _ref/moshutils; \
	 else echo "oracle: $(REF) absent - using prebuilt oracle/_ref/moshutils if any"; fi

_ref/moshutils: $(MU_PATHS)
	@mkdir -p _ref
	$(CC) -O2 -w $(MU_PATHS) -o $@ -lz -lm

.PHONY: ref
