"""Records tests/golden/fixfqb/ from the reference's fq2b (oracle/_ref/fq2b, where the reference is present): 600 read pairs, the
raw .fqb (no whitelist), the goodcodes of the barcodes present at least 3 times (ascending by packed word), and what
`fq2b -10x goodcodes` makes of the reads: fixed.fqb and its stderr. Run: python tests/golden/make_fixfqb_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fqb_model as fm

T = 3


def main():
    d = fm.GOLDEN
    os.makedirs(d, exist_ok=True)
    fm.write_fastq_pairs(d, 600, 7, n_codes=30)
    raw, _ = fm.run_fq2b_ref(d, "raw.fqb")
    good = fm.census(np.frombuffer(raw, dtype=np.uint32), T)[2]
    with open(os.path.join(d, "goodcodes.txt"), "w") as f:
        f.write(fm.text(good))
    _, err = fm.run_fq2b_ref(d, "fixed.fqb", "goodcodes.txt")
    with open(os.path.join(d, "fixed.stderr.txt"), "wb") as f:
        f.write(err)
    print("%d records, %d good barcodes, stderr:\n%s" % (len(raw) // 120, good.size, err.decode()))


if __name__ == "__main__":
    main()
