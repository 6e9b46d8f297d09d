"""Records tests/golden/crib/NAME.txt.gz: for every case of tests/crib_cases.py the lines of the reference binary's stdout that tests/crib_model.py
restates (crib_model.report), from oracle/_ref/hash10x run on the case's .hash and FASTA files in a temporary directory (the 67 MB FASTA of S3_long
among them). Needs the reference binary. Run: python tests/golden/make_crib_golden.py [case ...]"""
import gzip
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import crib_cases as cc
import crib_model as cm
import orc

OUT = os.path.join(orc.GOLDEN, "crib")


def main(names):
    assert orc.have_ref(), "oracle/_ref/hash10x is not built"
    os.makedirs(OUT, exist_ok=True)
    for name in names or list(cc.CASES):
        with tempfile.TemporaryDirectory() as d:
            files = cc.write_files(name, d)
            r = orc.run_ref(cc.args(name, *files), d)
            assert r.returncode == 0, (name, r.stderr.decode(errors="replace")[-2000:])
            lines = cm.report(r.stdout)
        with open(os.path.join(OUT, name + ".txt.gz"), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(("\n".join(lines) + "\n").encode())                 # (no name, no time: the same text gives the same bytes)
        print("%s: %d lines%s" % (name, len(lines), "" if lines == cc.model_text(name) else "   !! the model's text differs"))


if __name__ == "__main__":
    main(sys.argv[1:])
