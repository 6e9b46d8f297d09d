#!/usr/bin/env python3
"""Regenerates tests/golden/mosh/: inputs from fixed seeds, and what the REFERENCE's moshutils makes of them.

    python tests/golden/make_mosh_golden.py /path/to/reference

The reference's moshutils is compiled into a temporary directory outside the tree and run there with MALLOC_PERTURB_=255;
only data comes back: the inputs (gzipped), every output file (gzipped), and tests/golden/mosh_manifest.json with the command lines, the
exit status, the stdout / stderr lines (resource figures masked) and the sha256 of each output (for .mosh files after
zeroing the 8 bytes of value[0], which are uninitialised heap in a set the reference created). No reference source or
binary is copied."""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mosh_model as mm  # noqa: E402

OUT = os.path.join(HERE, "mosh")
SRC = "moshutils.c seqio.c seqhash.c moshset.c hash.c dict.c array.c utils.c".split()


def fasta(name, seq, width):
    return ">%s\n" % name + "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


def make_inputs():
    rs = np.random.RandomState(20181106)
    B = np.array(list("ACGT"))
    files = {}
    # g.fa: 4 x 50 kb, multi-line, one N run, one sequence a mutated copy of another (shared moshes, depth 2)
    chroms = ["".join(B[rs.randint(0, 4, 50000)]) for _ in range(3)]
    c3 = list(chroms[0])
    for p in rs.choice(50000, 600, replace=False):
        c3[p] = "ACGT"[rs.randint(0, 4)]
    chroms.append("".join(c3))
    chroms[1] = chroms[1][:20000] + "N" * 137 + chroms[1][20137:]
    files["g.fa"] = "".join(fasta("chr%d some description" % (i + 1), s, 60 + 10 * i) for i, s in enumerate(chroms))
    # r.fq: 3000 reads of 10..299 bases drawn from g with errors, either strand, constant quality
    comp = str.maketrans("ACGTN", "TGCAN")
    recs = []
    for i in range(3000):
        ln = int(rs.randint(10, 300)); c = int(rs.randint(0, 4)); p = int(rs.randint(0, 50000 - ln))
        s = list(chroms[c][p:p + ln])
        for q in np.nonzero(rs.rand(ln) < 0.01)[0]:
            s[q] = "ACGT"[rs.randint(0, 4)]
        s = "".join(s)
        if rs.rand() < 0.5:
            s = s.translate(comp)[::-1]
        recs.append("@r%d\n%s\n+\n%s\n" % (i, s, "I" * ln))
    files["r.fq"] = "".join(recs)
    # rep.fa: 66 000 copies of one 90-base sequence (depth saturates at 65535)
    import orc
    o = orc.Oracle(19, 31, 17, 20)
    while True:                                               # ... with exactly one mosh: the histogram is the single line DP 65535 1
        one = "".join(B[rs.randint(0, 4, 90)])
        if len(o.mosh(np.array(["ACGT".index(c) for c in one], np.uint8))[0]) == 1:
            break
    files["rep.fa"] = "".join(">c%d\n%s\n" % (i, one) for i in range(66000))
    # x.fq: interleaved 10x pairs of 23..150 bases, mixed case, N
    recs = []
    for i in range(1200):
        ln = int(rs.randint(23, 151)); c = int(rs.randint(0, 4)); p = int(rs.randint(0, 50000 - ln))
        s = list(chroms[c][p:p + ln])
        for q in np.nonzero(rs.rand(ln) < 0.02)[0]:
            s[q] = "N"
        for q in np.nonzero(rs.rand(ln) < 0.3)[0]:
            s[q] = s[q].lower()
        recs.append("@x%d/%d\n%s\n+\n%s\n" % (i // 2, i % 2 + 1, "".join(s), "F" * ln))
    files["x.fq"] = "".join(recs)
    # parser cases
    small = chroms[2][:6000]
    iu = list(small)
    for q in rs.choice(6000, 300, replace=False):
        iu[q] = "RYKMSWBDHVN-*.ryn"[rs.randint(0, 17)]
    files["iupac.fa"] = fasta("iu the description\twith a tab", "".join(iu), 70) + fasta("second", small[1000:3000].lower(), 50)
    files["nonl.fa"] = fasta("a", small[:2000], 80) + fasta("b", small[2000:4000], 80) + ">c\n" + small[4000:4500] + "\n" + small[4500:5000]
    files["crlf.fa"] = (fasta("a desc", small[:3000], 64) + fasta("b", small[3000:], 64)).replace("\n", "\r\n")
    return {k: v.encode() for k, v in files.items()}


C = ["-c", "20", "19", "31", "17"]
CASES = [
    ("build", C + "-a g.fa -w g.mosh -a r.fq -w gr.mosh -H gr.his -p 2 0 -s 2 3 5 -w p.mosh -d p.dep g.mosh".split(), []),
    ("saturation", C + "-a rep.fa -H rep.his".split(), []),
    ("reads", C + "-a r.fq -w r.mosh -s 2 4 8 -w rc.mosh".split(), []),
    ("merge", C + "-m g.mosh -m r.mosh -s 1 4 8 -w m1.mosh -m rc.mosh -sM 9 -w m2.mosh".split(), ["build/g.mosh", "reads/r.mosh", "reads/rc.mosh"]),
    ("tenx", "-c 20 19 7 17 -x x.fq -w x.mosh".split(), []),
    ("iupac", C + "-a iupac.fa -w iupac.mosh".split(), []),
    ("nonl", C + "-a nonl.fa -w nonl.mosh".split(), []),
    ("crlf", C + "-a crlf.fa -w crlf.mosh".split(), []),
    ("gzip", C + "-a g.fa.gz -w ggz.mosh".split(), []),
    ("defaults_k", "-c 20 16 -a g.fa -w k16.mosh".split(), []),
    ("incompatible", "-c 20 19 31 18 -m g.mosh -w empty18.mosh".split(), ["build/g.mosh"]),
    ("output_file", C + "-o out.txt -a g.fa -H g.his -o - -sM 2".split(), []),
    ("full_add", "-r g.mosh -a r.fq".split(), ["build/g.mosh"]),
    ("full_merge", "-r g.mosh -m r.mosh".split(), ["build/g.mosh", "reads/r.mosh"]),
    ("union", C + "-m g.mosh -m r.mosh -w union.mosh".split(), ["build/g.mosh", "reads/r.mosh"]),
]
INPUT_NAMES = ("g.fa", "g.fa.gz", "r.fq", "rep.fa", "x.fq", "iupac.fa", "nonl.fa", "crlf.fa")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    tmp = tempfile.mkdtemp(prefix="moshgold_")
    try:
        exe = os.path.join(tmp, "moshutils")
        subprocess.run(["gcc", "-O2", "-w", "-o", exe] + [os.path.join(ref, s) for s in SRC] + ["-lz", "-lm"], check=True)
        inputs = make_inputs()
        if os.path.isdir(OUT):
            shutil.rmtree(OUT)
        os.makedirs(os.path.join(OUT, "in"))
        for name, data in inputs.items():
            with open(os.path.join(OUT, "in", name + ".gz"), "wb") as f:
                f.write(gzip.compress(data, 9, mtime=0))
        manifest = {"inputs": sorted(inputs), "cases": []}
        produced = {}
        for name, args, needs in CASES:
            d = os.path.join(tmp, name)
            os.makedirs(d)
            for n, data in inputs.items():
                with open(os.path.join(d, n), "wb") as f:
                    f.write(data)
            with open(os.path.join(d, "g.fa.gz"), "wb") as f:
                f.write(gzip.compress(inputs["g.fa"], 6, mtime=0))
            for n in needs:
                with open(os.path.join(d, os.path.basename(n)), "wb") as f:
                    f.write(produced[n])
            before = set(os.listdir(d))
            r = subprocess.run([exe] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, MALLOC_PERTURB_="255"))
            outs = {}
            for n in sorted(set(os.listdir(d)) - before):
                with open(os.path.join(d, n), "rb") as f:
                    data = f.read()
                produced[name + "/" + n] = data
                masked = mm.mask_mosh(data) if n.endswith(".mosh") else data
                if not n.endswith(".mosh"):
                    masked = "\n".join(mm.mask_lines(data)).encode()
                outs[n] = hashlib.sha256(masked).hexdigest()
                with open(os.path.join(OUT, "%s.%s.gz" % (name, n)), "wb") as f:
                    f.write(gzip.compress(masked, 9, mtime=0))
            manifest["cases"].append({"name": name, "args": args, "needs": needs, "status": r.returncode,
                                      "stdout": mm.mask_lines(r.stdout), "stderr": mm.mask_lines(r.stderr), "outputs": outs})
            print(name, r.returncode, sorted(outs))
        # the merge case must hold entries for which OR-ing and replacing the copy bits differ (moshset.c:117)
        m1 = mm.MoshModel.from_bytes(produced["merge/m1.mosh"]); rc = mm.MoshModel.from_bytes(produced["reads/rc.mosh"])
        differ = 0
        for i in range(1, rc.max + 1):
            old = m1.info[m1.ix.get(rc.value[i], 0)] & 3
            c = min(3, old + (rc.info[i] & 3))
            differ += (old | c) != c
        assert differ > 0, "the merge fixture does not tell OR-ing the copy bits from replacing them"
        manifest["merge_or_differs"] = differ
        with open(os.path.join(HERE, "mosh_manifest.json"), "w") as f:
            json.dump(manifest, f, indent=1)
        big = [(n, os.path.getsize(os.path.join(OUT, n))) for n in os.listdir(OUT) if os.path.isfile(os.path.join(OUT, n))]
        big += [("in/" + n, os.path.getsize(os.path.join(OUT, "in", n))) for n in os.listdir(os.path.join(OUT, "in"))]
        print("OR-differs entries:", differ, " largest:", sorted(big, key=lambda x: -x[1])[:4], " total:", sum(s for _, s in big))
        assert max(s for _, s in big) < 283 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
