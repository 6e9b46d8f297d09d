#!/usr/bin/env python3
"""Regenerates tests/golden/map/: inputs from fixed seeds, and what the REFERENCE's moshmap makes of them.

    python tests/golden/make_map_golden.py /path/to/reference
    python tests/golden/make_map_golden.py /path/to/reference --time DIR     (no fixtures are touched)

--time compiles the reference's moshmap with -O3 into the temporary directory and prints the wall time of `-B 26 -f ref.fa -w idx` and of
`-r idx -q reads.fa` on the ref.fa and reads.fa of DIR (written by `python tests/test_moshmap_gpu.py gen DIR ...`): the CPU side of the
measurement in DESIGN.md, section 13.

The reference's moshmap is compiled into a temporary directory outside the tree and run there with MALLOC_PERTURB_=255; only data comes
back: the inputs (gzipped), every output file (gzipped, masked) and tests/golden/map_manifest.json with the command lines, exit status,
stdout / stderr lines (resource figures masked) and the sha256 of each masked output. Masks: value[0] of a .mosh; in a .ref the heap
pointers the reference leaks (ArrayStruct.base of the lengths, the dict's name pointers). No reference source or binary is copied.

The script refuses to write fixtures that do not exercise what the tests are for: see conditions()."""
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
import map_model as mp  # noqa: E402
import mosh_model as mm  # noqa: E402

OUT = os.path.join(HERE, "map")
LIB = "readseq.c seqhash.c moshset.c hash.c dict.c array.c utils.c".split()
COMP = str.maketrans("ACGT", "TGCA")
CODE = {c: i for i, c in enumerate("ACGT")}


def rc(s):
    return s.translate(COMP)[::-1]


def fasta(records, width=70):
    return "".join(">%s\n" % h + "".join(s[i:i + width] + "\n" for i in range(0, len(s), width)) for h, s in records).encode()


def make_inputs():
    rs = np.random.RandomState(20181027)
    B = np.array(list("ACGT"))

    def rnd(n):
        return "".join(B[rs.randint(0, 4, n)])

    def noisy(s, rate=0.01):
        s = list(s)
        for q in np.nonzero(rs.rand(len(s)) < rate)[0]:
            s[q] = "ACGT"[("ACGT".index(s[q]) + 1 + rs.randint(0, 3)) % 4]
        return "".join(s)

    dup, rep = rnd(4000), rnd(2000)                              # dup in both sequences: copy 2; rep three times: copy M
    chrA = rnd(10000) + dup + rnd(8000) + rep + rnd(6000) + rep   # dup at 10000, rep at 22000 and 30000
    chrB = rnd(6000) + rep + rnd(5000) + dup + rnd(5000)          # rep at 6000, dup at 13000
    # the file's text: lower case, a run of N (read as A) and line breaks; the queries are cut from what the reader makes of it
    textA = chrA[:15000] + chrA[15000:16000].lower() + chrA[16000:17000] + "N" * 40 + chrA[17040:]
    chrA = chrA[:17000] + "A" * 40 + chrA[17040:]
    ref = fasta([("chrA the first sequence, with a description", textA), ("chrB", chrB)])
    ms = mm.MoshModel(20, 19, 31, 17)
    _, pa = ms.moshes(np.array([CODE[c] for c in chrA], np.uint8))
    in_dup = [int(p) for p in pa if 10000 <= p <= 14000 - 19]
    q = [("single", chrA[1000:5000]),
         ("two_blocks", chrA[500:4000] + chrA[6500:9500]),
         ("small_excision", chrA[500:4000] + chrA[4500:7500]),
         ("reverse_two_blocks", rc(chrA[500:4000] + chrA[6500:9500])),
         ("chimera", chrA[1000:4000] + chrB[1000:4000]),
         ("rescue", chrB[10000:20000]),
         ("copy2_only", dup[500:3500]),
         ("last_block_two_copy2", chrA[7000:in_dup[1] + 19]),
         ("copyM_only", rep[200:1800]),
         ("first_mosh", chrA[0:1500] + dup[0:1000]),
         ("tandem", chrA[1000:2500] + chrA[1000:2500]),
         ("shorter_than_k", rnd(12)),
         ("random", rnd(3000)),
         ("noisy", noisy(chrB[500:5500])),
         ("reverse_noisy lower", rc(noisy(chrA[24000:29000])).lower()),
         ("empty", ""),
         ("after_empty", chrA[1000:5000])]
    many = [("s%d" % i, rnd(100)) for i in range(310)]
    manyq = [("m%d" % i, many[i][1] + many[i + 1][1]) for i in (0, 150, 308)]
    return {"ref.fa": ref, "q.fa": fasta(q, 100), "many.fa": fasta(many), "manyq.fa": fasta(manyq),
            "dupname.fa": fasta([("x", rnd(300)), ("y", rnd(300)), ("x again", rnd(300))])}


def cases():
    need = ["build/idx.mosh", "build/idx.ref"]
    return [("build", "-B 20 -f ref.fa -w idx -q q.fa".split(), ["ref.fa", "q.fa"], []),
            ("read", "-r idx -q q.fa".split(), ["q.fa"], need),
            ("rewrite", "-r idx -w idx2".split(), [], need),
            ("verbose_file", "-B 20 -f ref.fa -v -o out.txt -q q.fa".split(), ["ref.fa", "q.fa"], []),
            ("verbose_stdout", "-r idx -v -q q.fa -v -q q.fa".split(), ["q.fa"], need),
            ("params", "-K 16 -W 11 -S 5 -B 20 -f ref.fa -q q.fa -w p".split(), ["ref.fa", "q.fa"], []),
            ("many", "-B 20 -f many.fa -w many -q manyq.fa".split(), ["many.fa", "manyq.fa"], []),
            ("dupname", "-B 20 -f dupname.fa".split(), ["dupname.fa"], []),
            ("long", ["--threads", "2", "--kmer", "19", "--window", "31", "--seed", "17", "--tableBits", "20", "--referenceFasta", "ref.fa", "--referenceWrite", "l",
                      "--output", "long.txt", "--verbose", "--query", "q.fa", "--output", "-"], ["ref.fa", "q.fa"], []),
            ("q_before_ref", ["-q", "q.fa"], ["q.fa"], []), ("unknown", ["-x"], [], []), ("no_dash", ["foo"], [], []), ("no_fasta", ["-f", "nosuch.fa"], [], []),
            ("no_stem", ["-r", "nosuch"], [], []), ("no_query", ["-r", "idx", "-q", "nosuch.fa"], [], need), ("bad_bits", ["-B", "19", "-f", "ref.fa"], ["ref.fa"], []),
            ("bad_k", ["-K", "0", "-f", "ref.fa"], ["ref.fa"], []), ("bad_output", ["-o", "/nonexistent/dir/x", "-v"], [], []), ("short_args", ["-f"], [], [])]


def conditions(manifest):
    """what the fixture must show, from the reference's own output"""
    by = {c["name"]: c for c in manifest["cases"]}
    out = by["build"]["stdout"]

    def lines(tag, name):
        return [ln for ln in out if ln.startswith(tag + "\t" + name + "\t")]
    assert not lines("M", "single"), "a single copy-1 block printed an M line"
    assert len(lines("M", "two_blocks")) == 1, "the excision of 2.5 kb did not end the block"
    assert not lines("M", "small_excision"), "the excision of 0.5 kb ended the block"
    assert len(lines("M", "reverse_two_blocks")) == 1
    ch = lines("M", "chimera")
    assert len(ch) == 1 and ch[0].split("\t")[5] == "chrA", "no M line at the change of sequence"
    rescue = lines("M", "rescue")
    assert len(rescue) == 1 and rescue[0].split("\t")[5] == "chrB" and int(rescue[0].split("\t")[8].split()[1]) > 2, "the second copy was not taken: %r" % rescue
    c2 = lines("M", "copy2_only")
    assert len(c2) == 1 and c2[0].endswith("-nan"), "copy-2 only: %r" % c2
    last2 = lines("Q", "last_block_two_copy2")
    assert len(last2) == 1 and " 2 copy2," in last2[0] and not lines("M", "last_block_two_copy2")
    assert " 0 copy1, 0 copy2," in lines("Q", "copyM_only")[0] and " 0 multi" not in lines("Q", "copyM_only")[0]
    first = lines("M", "first_mosh")                              # hit 0 of the reference opens no block: the first block starts on the second seed
    assert "\t0 miss" in lines("Q", "first_mosh")[0] and first and first[0].split("\t")[6] != "0", "the query on the reference's first hit: %r" % first
    assert lines("M", "tandem"), "the backwards step of the tandem query ended no block"
    assert lines("Q", "shorter_than_k")[0].endswith("-nan hit")
    assert lines("Q", "random")[0].endswith("0.00 hit")
    assert not lines("Q", "empty") and not lines("Q", "after_empty"), "reading went on behind the empty sequence"
    assert by["dupname"]["status"] == 255 and by["dupname"]["stderr"][-1] == "FATAL ERROR: duplicate ref sequence name x"
    assert [ln for ln in by["read"]["stdout"] if ln[:1] in "QM"] == [ln for ln in out if ln[:1] in "QM"], "-r -q differs from -f -q"
    assert by["rewrite"]["outputs"]["idx2.ref"] == by["build"]["outputs"]["idx.ref"] and by["rewrite"]["outputs"]["idx2.mosh"] == by["build"]["outputs"]["idx.mosh"]
    manifest["conditions"] = {"m_lines": sum(ln.startswith("M\t") for ln in out), "q_lines": sum(ln.startswith("Q\t") for ln in out)}


def time_reference(ref, d):
    import time
    tmp = tempfile.mkdtemp(prefix="maptime_")
    try:
        exe = os.path.join(tmp, "moshmap")
        subprocess.run(["gcc", "-O3", "-w", "-o", exe, os.path.join(ref, "moshmap.c")] + [os.path.join(ref, s) for s in LIB] + ["-lm"], check=True)
        for args in ("-B 26 -f ref.fa -w idx", "-r idx -q reads.fa"):
            t0 = time.time()
            subprocess.run([exe] + args.split(), cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            print("reference moshmap (gcc -O3) %s: %.2f s wall" % (args, time.time() - t0))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    if len(sys.argv) > 3 and sys.argv[2] == "--time":
        return time_reference(ref, sys.argv[3])
    tmp = tempfile.mkdtemp(prefix="mapgold_")
    try:
        exe = os.path.join(tmp, "moshmap")
        subprocess.run(["gcc", "-O2", "-w", "-o", exe, os.path.join(ref, "moshmap.c")] + [os.path.join(ref, s) for s in LIB] + ["-lm"], check=True)
        inputs = make_inputs()
        env = dict(os.environ, MALLOC_PERTURB_="255")
        if os.path.isdir(OUT):
            shutil.rmtree(OUT)
        os.makedirs(os.path.join(OUT, "in"))
        for name, data in inputs.items():
            with open(os.path.join(OUT, "in", name + ".gz"), "wb") as f:
                f.write(gzip.compress(data, 9, mtime=0))
        manifest = {"cases": []}
        produced = {}
        for name, args, ins, needs in cases():
            d = os.path.join(tmp, name); os.makedirs(d)
            for n in ins:
                with open(os.path.join(d, n), "wb") as f:
                    f.write(inputs[n])
            for n in needs:
                with open(os.path.join(d, os.path.basename(n)), "wb") as f:
                    f.write(produced[n])
            before = set(os.listdir(d))
            r = subprocess.run([exe] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            outs = {}
            for n in sorted(set(os.listdir(d)) - before):
                with open(os.path.join(d, n), "rb") as f:
                    data = f.read()
                masked = mp.mask_file(n, data)
                produced[name + "/" + n] = masked
                outs[n] = hashlib.sha256(masked).hexdigest()
                with open(os.path.join(OUT, "%s.%s.gz" % (name, n)), "wb") as f:
                    f.write(gzip.compress(masked, 9, mtime=0))
            manifest["cases"].append({"name": name, "args": args, "inputs": ins, "needs": needs, "status": r.returncode & 255,
                                      "stdout": mm.mask_lines(r.stdout), "stderr": mm.mask_lines(r.stderr), "outputs": outs})
            print(name, r.returncode, sorted(outs))
        conditions(manifest)
        with open(os.path.join(HERE, "map_manifest.json"), "w") as f:
            json.dump(manifest, f, indent=1)
        big = [(os.path.join(dp, n), os.path.getsize(os.path.join(dp, n))) for dp, _, fn in os.walk(OUT) for n in fn]
        print("conditions:", manifest["conditions"], " largest:", sorted(big, key=lambda x: -x[1])[:3], " total:", sum(s for _, s in big))
        assert max(s for _, s in big) < 1 << 20
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
