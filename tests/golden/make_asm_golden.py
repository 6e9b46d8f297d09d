#!/usr/bin/env python3
"""Regenerates tests/golden/asm/: inputs from fixed seeds, and what the REFERENCE's moshasm makes of them.

    python tests/golden/make_asm_golden.py /path/to/reference
    python tests/golden/make_asm_golden.py /path/to/reference --time DIR     (no fixtures are touched)

--time compiles the reference's moshasm with -O3 into the temporary directory and prints the wall time of `-m hap.mosh -f reads.fa -w rs`
and of `-r rs -b -c` on the hap.mosh and reads.fa of DIR (written by `python tests/test_moshasm_gpu.py gen DIR ...`): the CPU side of the
measurement in DESIGN.md, section 12. rs.mosh and rs.readset stay in DIR, for the same commands of bin/moshasm-amd.

The reference's moshasm and moshutils are compiled into a temporary directory outside the tree and run there with
MALLOC_PERTURB_=255; only data comes back: the inputs (gzipped), every output file (gzipped, masked) and
tests/golden/asm_manifest.json with the command lines, exit status, stdout / stderr lines (resource figures masked) and the
sha256 of each masked output. Masks: value[0] of a .mosh; in a .readset the heap pointers the reference leaks
(ArrayStruct.base, Read.hit and Read.dx of every record). No reference source or binary is copied.

The script refuses to write fixtures that do not exercise what the tests are for: see conditions()."""
import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import asm_model as am  # noqa: E402
import mosh_model as mm  # noqa: E402

OUT = os.path.join(HERE, "asm")
LIB = "seqio.c seqhash.c moshset.c hash.c dict.c array.c utils.c".split()
COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(COMP)[::-1]


def make_inputs():
    rs = np.random.RandomState(20181106)
    B = np.array(list("ACGT"))

    def rnd(n):
        return "".join(B[rs.randint(0, 4, n)])

    def noisy(s, rate=0.01):
        s = list(s)
        for q in np.nonzero(rs.rand(len(s)) < rate)[0]:
            s[q] = "ACGT"[rs.randint(0, 4)]
        return "".join(s)

    rep = rnd(3000)                                             # present three times: copy M
    parts = [rnd(11000), rep, rnd(12000), rep, rnd(8000), rep]
    h1 = "".join(parts)
    h2 = list(h1)
    for p in range(100, len(h1), 200):                          # a SNP about every 200 bases, none inside the repeat copies
        q = p + int(rs.randint(0, 50))
        if not any(s <= q < s + 3000 for s in (11000, 26000, 37000)):
            h2[q] = "ACGT"[("ACGT".index(h2[q]) + 1 + rs.randint(0, 3)) % 4]
    h2 = "".join(h2)
    island = rnd(20000)                                         # haploid: every mosh of it is copy 1
    hap = "".join(">%s\n" % n + "".join(s[i:i + 80] + "\n" for i in range(0, len(s), 80)) for n, s in (("hap1", h1), ("hap2", h2), ("island", island)))
    reads, special = [], {}

    def plant(name, s):
        special[name] = len(reads) + 1                          # reads are numbered from 1
        reads.append(s)

    for i in range(300):                                        # ordinary reads: 1-8 kb, either strand, 1 % errors
        n = int(rs.randint(1000, 8000)); g = (h1, h2)[rs.randint(0, 2)]; p = int(rs.randint(0, len(g) - n))
        s = noisy(g[p:p + n])
        reads.append(rc(s) if rs.rand() < 0.5 else s)
        if i == 60:
            plant("order10", h1[4000:8000] + h1[500:4000])      # two segments in the wrong order, under 12 covering reads
            for j in range(12):
                reads.append(noisy(h1[300 - 20 * j:8200 + 20 * j]))
        if i == 120:
            plant("inverted", h2[16000:19000] + rc(h2[19000:22000]))
            plant("short_random", rnd(700)); plant("long_random", rnd(9000))
            plant("triple_only", rep[100:2900])
            plant("shorter_than_k", rnd(12)); plant("empty", "")
        if i == 200:
            plant("island_cover", island[0:6000]); plant("island_chimera", island[3000:4500] + island[1500:3000])
            plant("contained_tie", island[7000:8000]); plant("container1", island[6500:9500]); plant("container2", island[6200:9200])
            plant("tandem", island[9600:10600] + island[9600:10600]); plant("tandem_cover", island[9400:11800])
            for j, (a, b) in enumerate(((12500, 18500), (12700, 18300), (13000, 18000))):      # three covers: 3 bad overlaps, the second pass of -b
                plant("island_cover2_%d" % j, island[a:b])
            plant("island_chimera2", island[15500:17000] + island[14000:15500])
            plant("contained_short", h1[30000:31000]); plant("contained_long", h1[29000:33500])
            plant("dx_wrap", h1[22000:24000] + rnd(66000) + h1[24000:26000])
    fa = "".join(">r%d\n%s\n" % (i + 1, s) for i, s in enumerate(reads))
    return {"hap.fa": hap.encode(), "reads.fa": fa.encode()}, special


def cases(sp):
    need = ["build/rs.mosh", "build/rs.readset"]
    o1 = [sp[n] for n in ("order10", "inverted", "island_chimera", "contained_tie", "tandem", "dx_wrap", "triple_only")] + [0, 5]
    c = [("build", "-m hap.mosh -f reads.fa -S -w rs".split(), []),
         ("stats", "-r rs -S".split(), need),
         ("o2_1", "-r rs -o2 1".split(), need),
         ("o2_7", "-r rs -o2 7".split(), need)]
    c += [("o1_%d" % ix, ["-r", "rs", "-o1", str(ix)], need) for ix in o1]
    c += [("o3", ["-r", "rs", "-o3", str(sp["island_cover"]), str(sp["island_chimera"]), "-o3", str(sp["tandem"]), str(sp["tandem_cover"])], need),
          ("bad", "-r rs -b -S -w rb".split(), need),
          ("badc", "-r rs -b -c -S -w rc".split(), need),
          ("bad_o2", "-r rs -b -o2 1".split(), need),
          ("a1", ["-r", "rs", "-a1", str(sp["island_cover"]), "-a1", str(sp["order10"]), "-a1", "9"], need),
          ("long", ["--threads", "2", "--verbose", "--output", "long.txt", "--moshset", "hap.mosh", "--seqfile", "reads.fa", "--stats", "--overlaps2", "50",
                    "--overlap", "3", "4", "--overlaps1", "5", "--markBadReads", "--markContained", "--assemble1", "5", "--write", "rl", "--output", "-",
                    "--read", "rl", "--stats"], []),
         ("unknown", ["-x"], []), ("no_dash", ["foo"], []), ("no_mosh", ["-m", "nosuch.mosh"], []), ("no_stem", ["-r", "nosuch"], []),
         ("no_readset_file", ["-r", "hap"], []), ("f_before_m", ["-f", "reads.fa", "-t", "3"], []), ("bad_output", ["-o", "/nonexistent/dir/x", "-v"], []),
         ("short_args", ["-m"], [])]
    return c


def conditions(manifest, produced, inputs, sp):
    """what the fixture must show, from the reference's own output"""
    by = {c["name"]: c for c in manifest["cases"]}
    bad = [ln for ln in by["bad"]["stdout"] if ln.startswith("RS bad")][0]
    nums = [int(x) for x in re.findall(r"\d+", bad.replace("order10", "").replace("order1", "").replace("low_copy1", ""))]
    assert len(nums) == 7 and all(nums), "a bad class is empty after -b: " + bad
    mb = [int(ln.split()[1]) for ln in by["bad"]["stdout"] if ln.startswith("MB")]
    assert len(mb) == 3 and all(mb), "a pass of -b finds nothing: %r" % mb
    rh = [ln for c in manifest["cases"] if c["name"].startswith("o1_") for ln in c["stdout"] if ln.startswith("RH")]
    pm = [(int(re.search(r"nPlus (\d+)", ln).group(1)), int(re.search(r"nMinus (\d+)", ln).group(1))) for ln in rh]
    assert any(p == 0 and m > 0 for p, m in pm), "no minus-only overlap"
    assert any(p > 0 and m > 0 for p, m in pm), "no mixed overlap"
    mc = [ln for ln in by["badc"]["stdout"] if ln.startswith("MC")][0]
    assert int(mc.split()[2]) > 0, "no contained read"
    # the two conditions the reference's text does not show are read off its files with the model
    ms = mm.MoshModel.from_bytes(produced["build/rs.mosh"])
    ref = am.ReadsetModel.from_bytes(ms, produced["build/rs.readset"])
    seqs, _ = mm.parse_seq_bytes(inputs["reads.fa"], "reads.fa")
    wraps = 0
    for r, s in zip(ref.reads[1:], seqs):
        _, ps = ms.moshes(s)
        hits = [int(p) for h, p in zip(*ms.moshes(s)) if int(h) in ms.ix]
        wraps += sum(r.dx) != (hits[-1] if hits else 0)
    assert wraps > 0, "no dx that differs from the true distance"
    rb = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(produced["bad/rb.mosh"]), produced["bad/rb.readset"])
    rb.mark_contained()
    rcm = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(produced["badc/rc.mosh"]), produced["badc/rc.readset"])
    assert [r.contained for r in rb.reads] == [r.contained for r in rcm.reads], "the model's contained choices differ from the reference's"
    assert rb.ties > 0, "no read whose contained choice a tie in nHit decides"
    assert rcm.reads[sp["contained_tie"]].contained == sp["container1"]
    manifest["conditions"] = {"bad_line": nums, "mb": mb, "minus_only": sum(p == 0 and m > 0 for p, m in pm), "mixed": sum(p > 0 and m > 0 for p, m in pm),
                              "contained": int(mc.split()[2]), "tie_decided": rb.ties, "dx_wrapped_reads": wraps}


def time_reference(ref, d):
    import time
    tmp = tempfile.mkdtemp(prefix="asmtime_")
    try:
        exe = os.path.join(tmp, "moshasm")
        subprocess.run(["gcc", "-O3", "-w", "-o", exe, os.path.join(ref, "moshasm.c")] + [os.path.join(ref, s) for s in LIB] + ["-lz", "-lm"], check=True)
        for args in ("-m hap.mosh -f reads.fa -w rs", "-r rs -b -c"):
            t0 = time.time()
            subprocess.run([exe] + args.split(), cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            print("reference moshasm (gcc -O3) %s: %.2f s wall" % (args, time.time() - t0))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    if len(sys.argv) > 3 and sys.argv[2] == "--time":
        return time_reference(ref, sys.argv[3])
    tmp = tempfile.mkdtemp(prefix="asmgold_")
    try:
        exe = os.path.join(tmp, "moshasm"); util = os.path.join(tmp, "moshutils")
        for out, main_c in ((exe, "moshasm.c"), (util, "moshutils.c")):
            subprocess.run(["gcc", "-O2", "-w", "-o", out, os.path.join(ref, main_c)] + [os.path.join(ref, s) for s in LIB] + ["-lz", "-lm"], check=True)
        inputs, sp = make_inputs()
        env = dict(os.environ, MALLOC_PERTURB_="255")
        d0 = os.path.join(tmp, "set"); os.makedirs(d0)
        with open(os.path.join(d0, "hap.fa"), "wb") as f:
            f.write(inputs["hap.fa"])
        subprocess.run([util] + "-c 20 19 31 17 -a hap.fa -s 1 2 3 -w hap.mosh".split(), cwd=d0, check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(os.path.join(d0, "hap.mosh"), "rb") as f:
            inputs["hap.mosh"] = mm.mask_mosh(f.read())
        if os.path.isdir(OUT):
            shutil.rmtree(OUT)
        os.makedirs(os.path.join(OUT, "in"))
        for name, data in inputs.items():
            with open(os.path.join(OUT, "in", name + ".gz"), "wb") as f:
                f.write(gzip.compress(data, 9, mtime=0))
        manifest = {"inputs": sorted(inputs), "special": sp, "cases": []}
        produced = {}
        for name, args, needs in cases(sp):
            d = os.path.join(tmp, name); os.makedirs(d)
            for n, data in inputs.items():
                with open(os.path.join(d, n), "wb") as f:
                    f.write(data)
            for n in needs:
                with open(os.path.join(d, os.path.basename(n)), "wb") as f:
                    f.write(produced[n])
            before = set(os.listdir(d))
            r = subprocess.run([exe] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
            outs = {}
            for n in sorted(set(os.listdir(d)) - before):
                with open(os.path.join(d, n), "rb") as f:
                    data = f.read()
                masked = am.mask_file(n, data)
                produced[name + "/" + n] = masked
                outs[n] = hashlib.sha256(masked).hexdigest()
                with open(os.path.join(OUT, "%s.%s.gz" % (name, n)), "wb") as f:
                    f.write(gzip.compress(masked, 9, mtime=0))
            manifest["cases"].append({"name": name, "args": args, "needs": needs, "status": r.returncode & 255,
                                      "stdout": mm.mask_lines(r.stdout), "stderr": mm.mask_lines(r.stderr), "outputs": outs})
            print(name, r.returncode, sorted(outs))
        conditions(manifest, produced, inputs, sp)
        with open(os.path.join(HERE, "asm_manifest.json"), "w") as f:
            json.dump(manifest, f, indent=1)
        big = [(os.path.join(dp, n), os.path.getsize(os.path.join(dp, n))) for dp, _, fn in os.walk(OUT) for n in fn]
        print("conditions:", manifest["conditions"], " largest:", sorted(big, key=lambda x: -x[1])[:3], " total:", sum(s for _, s in big))
        assert max(s for _, s in big) < 1 << 20
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
