"""moshasm-amd and hash10x_amd.ReadSet on the MI355X (csrc/stage_h.hip). Every comparison is exact equality. Expected results come
from (a) the golden fixtures the reference's moshasm produced (tests/golden/make_asm_golden.py) and (b) the model of
tests/asm_model.py, which tests/test_moshasm_cpu.py pins to (a) byte for byte.

    python tests/test_moshasm_gpu.py gen <dir> <reads> <read length> <genome length> <seed>

writes hap.mosh and reads.fa of the generator below at any size (the measurement in DESIGN.md, stage h)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import asm_model as am
import mosh_model as mm
import orc

pytestmark = pytest.mark.gpu
EXE = os.path.join(orc.REPO, "bin", "moshasm-amd")
MAN = am.manifest()
COMP = str.maketrans("ACGT", "TGCA")


def run(args, cwd, timeout=600):
    if not os.path.exists(EXE):
        pytest.fail("bin/moshasm-amd is missing: run build()")
    return subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def strip_slab(r):
    """stdout / stderr lines of a run that began with --slab N, without that command's own lines"""
    out = mm.mask_lines(r.stdout)
    out.remove("user")
    return out, [ln for ln in mm.mask_lines(r.stderr) if not ln.startswith("COMMAND --slab")]


# ---- (a) every golden case through the program -----------------------------------------------------------------------
@pytest.mark.parametrize("case", MAN["cases"], ids=[c["name"] for c in MAN["cases"]])
def test_program_matches_reference_golden(case, tmp_path):
    d = str(tmp_path)
    before = am.stage_case(MAN, case, d)
    r = run(case["args"], d)
    am.check_case(case, d, before, r.returncode, r.stdout, r.stderr)


# ---- (b) a fresh random readset against the model ----------------------------------------------------------------------
def gen_genome(rs, glen, snp_every=200):
    """a diploid genome with one segment present three times; FASTA text of both haplotypes"""
    B = np.array(list("ACGT"))
    rep = "".join(B[rs.randint(0, 4, max(500, glen // 15))])
    third = (glen - 3 * len(rep)) // 3
    h1 = "".join("".join(B[rs.randint(0, 4, third)]) + rep for _ in range(3))
    h2 = list(h1)
    for p in range(snp_every // 2, len(h1), snp_every):
        q = p + int(rs.randint(0, snp_every // 4))
        if q < len(h2):
            h2[q] = "ACGT"[("ACGT".index(h2[q]) + 1 + rs.randint(0, 3)) % 4]
    return h1, "".join(h2)


def gen_reads(rs, haps, n, lo, hi, chimeras=6, err=0.01):
    reads = []
    for i in range(n):
        g = haps[rs.randint(0, 2)]
        ln = int(rs.randint(lo, hi)); p = int(rs.randint(0, len(g) - ln))
        s = np.array(list(g[p:p + ln]))
        e = np.nonzero(rs.rand(ln) < err)[0]
        s[e] = np.array(list("ACGT"))[rs.randint(0, 4, len(e))]
        s = "".join(s)
        if i < chimeras:                                       # planted: halves swapped, a half inverted, a third repeated
            a, b = s[:ln // 2], s[ln // 2:]
            s = (b + a, a + b.translate(COMP)[::-1], a + b[:ln // 3] + b)[i % 3]
        reads.append(s.translate(COMP)[::-1] if rs.rand() < 0.5 else s)
    order = rs.permutation(n)
    return [reads[i] for i in order]


def write_case(d, seed, n, lo, hi, glen):
    """hap.mosh (copy classes by -s 1 2 3 of the two haplotypes, built by the model) and reads.fa in d"""
    rs = np.random.RandomState(seed)
    haps = gen_genome(rs, glen)
    reads = gen_reads(rs, haps, n, lo, hi)
    code = {c: i for i, c in enumerate("ACGT")}
    ms = mm.MoshModel(20, 19, 31, 17)
    ms.add([np.array([code[c] for c in h], np.uint8) for h in haps])
    ms.set_copy(1, 2, 3)
    with open(os.path.join(d, "hap.mosh"), "wb") as f:
        f.write(ms.to_bytes())
    with open(os.path.join(d, "reads.fa"), "w") as f:
        f.write("".join(">r%d\n%s\n" % (i + 1, s) for i, s in enumerate(reads)))


CHAIN = ("-m hap.mosh -f reads.fa -S -w rs -o2 9 -o1 3 -o1 40 -o3 3 4 -a1 11 -b -S -w rb -c -S -w rc -o2 1 -o file.txt -r rc -S -o1 17").split()
FILES = ("rs.mosh", "rs.readset", "rb.mosh", "rb.readset", "rc.mosh", "rc.readset", "file.txt")


@pytest.fixture(scope="module")
def fresh(tmp_path_factory):
    """the model's run of CHAIN over 200 reads of 0.5-6 kb on a 30 kb diploid genome: computed once"""
    d = str(tmp_path_factory.mktemp("fresh_model"))
    write_case(d, 4711, 200, 500, 6000, 30000)
    st, out, err = am.run_commands(CHAIN, d)
    assert st == 0, err
    return d, out, err


@pytest.mark.parametrize("slab", [0, 4000])
def test_fresh_readset_program(fresh, slab, tmp_path):
    """default slab: one batch; --slab 4000: one or a few reads per batch, so most reads are the first or the last of one"""
    md, mout, merr = fresh
    d = str(tmp_path)
    for n in ("hap.mosh", "reads.fa"):
        os.link(os.path.join(md, n), os.path.join(d, n))
    r = run((["--slab", slab] if slab else []) + CHAIN, d)
    assert r.returncode == 0, r.stderr.decode()
    out, err = strip_slab(r) if slab else (mm.mask_lines(r.stdout), mm.mask_lines(r.stderr))
    assert err == mm.mask_lines(merr.encode())
    assert out == mm.mask_lines(mout.encode())
    for n in FILES:
        got = am.mask_file(n, open(os.path.join(d, n), "rb").read()); exp = am.mask_file(n, open(os.path.join(md, n), "rb").read())
        assert got == exp, n


def test_fresh_readset_python(fresh, tmp_path):
    import hash10x_amd
    md = fresh[0]
    d = str(tmp_path)
    ms = hash10x_amd.MoshSet.read(os.path.join(md, "hap.mosh"))
    rs = hash10x_amd.ReadSet(ms)
    assert rs.add_file(os.path.join(md, "reads.fa"), slab=7000) == ""
    rs.write(os.path.join(d, "rs"))
    model = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(open(os.path.join(md, "rs.mosh"), "rb").read()), open(os.path.join(md, "rs.readset"), "rb").read())
    for ix in (0, 3, 40, 111):
        o, nrep, ng, nb = rs.overlaps(ix)
        lines = []
        exp = model.find_overlaps(ix, 1, lines.append)
        assert [(int(a["iy"]), int(a["nHit"]), int(a["offset"]), int(a["isPlus"]), int(a["isBad"])) for a in o] == [tuple(e) for e in exp]
        assert lines[0].endswith("nRepeatMosh %d\tnGood %4d\tnBad %4d\n" % (nrep, ng, nb))
    rs.write(os.path.join(d, "rs2"))                             # the flags the four calls set
    assert open(os.path.join(d, "rs2.readset"), "rb").read() == model.to_bytes()
    mb = model.mark_bad()
    assert rs.mark_bad() == [int(ln.split()[1]) for ln in mb.splitlines()]
    mc = model.mark_contained()
    nc, nn, tot = rs.mark_contained()
    assert mc == "MC  found %d contained reads, leaving %d not contained, av length %.1f\n" % (nc, nn, tot / float(nn) if nn else 0.)
    rs.write(os.path.join(d, "rc"))
    for ext in (".mosh", ".readset"):
        assert open(os.path.join(d, "rs" + ext), "rb").read() == open(os.path.join(md, "rs" + ext), "rb").read()
    assert open(os.path.join(d, "rc.readset"), "rb").read() == model.to_bytes()
    reads, hs, hit, dx = rs.export()
    assert [int(x) for x in reads["contained"]] == [r.contained for r in model.reads] and int(hs[-1]) == model.totHit == len(hit) == len(dx)
    st = rs.stats()
    assert st["totHit"] == model.totHit and int(st["nCopy"].sum()) == model.ms.max
    rs.close()
    back = hash10x_amd.ReadSet.read(os.path.join(d, "rc"))       # -w then -r: identical files
    back.write(os.path.join(d, "rc2"))
    for ext in (".mosh", ".readset"):
        assert open(os.path.join(d, "rc2" + ext), "rb").read() == open(os.path.join(d, "rc" + ext), "rb").read()
    back.close(); back.ms.close(); ms.close()


# ---- (c) shapes where the kernels can go wrong, hand-built as files ---------------------------------------------------------
def hand_set(n1, nM=4):
    """a set of n1 copy-1 moshes (indices 1 .. n1) and nM of class M after them; the hashes are arbitrary distinct numbers"""
    ms = mm.MoshModel(20, 19, 31, 17)
    for i in range(n1 + nM):
        ms._find_add(0x1000 + 7919 * i)
        ms.info[-1] = 1 if i < n1 else 3
    return ms


def hand_readset(ms, reads):
    """reads = lists of (index, forward, dx); depth is rebuilt from them as -f would"""
    rs = am.ReadsetModel(ms)
    ms.depth = [0] * len(ms.depth)
    for hits in reads:
        r = am.Read()
        r.hit = [i | am.TOPBIT if f else i for i, f, _ in hits]; r.dx = [x for _, _, x in hits]
        r.len = sum(r.dx) + 19; r.nMiss = len(hits) % 3
        for i, _, _ in hits:
            ms.depth[i] = min(65535, ms.depth[i] + 1)
        rs.reads.append(r); rs.totHit += len(hits)
    rs.inv_build()
    return rs


def shapes():
    F = lambda ids, step=31, fwd=True: [(i, fwd, step) for i in ids]          # noqa: E731
    out = {}
    # zero hits; 1, 2 and 3 shared copy-1 hits (the nHit >= 3 cut-off); a read whose only candidate is itself
    out["cutoff"] = (40, [[], F(range(1, 11)), F([1] + list(range(20, 24))), F([1, 2] + list(range(24, 28))), F([1, 2, 3] + list(range(28, 32))),
                          F(range(33, 39)), F([41, 42, 43])])
    # y holds one mosh twice, its list entries spread over two of x's hits; minus and mixed orientations; order violations both ways
    out["twice"] = (30, [F([1, 2, 3, 4, 5, 6]), F([2, 9, 2, 3, 10, 5]), F([6, 5, 4, 3], fwd=False), F([1, 2, 3], fwd=True) + F([4, 5], fwd=False),
                         F([3, 2, 1, 4, 5, 6]), F([4, 5, 6, 3], fwd=False), F([1, 1, 2, 3, 2])])
    # queries with 65 and 257 copy-1 hits (wave and workgroup edges) against reads of 64, 65, 129 and 300 hits, some reversed
    big = list(range(1, 301))
    out["edges"] = (300, [F(big[:65]), F(big[:257]), F(big[:64]), F(big[1:66]), F(big[100:229]), F(big), F(big[:65][::-1], fwd=False), F(big[60:70] + big[:5]),
                          F(big[250:] + big[:7])])
    # one mosh whose inverse list is longer than a workgroup has lanes: 300 reads hold mosh 1, with 2 .. 4 more shared moshes
    out["long_list"] = (12, [F([1, 2, 3, 4][:2 + i % 3] + [5 + i % 7]) for i in range(300)] + [F([1, 2, 3, 4, 5, 6, 7, 8])])
    return out


SHAPES = shapes()
SHAPE_CMDS = "-r in -o2 1 -S -b -S -w b -c -S -w c -o2 2".split()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(name, tmp_path):
    n1, reads = SHAPES[name]
    dm, dp = os.path.join(str(tmp_path), "model"), os.path.join(str(tmp_path), "prog")
    for d in (dm, dp):
        os.makedirs(d)
        ms = hand_set(n1)
        rs = hand_readset(ms, reads)
        with open(os.path.join(d, "in.mosh"), "wb") as f:
            f.write(ms.to_bytes())
        with open(os.path.join(d, "in.readset"), "wb") as f:
            f.write(rs.to_bytes())
    last = len(reads)
    cmds = SHAPE_CMDS + [x for ix in sorted({0, 1, 2, last // 2, last}) for x in ("-o1", str(ix))] + ["-a1", "1", "-a1", str(last)]
    st, out, err = am.run_commands(cmds, dm)
    assert st == 0, err
    if name == "cutoff":                                        # the fixture does what it is for: 3 shared hits is an overlap, 2 is not
        o2 = [ln for ln in out.splitlines() if ln.startswith("RR")][:len(reads)]
        assert [int(ln.split("nGood")[1].split()[0]) for ln in o2] == [0, 2, 1, 1, 2, 1, 0]
    r = run(cmds, dp)
    assert r.returncode == 0, r.stderr.decode()
    assert mm.mask_lines(r.stderr) == mm.mask_lines(err.encode())
    assert mm.mask_lines(r.stdout) == mm.mask_lines(out.encode())
    for n in ("b.mosh", "b.readset", "c.mosh", "c.readset"):
        assert open(os.path.join(dp, n), "rb").read() == open(os.path.join(dm, n), "rb").read(), n


def test_hit_limit(tmp_path):
    """a read with 65534 hits is taken, one with 65535 is refused: a periodic sequence, counted by the oracle's iterator"""
    d = str(tmp_path)
    rs = np.random.RandomState(65534)
    o = orc.Oracle(19, 31, 17, 20)
    while True:
        unit = rs.randint(0, 4, 24).astype(np.uint8)
        probe = np.tile(unit, 4)
        if len(o.mosh(probe)[0]) >= 4:                          # at least one mosh per period
            break
    seq = np.tile(unit, 65600)
    hs, ps = o.mosh(seq)
    assert len(hs) > 65535
    ms = mm.MoshModel(20, 19, 31, 17)
    ms.add([probe]); ms.set_copy(1, 2, 3)
    with open(os.path.join(d, "per.mosh"), "wb") as f:
        f.write(ms.to_bytes())
    for n in (65534, 65535):
        s = seq[:int(ps[n - 1]) + 19]
        assert len(o.mosh(s)[0]) == n
        with open(os.path.join(d, "p%d.fa" % n), "wb") as f:
            f.write(b">p\n" + np.frombuffer(b"ACGT", np.uint8)[s].tobytes() + b"\n")
    r = run(["-m", "per.mosh", "-f", "p65534.fa", "-S"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert any(ln.startswith("RS 65534 mosh hits") for ln in r.stdout.decode().splitlines())
    r = run(["-m", "per.mosh", "-f", "p65535.fa", "-S"], d)
    assert r.returncode == 255 and r.stderr.decode().splitlines()[-1] == "FATAL ERROR: read 1 has 65535 hits: more than 65534 are not supported"


def test_misuse_ends_with_a_message(tmp_path):
    d = str(tmp_path)
    case = [c for c in MAN["cases"] if c["name"] == "stats"][0]
    am.stage_case(MAN, case, d)
    for args, last in ((["-m", "hap.mosh", "-S"], "-S needs a readset: give -f or -r first"),
                       (["-m", "hap.mosh", "-f", "reads.fa", "-f", "reads.fa"], "a second -f needs a new -m first (the reference closes the mosh file twice here)"),
                       (["-r", "rs", "-o1", "100000"], "read 100000 is outside the readset of "),
                       (["-r", "rs", "-o2", "0"], "-o2 needs a step of at least 1")):
        r = run(args, d)
        assert r.returncode == 255, args
        got = r.stderr.decode().splitlines()[-1]
        assert got.startswith("FATAL ERROR: " + last) and (got == "FATAL ERROR: " + last or last.endswith(" of "))


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "gen":
    os.makedirs(sys.argv[2], exist_ok=True)
    n, ln, glen, seed = (int(x) for x in sys.argv[3:7])
    write_case(sys.argv[2], seed, n, ln * 3 // 4, ln * 5 // 4, glen)
