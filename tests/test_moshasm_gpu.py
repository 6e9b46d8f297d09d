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
from gap_cases import scan_cap
import orc

pytestmark = pytest.mark.gpu
EXE = os.path.join(orc.REPO, "bin", "moshasm-amd")
MAN = am.manifest()
COMP = str.maketrans("ACGT", "TGCA")


def run(args, cwd, timeout=600):
    if not os.path.exists(EXE):
        pytest.fail("bin/moshasm-amd is missing: run build()")
    return subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def strip_slab(r, n=1):
    """stdout / stderr lines of a run that began with n commands --slab N / --chunk N, without those commands' own lines"""
    out = mm.mask_lines(r.stdout)
    for _ in range(n):
        out.remove("user")
    return out, [ln for ln in mm.mask_lines(r.stderr) if not ln.startswith(("COMMAND --slab", "COMMAND --chunk"))]


def expected_chunks(model, entries=1 << 26, reads=65536):
    """the chunks of queries of the overlap table (include/h10x.h, h10x_mosh_set_option): a read's entries = the depths of its distinct copy-1
    moshes; a chunk ends before the read that takes it past `entries` or `reads`; one without entries is not counted"""
    ms = model.ms
    E = [sum(ms.depth[y] for y in {h & ~am.TOPBIT for h in r.hit} if ms.info[y] & 3 == 1) for r in model.reads]
    n, x0, R = 0, 0, len(E)
    while x0 < R:
        x1, tot = x0 + 1, E[x0]
        while x1 < R and x1 - x0 < reads and tot + E[x1] <= entries:
            tot += E[x1]; x1 += 1
        n += tot > 0
        x0 = x1
    return n


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


def _fresh_program(fresh, pre, tmp_path):
    md, mout, merr = fresh
    d = str(tmp_path)
    for n in ("hap.mosh", "reads.fa"):
        os.link(os.path.join(md, n), os.path.join(d, n))
    r = run(pre + CHAIN, d)
    assert r.returncode == 0, r.stderr.decode()
    out, err = strip_slab(r, len(pre) // 2)
    assert err == mm.mask_lines(merr.encode())
    assert out == mm.mask_lines(mout.encode())
    for n in FILES:
        got = am.mask_file(n, open(os.path.join(d, n), "rb").read()); exp = am.mask_file(n, open(os.path.join(md, n), "rb").read())
        assert got == exp, n


@pytest.mark.parametrize("slab", [0, 4000])
def test_fresh_readset_program(fresh, slab, tmp_path):
    """default slab: one batch; --slab 4000: one or a few reads per batch, so most reads are the first or the last of one"""
    _fresh_program(fresh, ["--slab", slab] if slab else [], tmp_path)


def test_fresh_readset_program_chunked(fresh, tmp_path):
    """--chunk 5000: the overlap table of the 200 reads in many chunks of queries (counted in test_fresh_readset_python_chunked)"""
    md = fresh[0]
    model = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(open(os.path.join(md, "rs.mosh"), "rb").read()), open(os.path.join(md, "rs.readset"), "rb").read())
    assert expected_chunks(model, 5000) > 3
    _fresh_program(fresh, ["--chunk", 5000], tmp_path)


def test_fresh_readset_python(fresh, tmp_path):
    _fresh_python(fresh, tmp_path, {})


@pytest.mark.parametrize("opt,value", [("overlap_chunk_reads", 2), ("overlap_chunk_reads", 64), ("overlap_chunk", 5000)])
def test_fresh_readset_python_chunked(fresh, opt, value, tmp_path):
    """overlaps, mark_bad, mark_contained and write over a table in many chunks: every call reads rows of chunks whose first read is not 0"""
    _fresh_python(fresh, tmp_path, {opt: value})


def _fresh_python(fresh, tmp_path, opts):
    import hash10x_amd
    md = fresh[0]
    d = str(tmp_path)
    ms = hash10x_amd.MoshSet.read(os.path.join(md, "hap.mosh"))
    for name, v in opts.items():
        ms.set_option(name, v)
    with pytest.raises(hash10x_amd.Hash10xError):
        ms.set_option("overlap_chunk_reads", 65537)              # a read's place in its chunk has 16 bits
    rs = hash10x_amd.ReadSet(ms)
    assert rs.add_file(os.path.join(md, "reads.fa"), slab=7000) == ""
    rs.write(os.path.join(d, "rs"))
    model = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(open(os.path.join(md, "rs.mosh"), "rb").read()), open(os.path.join(md, "rs.readset"), "rb").read())
    assert rs.info().chunks == 0                                 # no table yet
    want = expected_chunks(model, opts.get("overlap_chunk", 1 << 26), opts.get("overlap_chunk_reads", 65536))
    for ix in (0, 3, 40, 111):
        o, nrep, ng, nb = rs.overlaps(ix)
        lines = []
        exp = model.find_overlaps(ix, 1, lines.append)
        assert [(int(a["iy"]), int(a["nHit"]), int(a["offset"]), int(a["isPlus"]), int(a["isBad"])) for a in o] == [tuple(e) for e in exp]
        assert lines[0].endswith("nRepeatMosh %d\tnGood %4d\tnBad %4d\n" % (nrep, ng, nb))
    assert rs.info().chunks == want and (want > 3 if opts else want == 1)
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


# ---- the scan's second attempt of -f: a batch of reads with more hits than the estimate its list is sized by (rsAddBatch) ---------------
RUNS = "-m hap.mosh -f reads.fa -S -w rs -o2 7 -b -c".split()
RUN_READS, RUN_LEN = 150, 620


def write_run_case(d, runs):
    """hap.mosh: a 30 kb diploid genome with A^25 at three places of each haplotype, so that hash value 0 is in the set with class M (as a copy-1
    mosh its depth of 65535 would rightly be fatal); reads.fa: 200 reads of 1 kb, the first RUN_READS of them with a run of A or of N in the middle
    when runs is set. Returns the reads"""
    rs = np.random.RandomState(582)
    haps = [h[:4000] + "A" * 25 + h[4000:15000] + "A" * 25 + h[15000:26000] + "A" * 25 + h[26000:] for h in gen_genome(rs, 30000)]
    reads = gen_reads(rs, haps, 200, 1000, 1001, chimeras=0)
    if runs:
        reads = [s[:190] + "AN"[i % 2] * RUN_LEN + s[190 + RUN_LEN:] if i < RUN_READS else s for i, s in enumerate(reads)]
    code = {c: i for i, c in enumerate("ACGT")}
    ms = mm.MoshModel(20, 19, 31, 17)
    ms.add([np.array([code[c] for c in h], np.uint8) for h in haps])
    ms.set_copy(1, 2, 3)
    assert ms.info[ms.ix[0]] & 3 == 3
    with open(os.path.join(d, "hap.mosh"), "wb") as f:
        f.write(ms.to_bytes())
    with open(os.path.join(d, "reads.fa"), "w") as f:
        f.write("".join(">r%d\n%s\n" % (i + 1, s) for i, s in enumerate(reads)))
    return reads


@pytest.mark.parametrize("runs", [True, False], ids=["runs", "control"])
def test_readset_of_low_complexity_reads(runs, tmp_path):
    """150 of 200 reads hit mosh 0 some 600 times each: the batch lists more hits than 2 * (k-mers / w) + 65536 and is scanned again, with acc[] and
    the per-read miss counts cleared in between. Text and files equal the model's; scan_retries rises by one per overflowing batch, by none without runs"""
    import hash10x_amd
    dm = os.path.join(str(tmp_path), "model"); os.makedirs(dm)
    reads = write_run_case(dm, runs)
    st, out, err = am.run_commands(RUNS, dm)
    assert st == 0, err
    model = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(open(os.path.join(dm, "rs.mosh"), "rb").read()), open(os.path.join(dm, "rs.readset"), "rb").read())
    hits = [len(r.hit) for r in model.reads[1:]]
    cap_all, cap_160 = scan_cap([len(s) for s in reads], 19, 31), scan_cap([len(s) for s in reads[:160]], 19, 31)
    assert max(hits) < 65534
    if runs:
        assert sum(hits) > cap_all and sum(hits[:160]) > cap_160 and sum(hits[160:]) < 10000 and model.ms.depth[model.ms.ix[0]] == 65535
    else:
        assert sum(hits) < 10000
    for slab in (0, 160000):                                    # one batch; the first 160 reads (all with a run), then the other 40
        d = os.path.join(str(tmp_path), "slab%d" % slab); os.makedirs(d)
        for n in ("hap.mosh", "reads.fa"):
            os.link(os.path.join(dm, n), os.path.join(d, n))
        r = run((["--slab", slab] if slab else []) + RUNS, d)
        assert r.returncode == 0, r.stderr.decode()
        gout, gerr = strip_slab(r, 1 if slab else 0)
        assert gerr == mm.mask_lines(err.encode())
        assert gout == mm.mask_lines(out.encode())
        for n in ("rs.mosh", "rs.readset"):
            assert am.mask_file(n, open(os.path.join(d, n), "rb").read()) == am.mask_file(n, open(os.path.join(dm, n), "rb").read()), "%s (slab %d)" % (n, slab)
        ms = hash10x_amd.MoshSet.read(os.path.join(dm, "hap.mosh"))
        rs = hash10x_amd.ReadSet(ms)
        assert rs.add_file(os.path.join(dm, "reads.fa"), slab=slab) == ""
        assert ms.counters()["scan_retries"] == (1 if runs else 0), "slab %d" % slab
        rs.write(os.path.join(d, "py"))
        for ext in (".mosh", ".readset"):
            assert open(os.path.join(d, "py" + ext), "rb").read() == open(os.path.join(d, "rs" + ext), "rb").read()
        rs.close(); ms.close()


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
    _shape(name, 0, tmp_path)


@pytest.mark.parametrize("chunk", [1, 200])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_chunked(name, chunk, tmp_path):
    """--chunk 1: every read that has entries is a chunk of its own, the others make none; --chunk 200: chunk ends inside `edges` and `long_list`"""
    _shape(name, chunk, tmp_path)


def _shape(name, chunk, tmp_path):
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
    r = run((["--chunk", chunk] if chunk else []) + cmds, dp)
    assert r.returncode == 0, r.stderr.decode()
    gout, gerr = strip_slab(r, 1 if chunk else 0)
    assert gerr == mm.mask_lines(err.encode())
    assert gout == mm.mask_lines(out.encode())
    for n in ("b.mosh", "b.readset", "c.mosh", "c.readset"):
        assert open(os.path.join(dp, n), "rb").read() == open(os.path.join(dm, n), "rb").read(), n
    if chunk:                                                   # the knob does something: the same files through the class, where the chunks can be counted
        import hash10x_amd
        want = expected_chunks(hand_readset(hand_set(n1), reads), chunk)
        assert (want > 1 or (chunk == 200 and name in ("cutoff", "twice"))) and (chunk != 1 or want == sum(1 for hits in [[]] + reads if any(i <= n1 for i, _, _ in hits)))
        back = hash10x_amd.ReadSet.read(os.path.join(dp, "in"))
        back.ms.set_option("overlap_chunk", chunk)
        back.mark_bad(); back.mark_contained()
        assert back.info().chunks == want
        back.write(os.path.join(dp, "py"))
        for ext in (".mosh", ".readset"):
            assert open(os.path.join(dp, "py" + ext), "rb").read() == open(os.path.join(dm, "c" + ext), "rb").read()
        back.close(); back.ms.close()


# ---- a readset beyond one chunk with no knob: more than 65536 reads ---------------------------------------------------------
BIG_R = 66000
BIG_CMDS = "-r in -o1 65535 -o1 65536 -o1 65537 -o1 66000 -o3 65535 65536 -o2 4001 -b -c -w c".split()


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """66 000 reads of 4 copy-1 hits: read r holds moshes r, r + 1, r + 2, r + 3 (wrapping to 1 after 66 000), so it shares 3 hits with r - 1 and with
    r + 1 and 2 with r - 2 and r + 2: reads 65534 .. 65537 have candidates on both sides of the boundary between the chunks, and the last read has read
    1 and read 65 999. Every fourth read runs backwards and every 500th has a hit out of order. The model's run: computed once"""
    d = str(tmp_path_factory.mktemp("big_model"))
    ms = hand_set(BIG_R)
    reads = []
    for r in range(1, BIG_R + 1):
        ids = [(r - 1 + j) % BIG_R + 1 for j in range(4)]
        if r % 500 == 0:
            ids[1], ids[2] = ids[2], ids[1]
        reads.append([(i, r % 4 != 0, 31 + r % 5) for i in (ids if r % 4 else ids[::-1])])
    rs = hand_readset(ms, reads)
    for ix in range(rs.dim, len(rs.reads)):                    # the reads array grows as -f grows it
        if ix >= rs.dim:
            rs.dim = am.grow_dim(rs.dim, ix)
    assert expected_chunks(rs) == 2
    with open(os.path.join(d, "in.mosh"), "wb") as f:
        f.write(ms.to_bytes())
    with open(os.path.join(d, "in.readset"), "wb") as f:
        f.write(rs.to_bytes())
    st, out, err = am.run_commands(BIG_CMDS, d)
    assert st == 0, err
    for ix in (65534, 65535, 65536, 65537, BIG_R):             # at least two candidates with 3 or more shared hits besides the read itself
        assert sum(1 for e in rs.find_overlaps(ix, 0, lambda s: None) if e[1] >= 3 and e[0] != ix) >= 2
    return d, out, err


def test_readset_beyond_one_chunk(big, tmp_path):
    import hash10x_amd
    md, mout, merr = big
    d = str(tmp_path)
    for n in ("in.mosh", "in.readset"):
        os.link(os.path.join(md, n), os.path.join(d, n))
    r = run(BIG_CMDS, d)
    assert r.returncode == 0, r.stderr.decode()
    assert mm.mask_lines(r.stderr) == mm.mask_lines(merr.encode())
    assert mm.mask_lines(r.stdout) == mm.mask_lines(mout.encode())
    for n in ("c.mosh", "c.readset"):
        assert open(os.path.join(d, n), "rb").read() == open(os.path.join(md, n), "rb").read(), n
    back = hash10x_amd.ReadSet.read(os.path.join(d, "in"))
    back.mark_bad(); back.mark_contained()
    assert back.info().chunks == 2
    back.write(os.path.join(d, "py"))
    assert open(os.path.join(d, "py.readset"), "rb").read() == open(os.path.join(md, "c.readset"), "rb").read()
    back.close(); back.ms.close()


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
