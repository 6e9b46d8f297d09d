"""moshmap-amd and hash10x_amd.RefMap on the MI355X (csrc/stage_i.hip). Every comparison is exact equality. Expected results come from
(a) the golden fixtures the reference's moshmap produced (tests/golden/make_map_golden.py) and (b) the model of tests/map_model.py,
which tests/test_moshmap_cpu.py pins to (a) byte for byte.

    python tests/test_moshmap_gpu.py gen <dir> <reference length> <reads> <read length> <seed>

writes ref.fa and reads.fa of the generator below at any size (the measurement in DESIGN.md, section 13)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import map_model as mp
import mosh_model as mm
from gap_cases import GAP, gap_seqs, scan_cap, to_codes, write_fa
import orc

pytestmark = pytest.mark.gpu
EXE = os.path.join(orc.REPO, "bin", "moshmap-amd")
MAN = mp.manifest()
COMP = str.maketrans("ACGT", "TGCA")
CODE = {c: i for i, c in enumerate("ACGT")}


def run(args, cwd, timeout=600):
    if not os.path.exists(EXE):
        pytest.fail("bin/moshmap-amd is missing: run build()")
    return subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def case(name):
    return next(c for c in MAN["cases"] if c["name"] == name)


# ---- (a) every golden case through the program -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MAN["cases"], ids=[c["name"] for c in MAN["cases"]])
def test_program_matches_reference_golden(c, tmp_path):
    d = str(tmp_path)
    before = mp.stage_case(MAN, c, d)
    r = run(c["args"], d)
    mp.check_case(c, d, before, r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("name", ["build", "verbose_stdout", "many"])
def test_slab_does_not_change_the_result(name, tmp_path):
    """--slab 1000: every query of q.fa but two is longer than the slab and goes alone; the 310 sequences of 100 bases go ten to a slab"""
    c = case(name)
    d = str(tmp_path)
    before = mp.stage_case(MAN, c, d)
    r = run(["--slab", 1000] + c["args"], d)
    out = mm.mask_lines(r.stdout)
    out.remove("user")
    err = [ln for ln in mm.mask_lines(r.stderr) if not ln.startswith("COMMAND --slab")]
    mp.check_case(c, d, before, r.returncode, "\n".join(out).encode(), "\n".join(err).encode())


# ---- (b) a fresh seeded case against the model -----------------------------------------------------------------------------------------
def gen_case(d, glen, n, lo, hi, seed, err=0.01):
    """ref.fa: three sequences with a stretch present twice and one present three times; reads.fa: n reads of lo .. hi bases, both strands"""
    rs = np.random.RandomState(seed)
    B = np.frombuffer(b"ACGT", np.uint8)
    CB = np.zeros(256, np.uint8); CB[B] = B[::-1]                # complement
    rnd = lambda m: B[rs.randint(0, 4, m)]
    dup, rep = rnd(max(500, glen // 25)), rnd(max(300, glen // 50))
    third = glen // 3
    seqs = [np.concatenate(p) for p in ((rnd(third), dup, rnd(third // 4), rep), (rep, rnd(third), dup), (rnd(third // 2), rep, rnd(third // 2)))]
    with open(os.path.join(d, "ref.fa"), "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">chr%d sequence %d\n" % (i + 1, i))
            pad = np.full((-len(s)) % 80, 10, np.uint8)          # 80 bases a line; the last line is padded with newlines, which the reader passes over
            f.write(np.concatenate([np.concatenate([s, pad]).reshape(-1, 80), np.full(((len(s) + 79) // 80, 1), 10, np.uint8)], axis=1).tobytes())
    with open(os.path.join(d, "reads.fa"), "wb") as f:
        for i in range(n):
            g = seqs[rs.randint(0, 3)]
            ln = int(rs.randint(lo, hi + 1)); p = int(rs.randint(0, len(g) - ln))
            s = g[p:p + ln].copy()
            e = np.nonzero(rs.rand(ln) < err)[0]
            s[e] = B[rs.randint(0, 4, len(e))]
            if i % 37 == 5:                                        # a chimera of two places
                p2 = int(rs.randint(0, len(g) - ln))
                s = np.concatenate([s[:ln // 2], g[p2:p2 + ln // 2]])
            if rs.rand() < 0.5:
                s = CB[s][::-1]
            f.write(b">r%d\n" % (i + 1) + s.tobytes() + b"\n")


FRESH = "-B 20 -f ref.fa -w idx -q reads.fa -v -o v.txt -q reads.fa".split()


@pytest.fixture(scope="module")
def fresh(tmp_path_factory):
    """the model's run of FRESH over a 200 kb reference and 300 reads of 1 - 5 kb: computed once"""
    d = str(tmp_path_factory.mktemp("fresh_map"))
    gen_case(d, 200000, 300, 1000, 5000, 1027)
    st, out, err = mp.run_commands(FRESH, d)
    assert st == 0, err
    assert sum(ln.startswith("M\t") for ln in out.splitlines()) > 10             # (most reads are one copy-1 block, which prints no M line)
    files = {}
    for n in ("idx.mosh", "idx.ref", "v.txt"):
        with open(os.path.join(d, n), "rb") as f:
            files[n] = f.read()
        os.remove(os.path.join(d, n))
    return d, out, err, files


@pytest.mark.parametrize("slab", [0, 3000])
def test_fresh_reference_program(fresh, slab, tmp_path):
    md, mout, merr, mfiles = fresh
    d = str(tmp_path)
    for n in ("ref.fa", "reads.fa"):
        os.link(os.path.join(md, n), os.path.join(d, n))
    r = run((["--slab", slab] if slab else []) + FRESH, d)
    assert r.returncode == 0, r.stderr.decode()
    out, err = mm.mask_lines(r.stdout), mm.mask_lines(r.stderr)
    if slab:
        out.remove("user")
        err = [ln for ln in err if not ln.startswith("COMMAND --slab")]
    assert err == mm.mask_lines(merr.encode())
    assert out == mm.mask_lines(mout.encode())
    for n, exp in mfiles.items():
        with open(os.path.join(d, n), "rb") as f:
            assert mp.mask_file(n, f.read()) == mp.mask_file(n, exp), n


def test_fresh_reference_refmap(fresh):
    """the same through hash10x_amd.RefMap: the arrays of the .ref file, the Q counts and the M records as integers"""
    import hash10x_amd
    md, _, _, mfiles = fresh
    with open(os.path.join(md, "ref.fa"), "rb") as f:
        rnames, rseqs = mp.parse_fasta(f.read())
    with open(os.path.join(md, "reads.fa"), "rb") as f:
        qnames, qseqs = mp.parse_fasta(f.read())
    model = mp.RefModel.from_bytes(mm.MoshModel.from_bytes(mfiles["idx.mosh"]), mfiles["idx.ref"])
    ms = hash10x_amd.MoshSet(B=20)
    rm = hash10x_amd.RefMap(ms)
    assert rm.add(*mm.flatten(rseqs[:2])) + rm.add(*mm.flatten(rseqs[2:]), id_base=2) == model.max
    n1, n2, nM = rm.pack()
    got = rm.export()
    for k, exp in (("index", model.index), ("offset", model.offset), ("id", model.id), ("depth", model.depth_arr), ("rev", model.rev), ("loc", model.loc)):
        assert np.array_equal(got[k], np.array(exp, np.uint32)), k
    ex = ms.export()
    assert not ex[2].any() and np.array_equal(ex[3], np.array(model.ms.info, np.uint8))
    assert (n1, n2, nM) == tuple(int(c) for c in np.bincount(np.array(model.ms.info[1:]) & 3, minlength=4)[1:])
    res = rm.query(*mm.flatten(qseqs), seeds=True)
    for q, (name, s) in enumerate(zip(qnames, qseqs)):
        ev = model.query(name, s, False)
        c = res["counts"][q]
        assert ev[0][1] == "Q\t%s\t%d\t%d miss, %d copy1, %d copy2, %d multi, %s hit\n" % (name, len(s), c[0], c[1], c[2], c[3], mp.c_ratio(int(c[1] + c[2] + c[3]), int(c.sum())))
        recs = res["recs"][int(res["rec_start"][q]):int(res["rec_start"][q + 1])]
        lines = ["M\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d %d\t%s\t%s\n" % (name, r["pos0"], r["posN"], len(s), model.dict.names[model.id[r["loc0"]] + 1], model.offset[r["loc0"]],
                                                                  model.offset[r["locN"]], r["n1"], r["n2"], mp.c_ratio(int(r["n1"] + r["n2"]), abs(int(r["locN"]) - int(r["loc0"]))),
                                                                  mp.c_ratio(int(r["n1"]), int(c[1]))) for r in recs]
        assert lines == [ln for _, ln in ev[1:]], name
        assert (recs["query"] == q).all()
        assert int(res["seed_start"][q + 1] - res["seed_start"][q]) == int(c.sum())
    # -r through RefMap.from_arrays: the same arrays over the set read back give the same answers
    ms2 = hash10x_amd.MoshSet.from_arrays(20, 19, 31, model.ms.factor1, model.ms.factor2, *ms.export())
    rm2 = hash10x_amd.RefMap.from_arrays(ms2, *[got[k] for k in ("index", "offset", "id", "depth", "rev", "loc")], n_ids=3)
    res2 = rm2.query(*mm.flatten(qseqs), seeds=True)
    for k in res:
        assert np.array_equal(res[k], res2[k]), k
    with pytest.raises(hash10x_amd.Hash10xError, match="is on sequence 2 of 2"):
        hash10x_amd.RefMap.from_arrays(ms2, *[got[k] for k in ("index", "offset", "id", "depth", "rev", "loc")], n_ids=2)
    ms2.close(); rm2.close()                                   # the wrong order: the map's handle is forgotten, not released through a freed set
    rm.close(); ms.close()


# ---- the scan's second attempt (tests/gap_cases.py): a reference sequence and a query with a 100 kb run of N, A or T ---------------------
GAPPED = "-B 20 -f ref.fa -w r -q q.fa".split()


def gap_case(d, fill):
    """ref.fa: the gapped sequence and 30 kb of random sequence; q.fa: a query that holds the run, three that span a flank (one reversed, one
    ending in the run) and one from the second reference sequence"""
    left, gapped, right = gap_seqs(fill)
    B = np.array(list("ACGT"))
    other = "".join(B[np.random.RandomState(7).randint(0, 4, 30000)])
    refs = [gapped, other]
    qs = [gapped[15000:FLANK_END(gapped) + 6000], left[2000:9000], right[3000:15000].translate(COMP)[::-1], gapped[18000:20600], other[100:8000]]
    write_fa(os.path.join(d, "ref.fa"), refs, ["chrG", "chrO"]); write_fa(os.path.join(d, "q.fa"), qs, ["q%d" % i for i in range(len(qs))])
    return refs, qs


def FLANK_END(gapped):
    return len(gapped) - 20000                                    # where the right flank starts


@pytest.mark.parametrize("fill", ["N", "A", "T", None], ids=["N", "A", "T", "control"])
def test_gapped_reference_and_query(fill, tmp_path):
    """-f of a reference sequence and -q of a query that list more moshes than the estimate: text, .mosh and .ref equal the model's with and without
    --slab 3000 (every sequence alone); through RefMap the set's scan_retries rises by two for the reference batch (-f scans a batch twice: find-or-add, which
    counts found hashes in acc[], then the ordered list) and by one for the query batch"""
    import hash10x_amd
    dm = os.path.join(str(tmp_path), "model"); os.makedirs(dm)
    refs, qs = gap_case(dm, fill)
    st, out, err = mp.run_commands(GAPPED, dm)
    assert st == 0, err
    k, w = 19, 31
    model = mm.MoshModel(20, k, w, 17)
    listed = [len(model.moshes(to_codes(s))[0]) for s in (refs[0], qs[0])]
    if fill:
        assert listed[0] > scan_cap([len(s) for s in refs], k, w) and listed[1] > scan_cap([len(s) for s in qs], k, w) and min(listed) > GAP - k
    else:
        assert max(listed) < 6000
    for slab in (0, 3000):
        d = os.path.join(str(tmp_path), "slab%d" % slab); os.makedirs(d)
        for n in ("ref.fa", "q.fa"):
            os.link(os.path.join(dm, n), os.path.join(d, n))
        r = run((["--slab", slab] if slab else []) + GAPPED, d)
        assert r.returncode == 0, r.stderr.decode()
        gout, gerr = mm.mask_lines(r.stdout), mm.mask_lines(r.stderr)
        if slab:
            gout.remove("user")
            gerr = [ln for ln in gerr if not ln.startswith("COMMAND --slab")]
        assert gerr == mm.mask_lines(err.encode())
        assert gout == mm.mask_lines(out.encode())
        for n in ("r.mosh", "r.ref"):
            with open(os.path.join(d, n), "rb") as f, open(os.path.join(dm, n), "rb") as g:
                assert mp.mask_file(n, f.read()) == mp.mask_file(n, g.read()), "%s (slab %d)" % (n, slab)
        ms = hash10x_amd.MoshSet(B=20)
        if slab:
            ms.set_option("mosh_slab", slab)
        rm = hash10x_amd.RefMap(ms)
        rm.add(*mm.flatten([to_codes(s) for s in refs]))
        assert ms.counters()["scan_retries"] == (2 if fill else 0)
        rm.pack()
        ref_model = mp.RefModel.from_bytes(mm.MoshModel.from_bytes(open(os.path.join(dm, "r.mosh"), "rb").read()), open(os.path.join(dm, "r.ref"), "rb").read())
        got = rm.export()
        for key, exp in (("index", ref_model.index), ("offset", ref_model.offset), ("id", ref_model.id), ("rev", ref_model.rev), ("loc", ref_model.loc)):
            assert np.array_equal(got[key], np.array(exp, np.uint32)), key
        res = rm.query(*mm.flatten([to_codes(s) for s in qs]))
        assert ms.counters()["scan_retries"] == (3 if fill else 0)
        qlines = [ln for ln in out.splitlines() if ln.startswith("Q\t")]
        for q, s in enumerate(qs):
            c = res["counts"][q]
            assert qlines[q] == "Q\tq%d\t%d\t%d miss, %d copy1, %d copy2, %d multi, %s hit" % (q, len(s), c[0], c[1], c[2], c[3], mp.c_ratio(int(c[1] + c[2] + c[3]), int(c.sum())))
        rm.close(); ms.close()


# ---- (c) limits and misuse ---------------------------------------------------------------------------------------------------------------
def golden_reference():
    names, seqs = mp.parse_fasta(mp.gold("in/ref.fa"))
    return mm.flatten(seqs)


def test_reference_size_overflow():
    import hash10x_amd
    ms = hash10x_amd.MoshSet(B=20)
    rm = hash10x_amd.RefMap(ms, size=100)
    with pytest.raises(hash10x_amd.Hash10xError, match="^reference size overflow$"):
        rm.add(*golden_reference())
    rm.close(); ms.close()


def test_set_depths_stay_zero_and_table_is_the_references():
    """after the -f loop the set's 16-bit depth[] is all 0 (moshmap.c never touches it) and its probe table is the golden .mosh's"""
    import hash10x_amd
    ms = hash10x_amd.MoshSet(B=20)
    rm = hash10x_amd.RefMap(ms)
    rm.add(*golden_reference())
    rm.pack()
    index, value, depth, info = ms.export()
    gold = mm.MoshModel.from_bytes(mp.gold("build.idx.mosh"))
    assert not depth.any()
    assert np.array_equal(index, gold.file_index)
    assert np.array_equal(value[1:], np.array(gold.value[1:], np.uint64)) and np.array_equal(info, np.array(gold.info, np.uint8))
    rm.close(); ms.close()


def test_refmap_misuse():
    import hash10x_amd
    ms = hash10x_amd.MoshSet(B=20)
    with pytest.raises(hash10x_amd.Hash10xError, match="refCreate must have size > 0"):
        hash10x_amd.RefMap(ms, size=0)
    used = hash10x_amd.MoshSet(B=20)                               # a set with depths of its own is not one to build a reference over
    used.add(*golden_reference())
    with pytest.raises(hash10x_amd.Hash10xError, match="has a depth: a reference is built over a set whose depths are all 0"):
        hash10x_amd.RefMap(used)
    assert used.export(index=False)[2].any()
    used.close()
    rm = hash10x_amd.RefMap(ms)
    codes, start = golden_reference()
    with pytest.raises(hash10x_amd.Hash10xError, match="not packed"):
        rm.query(codes, start)
    with pytest.raises(hash10x_amd.Hash10xError, match="not packed"):
        rm.export()
    rm.add(codes, start)
    rm.pack()
    with pytest.raises(hash10x_amd.Hash10xError, match="is packed"):
        rm.add(codes, start)
    with pytest.raises(hash10x_amd.Hash10xError, match="is packed"):
        rm.pack()
    rm.close(); ms.close()


def test_write_before_reference(tmp_path):
    r = run(["-w", "x"], str(tmp_path))
    assert r.returncode == 255 and r.stderr.decode().splitlines()[-1] == "FATAL ERROR: -w needs a reference: give -f or -r first"
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("name,data,message", mp.bad_refs(), ids=[b[0] for b in mp.bad_refs()])
def test_malformed_ref_file(name, data, message, tmp_path):
    d = str(tmp_path)
    with open(os.path.join(d, "bad.mosh"), "wb") as f:
        f.write(mp.gold("build.idx.mosh"))
    with open(os.path.join(d, "bad.ref"), "wb") as f:
        f.write(data)
    r = run(["-r", "bad", "-q", "nosuch.fa"], d)
    last = r.stderr.decode().splitlines()[-1]
    assert r.returncode == 255 and last.startswith("FATAL ERROR: ") and message in last, last


def test_ref_file_against_another_set(tmp_path):
    """a .ref beside the .mosh of other parameters: depth[] and loc[] have another length, so nothing lines up"""
    d = str(tmp_path)
    with open(os.path.join(d, "bad.mosh"), "wb") as f:
        f.write(mp.gold("params.p.mosh"))
    with open(os.path.join(d, "bad.ref"), "wb") as f:
        f.write(mp.gold("build.idx.ref"))
    r = run(["-r", "bad"], d)
    assert r.returncode == 255 and r.stderr.decode().splitlines()[-1].startswith("FATAL ERROR: ")


@pytest.mark.parametrize("to", [2, 0])
def test_copy_classes_must_fit_the_reference(to, tmp_path):
    """a set whose info says copy 2 for an index the .ref holds once is refused, since the query pass would read rev[] past that index's hits;
    so is one with copy class 0, which -f never leaves and the reference would walk as copy 2"""
    d = str(tmp_path)
    mosh = bytearray(mp.gold("build.idx.mosh"))
    ms = mm.MoshModel.from_bytes(bytes(mosh))
    i = ms.info.index(1)
    mosh[len(mosh) - len(ms.info) + i] = to
    with open(os.path.join(d, "bad.mosh"), "wb") as f:
        f.write(bytes(mosh))
    with open(os.path.join(d, "bad.ref"), "wb") as f:
        f.write(mp.gold("build.idx.ref"))
    r = run(["-r", "bad"], d)
    assert r.returncode == 255
    assert r.stderr.decode().splitlines()[-1] == "FATAL ERROR: mosh index %d: its copy class in the set is 0 or asks for more hits than the reference holds for it" % i


if __name__ == "__main__":
    if len(sys.argv) == 7 and sys.argv[1] == "gen":
        os.makedirs(sys.argv[2], exist_ok=True)
        gen_case(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[5]), int(sys.argv[6]))
    else:
        sys.exit(__doc__)
