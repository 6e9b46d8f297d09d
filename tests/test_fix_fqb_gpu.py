"""--codeCensus, --fixFQB and --fixFQBThresh on the GPU (csrc/stage_j.hip) against the reference's `fq2b -10x` (recorded under
tests/golden/fixfqb and run fresh from oracle/_ref/fq2b) and against the numpy model of tests/fqb_model.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fqb_model as fm
import orc

pytestmark = pytest.mark.gpu
EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
needs_fq2b = pytest.mark.skipif(not os.path.exists(fm.FQ2B_REF), reason="oracle/_ref/fq2b not present")


def run(args, cwd, limit=120):
    return subprocess.run([EXE] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)


def read_lines(n, name):
    return b"read %d barcodes from file %s\n" % (n, name.encode())


@pytest.fixture(scope="module")
def fresh(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fixfqb"))
    case = fm.fresh_case(d)
    case["dir"] = d
    return case


@pytest.fixture(scope="module")
def shapes():
    recs, good = fm.synthetic_records(70001, 3000, 21)
    T = 4
    codes, counts, g = fm.census(recs, T)
    out, st = fm.fix(recs, g)
    return {"recs": recs, "T": T, "codes": codes, "counts": counts, "good": g, "out": out, "stats": st, "planted": good}


def test_golden(tmp_path):
    for f in ("raw.fqb", "goodcodes.txt"):
        shutil.copy(os.path.join(fm.GOLDEN, f), tmp_path / f)
    g = run(["--fixFQB", "goodcodes.txt", "raw.fqb", "out.fqb"], tmp_path)
    assert g.returncode == 0, g.stderr.decode()
    assert (tmp_path / "out.fqb").read_bytes() == open(os.path.join(fm.GOLDEN, "fixed.fqb"), "rb").read()
    assert g.stderr == open(os.path.join(fm.GOLDEN, "fixed.stderr.txt"), "rb").read()


@needs_fq2b
@pytest.mark.parametrize("T", fm.FRESH_T)
def test_fresh_against_reference(fresh, T):
    d, ref = fresh["dir"], fresh[T]
    g = run(["--codeCensus", T, "raw.fqb", "hip%d.txt" % T], d)
    assert g.returncode == 0, g.stderr.decode()
    assert open(os.path.join(d, "hip%d.txt" % T)).read() == fm.text(ref["codes"])
    recs = np.frombuffer(fresh["raw"], dtype=np.uint32).reshape(-1, 30)
    codes, counts, good = fm.census(recs, T)
    line = "  4000 records, %d distinct barcodes, %d good barcodes (at least %d records) holding %d records\n" % (codes.size, good.size, T, counts[counts >= T].sum())
    assert line.encode() in g.stdout
    g = run(["--fixFQB", ref["good"], "raw.fqb", "a%d.fqb" % T], d)
    assert g.returncode == 0, g.stderr.decode()
    assert open(os.path.join(d, "a%d.fqb" % T), "rb").read() == ref["bytes"] and g.stderr == ref["stderr"]
    g = run(["--fixFQBThresh", T, "raw.fqb", "b%d.fqb" % T], d)
    assert g.returncode == 0, g.stderr.decode()
    assert open(os.path.join(d, "b%d.fqb" % T), "rb").read() == ref["bytes"]
    first, rest = g.stderr.split(b"\n", 1)
    assert first == b"found %d barcodes with at least %d records in raw.fqb" % (good.size, T)
    assert rest == ref["stderr"].split(b"\n", 1)[1]


@needs_fq2b
def test_whitelist_in_file_order(tmp_path):
    wl = fm.shadow_whitelist(np.random.default_rng(5))
    fm.write_fastq_for_whitelist(str(tmp_path), wl, 900, 6)
    (tmp_path / "wl.txt").write_text("\n".join(wl) + "\n")
    fm.run_fq2b_ref(str(tmp_path), "raw.fqb")
    exp, err = fm.run_fq2b_ref(str(tmp_path), "ref.fqb", "wl.txt")
    g = run(["--fixFQB", "wl.txt", "raw.fqb", "hip.fqb"], tmp_path)
    assert g.returncode == 0, g.stderr.decode()
    assert (tmp_path / "hip.fqb").read_bytes() == exp and g.stderr == err


@pytest.mark.parametrize("slab", [1000, 4096, 0])
def test_shapes(shapes, slab, tmp_path):
    """70 001 records (no multiple of 256 or 1024, several scan tiles), about 3000 good barcodes with all-A and all-T among them,
    good codes one substitution apart, records with several good neighbours, records two substitutions away: census, fix and the
    file command equal the model whatever the batch size"""
    import hash10x_amd
    s = shapes
    assert 0 in s["good"] and 0xFFFFFFFF in s["good"] and 2500 < s["good"].size < 3500 and s["stats"]["dropped"] > 5000
    cand = fm.candidates(s["recs"][:, 0])
    assert (np.isin(cand, s["good"]).sum(axis=1) >= 2).sum() > 100
    gs = np.sort(s["good"])
    assert np.isin(fm.candidates(gs)[:, 1:], gs).any()
    h = hash10x_amd.Hash10x(B=20)
    h.set_option("fqb_slab", slab)
    codes, counts, good = h.code_census(s["recs"], s["T"])
    assert np.array_equal(codes, s["codes"]) and np.array_equal(counts, s["counts"]) and np.array_equal(good, s["good"])
    out, st = h.fix_fqb(s["recs"])
    assert st == s["stats"]
    assert out.shape == s["out"].shape and np.array_equal(out, s["out"])
    s["recs"].tofile(tmp_path / "in.fqb")
    rc = h._host.h10x_session_fixFQBThresh(h._s, s["T"], os.fsencode(str(tmp_path / "in.fqb")), os.fsencode(str(tmp_path / "out.fqb")), None)
    assert rc == 0, h._host.h10x_session_error(h._s)
    assert (tmp_path / "out.fqb").read_bytes() == s["out"].tobytes()
    h.close()


def test_large_whitelist():
    """300 000 random codes (with repeats) through set_whitelist, 5000 records: the table is loaded and its slots collide"""
    import hash10x_amd
    rng = np.random.default_rng(31)
    wl = rng.integers(0, 1 << 32, 300000, dtype=np.uint64).astype(np.uint32)
    wl[1000:1100] = wl[:100]                                                           # repeated lines
    wl[2000:2100] = wl[100:200] ^ np.uint32(1 << 6)                                    # neighbours listed after the code they shadow
    pick = wl[rng.integers(0, wl.size, 5000)]
    u = rng.random(5000)
    one = rng.integers(1, 4, 5000).astype(np.uint32) << (2 * rng.integers(0, 16, 5000)).astype(np.uint32)
    recs = rng.integers(0, 1 << 32, (5000, 30), dtype=np.uint64).astype(np.uint32)
    recs[:, 0] = np.where(u < 0.4, pick ^ one, np.where(u < 0.6, recs[:, 0], pick))
    recs[:200, 0] = wl[100:300]
    exp, est = fm.fix(recs, wl)
    assert est["dropped"] > 500 and est["corrected"] > 1000
    h = hash10x_amd.Hash10x(B=20)
    h.set_whitelist(wl)
    out, st = h.fix_fqb(recs)
    assert st == est and np.array_equal(out, exp)
    h.close()


def test_edges(tmp_path):
    rng = np.random.default_rng(41)
    codes = rng.integers(0, 1 << 32, 20, dtype=np.uint64).astype(np.uint32)
    (tmp_path / "wl.txt").write_text(fm.text(codes))
    recs = rng.integers(0, 1 << 32, (300, 30), dtype=np.uint64).astype(np.uint32)
    recs[:, 0] = codes[rng.integers(0, 20, 300)]
    exp, est = fm.fix(recs, codes)
    assert est["dropped"] == 0 and est["corrected"] == 0                               # every record kept, none corrected
    zero = {"dropped": 0, "corrected": 0, "correctedAt": [0] * 16}
    (tmp_path / "empty.fqb").write_bytes(b"")
    recs.tofile(tmp_path / "all.fqb")
    recs[:1].tofile(tmp_path / "one.fqb")
    far = recs.copy()
    far[:, 0] ^= np.uint32(0x00050005)                                                 # two substitutions away from its own code
    fexp, fst = fm.fix(far, codes)
    assert fexp.shape[0] == 0 and fst["dropped"] == 300
    far.tofile(tmp_path / "far.fqb")
    for name, n_in, out, st in (("empty", 0, recs[:0], zero), ("one", 1, recs[:1], zero), ("all", 300, exp, est), ("far", 300, fexp, fst)):
        g = run(["--fixFQB", "wl.txt", name + ".fqb", name + ".out"], tmp_path)
        assert g.returncode == 0, g.stderr.decode()
        assert (tmp_path / (name + ".out")).read_bytes() == out.tobytes(), name
        assert g.stderr == read_lines(20, "wl.txt") + fm.stats_lines(out.shape[0], st), name
    assert b"(-nan%)" in fm.stats_lines(0, zero)                                        # as C prints 0 / 0
    g = run(["--fixFQBThresh", 1000, "all.fqb", "x.out"], tmp_path)                      # threshold above every count
    assert g.returncode == 255 and b"FATAL ERROR: no barcode occurs at least 1000 times in all.fqb" in g.stderr
    g = run(["--codeCensus", 0, "all.fqb", "x.txt"], tmp_path)
    assert g.returncode == 255 and b"FATAL ERROR: barcode threshold 0 must be at least 1" in g.stderr
    (tmp_path / "odd.fqb").write_bytes(b"\0" * 121)
    for args in (["--fixFQB", "wl.txt", "odd.fqb", "x.out"], ["--fixFQBThresh", 1, "odd.fqb", "x.out"], ["--codeCensus", 1, "odd.fqb", "x.txt"]):
        g = run(args, tmp_path)
        assert g.returncode == 255 and b"FATAL ERROR: odd.fqb: size 121 is not a multiple of the 120-byte record" in g.stderr
    g = run(["--fixFQB", "nosuch.txt", "all.fqb", "x.out"], tmp_path)
    assert g.returncode == 255 and g.stderr == b"FATAL ERROR: failed to open 10x whitelist file nosuch.txt\n\n"
    (tmp_path / "bad.txt").write_text("ACGTACGTACGTACGT\nACGT\n")
    g = run(["--fixFQB", "bad.txt", "all.fqb", "x.out"], tmp_path)
    assert g.returncode == 255 and g.stderr == b"FATAL ERROR: bad barcode line 2 in bad.txt: ACGT\n"


def test_chain(tmp_path):
    """fix, sort and read in one command line: the .hash of the model's fixed records, stably sorted on the byte-swapped word"""
    shutil.copy(os.path.join(fm.GOLDEN, "raw.fqb"), tmp_path / "raw.fqb")
    g = run(["--fixFQBThresh", 3, "raw.fqb", "fixed.fqb", "--sortFQB", "fixed.fqb", "sorted.fqb", "-B", 20, "--readFQB", "sorted.fqb", "--writeHash", "hip.hash"], tmp_path)
    assert g.returncode == 0, g.stderr.decode()
    raw = np.fromfile(tmp_path / "raw.fqb", dtype=np.uint32).reshape(-1, 30)
    fixed, _ = fm.fix(raw, fm.census(raw, 3)[2])
    assert (tmp_path / "fixed.fqb").read_bytes() == fixed.tobytes() == open(os.path.join(fm.GOLDEN, "fixed.fqb"), "rb").read()
    exp = fixed[np.argsort(fixed[:, 0].byteswap(), kind="stable")]
    assert (tmp_path / "sorted.fqb").read_bytes() == exp.tobytes()
    o = orc.Oracle(B=20); o.read_fqb(exp.reshape(-1)); o.write_hash(str(tmp_path / "orc.hash"))
    a, b = (tmp_path / "hip.hash").read_bytes(), (tmp_path / "orc.hash").read_bytes()
    assert a == b, orc.describe_diff(a, b)


def test_python_on_device_records(shapes):
    import hash10x_amd
    recs = shapes["recs"][:20001]
    T = 2
    codes, counts, good = fm.census(recs, T)
    wl = np.concatenate([good[::-1], good[:50]])                                        # descending, then repeats: line order matters
    exp, est = fm.fix(recs, wl)
    h = hash10x_amd.Hash10x(B=20)
    d = hash10x_amd.DeviceRecords(recs)

    def once():
        c, n, g = h.code_census(d, T)
        assert np.array_equal(c, codes) and np.array_equal(n, counts) and np.array_equal(g, good)
        out, st = h.fix_fqb(d)                                                          # the census's own whitelist: ascending
        e2, s2 = fm.fix(recs, good)
        assert st == s2 and np.array_equal(out.download(), e2)
        out.free()
        h.set_whitelist(wl)
        out, st = h.fix_fqb(d)
        assert st == est and out.n_records == exp.shape[0] and np.array_equal(out.download(), exp)
        out.free()

    once()
    before = hash10x_amd.alloc_stats()
    once()
    assert hash10x_amd.alloc_stats() == before
    d.free()
    h.close()
