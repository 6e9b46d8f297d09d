"""The sequence spectrum without a GPU: the plain-Python model of the definition (tests/seqspectrum_model.py) held to the properties the definition
gives (through the --seqBlocks and --seqSpans models), the scripted cases' own claims (tests/seqspectrum_cases.py), read_seq_spectrum and its
refusals, and the .sp writer under AddressSanitizer + UBSan behind a main of its own. Every comparison is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import orc
import seqblocks_cases as sbc
import seqblocks_model as sbm
import seqspans_model as ssm
import seqspectrum_cases as cases
import seqspectrum_model as spm

K = cases.K
F = spm.FIELDS


@pytest.fixture(scope="module")
def scripted():
    return cases.script()


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    recs = sbc.small_records()
    o = orc.Oracle(k=sbc.K, w=sbc.W, seed=sbc.R, B=20)
    o.read_fqb(recs)
    p = str(tmp_path_factory.mktemp("sp") / "small.hash")
    o.write_hash(p)
    o.close()
    sb = sbm.SeqBlocksModel.from_hash_file(orc.HashFile(open(p, "rb").read()), [sbc.SMALL_RANGE])
    return spm.SeqSpectrumModel(ssm.SeqSpansModel(sb)), [s for s, _ in sbc.sequences(recs)], sbc.SMALL_RANGE


def _properties(m, seqs, thresholds, w, rng):
    """properties 1 - 8 of the definition on one state"""
    c1, c2, cm = thresholds
    (figs, off, win, s, totals), copies, info = m.seq_spectrum(seqs, c1, c2, cm, w)
    found = 0
    for i, q in enumerate(seqs):
        moshes, fnd = m.ss.sb.query(q)[1][:2]                                            # 1: moshes and found of seq_hashes ..
        assert (int(figs["moshes"][i]), int(figs["moshes"][i]) - int(figs["absent"][i])) == (moshes, fnd)
        assert m.ss.hits(q)[1][:2] == (moshes, fnd)                                      # .. and of seq_spans
        found += fnd
        a, b = int(off[i]), int(off[i + 1])
        assert b - a == -(-len(q) // w)
        for k in F:                                                                      # 2: the windows sum field by field
            assert int(win[k][a:b].astype(np.uint64).sum()) == int(figs[k][i]), (i, k)
    assert int(copies.sum()) == found and copies[0] == 0                                 # 3
    assert int(s.sum()) == m.hash_number - 1 == int(totals[0].sum())                     # 4, 5
    rc = [sbm.revcomp(q) for q in seqs]                                                  # 6
    (rfigs, _, _, rs, rtotals), rcopies, _ = m.seq_spectrum(rc, c1, c2, cm, w)
    assert rfigs.tobytes() == figs.tobytes() and np.array_equal(rcopies, copies) and np.array_equal(rs, s) and np.array_equal(rtotals, totals)
    assert np.array_equal(m.copies(list(seqs) + list(seqs)), 2 * copies)                 # 7
    lo, hi = rng                                                                         # 8: n2 at (lo, lo, hi) is the inRange figure of seq_spans
    n2 = m.seq_spectrum(seqs, lo, lo, hi)[0][0]["n2"]
    assert n2.tolist() == [m.ss.hits(q)[1][2] for q in seqs] and int(n2.sum()) > 0
    return info


def test_properties_on_scripted(scripted):
    z, _, m = scripted
    info = _properties(m, cases.sequences(z), (cases.C1, cases.C2, cases.CM), cases.WIN, cases.RANGE)
    assert min(info[k] for k in ("absent", "n0", "n1", "n2", "nM")) > 0


def test_properties_on_small(small):
    m, seqs, rng = small
    info = _properties(m, seqs, (3, 6, 10), 40, rng)                                     # (the deepest hash of the set has depth 12)
    assert min(info[k] for k in ("absent", "n0", "n1", "n2", "nM")) > 0 and info["maxCopies"] >= 2


# ------------------------------------------------------------------------------------ the scripted cases: each states the edge it hits and asserts it from the model
def test_class_and_bin_edges(scripted):
    z, _, m = scripted
    occ = m.occurrences(z.seqs["cls"])
    assert [p for p, _ in occ] == sorted(p for p, _ in occ)                              # (the oracle lists them by position, as the script numbers them)
    depths = [int(m.depth[x]) for _, x in occ[:9]]
    assert tuple(depths) == cases.CLS_DEPTHS and all(x == 0 for _, x in occ[9:]) and len(occ) > 12
    rec = {t: m.record(occ, *t) for t in cases.threshold_sets()}
    n, absent = len(occ), len(occ) - 9
    assert rec[(3, 6, 10)] == (n, absent, 1, 2, 2, 4, sum(depths))                       # c - 1 below, c at each of the three thresholds
    assert rec[(3, 3, 10)] == (n, absent, 1, 0, 4, 4, sum(depths)) and rec[(3, 10, 10)] == (n, absent, 1, 4, 0, 4, sum(depths))
    assert rec[(0, 0, 0)] == (n, absent, 0, 0, 0, 9, sum(depths)) and rec[(5000, 5000, 5000)] == (n, absent, 9, 0, 0, 0, sum(depths))
    s = m.seq_spectrum([z.seqs["cls"]], 3, 6, 10)[0][3]
    assert s[1022].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and s[1023].tolist() == [0, 2, 0, 0, 0, 0, 0, 0]   # 1023 and 1024 share the last bin
    hf = orc.HashFile(scripted[1])
    assert int(hf.blocks["nHash"][cases.B_HEAVY]) == cases.ssc.HEAVY_RECORDS and max(int(hf.blocks["nHash"][b]) for b in range(1, cases.B_HEAVY)) <= 1100


def test_copies_edges(scripted):
    z, _, m = scripted
    x = m.occurrences(z.seqs["rep7"])[z.rep][1]
    assert x and int(m.depth[x]) == 4
    for names, n in ((["rep7"], 7), (["rep7", "rep8"], 8), (["rep7", "rep8", "rep9"], 9), (z.names, 9)):
        (_, _, _, s, _), copies, info = m.seq_spectrum(cases.sequences(z, names), cases.C1, cases.C2, cases.CM)
        assert int(copies[x]) == n == info["maxCopies"] and int(s[4, 7]) == 1            # 7, 8 and 9 stand in the last column; copies[] is not clipped
        assert int(s[:, 7].sum()) == 1


def test_window_edges(scripted):
    z, _, m = scripted
    t = (cases.C1, cases.C2, cases.CM)
    count = lambda name, w: len(m.windows(z.seqs[name], *t, w))   # noqa: E731
    W = cases.WIN
    assert [len(z.seqs[n]) for n in ("main", "even", "short", "k-1", "empty")] == [2 * W + 1, 2 * W, W - 1, K - 1, 0]
    assert [count(n, W) for n in ("main", "even", "short", "k-1", "empty")] == [3, 2, 1, 1, 0]
    assert m.windows(z.seqs["main"], *t, W)[2] == (0,) * 7 and m.windows(z.seqs["k-1"], *t, W) == [(0,) * 7]   # p <= L - k: the last window is empty
    u = z.unit
    b = z.pos("main", u + 1)
    assert z.pos("main", u) == b - 1 and b in cases.windows(z)
    win = m.windows(z.seqs["main"], *t, b)
    assert win[0][0] == u + 1 and win[1][0] >= 1 and sum(w[0] for w in win) == len(z.occ["main"])   # the boundary lies between the two
    assert [count(n, 10 ** 6) for n in z.names] == [0 if n == "empty" else 1 for n in z.names]      # W > L
    assert m.windows(z.seqs["s65"], *t, 10000)[0][0] == len(z.occ["s65"]) >= 65 and m.windows(z.seqs["s257"], *t, 10000)[0][0] == len(z.occ["s257"]) >= 257
    one = m.windows(z.seqs["w1"], *t, 1)                                                 # W = 1: a window per base
    assert len(one) == 100 and [i for i, w in enumerate(one) if w[0]] == [p for p, _ in z.occ["w1"]] and one[z.pos("w1", 0)] == (1, 0, 0, 0, 1, 0, cases.C2)
    assert m.windows(z.seqs["main"], *t, 0) == [] and m.seq_spectrum(cases.sequences(z), *t, 0)[0][1].tolist() == [0] * (len(z.names) + 1)


# ------------------------------------------------------------------------------------ read_seq_spectrum
def test_read_seq_spectrum(scripted, tmp_path):
    hx = orc.hx()
    z, _, m = scripted
    seqs, names = cases.sequences(z), list(z.names)
    t = (cases.C1, cases.C2, cases.CM)
    result, copies, _ = m.seq_spectrum(seqs, *t, cases.WIN)
    good = spm.sp_bytes(m.hash_number, *t, cases.WIN, result, copies, names)
    p = tmp_path / "x.sp"
    p.write_bytes(good)
    info, figs, off, win, s, totals, held, rnames = hx.read_seq_spectrum(str(p))
    assert info == {"version": 1, "hashNumber": m.hash_number, "copy1min": t[0], "copy2min": t[1], "copyMmin": t[2], "window": cases.WIN, "depthBins": 1024,
                    "copyBins": 8, "nSeq": len(names), "windows": len(result[2]), "nameBytes": sum(len(n) + 1 for n in names)}
    assert figs.tobytes() == result[0].tobytes() and win.tobytes() == result[2].tobytes() and np.array_equal(off, result[1])
    assert s.dtype == np.uint64 and s.shape == (1024, 8) and np.array_equal(s, result[3]) and np.array_equal(totals, result[4])
    assert held.dtype == np.uint8 and np.array_equal(held, np.minimum(copies, 255)) and rnames == names

    def refused(data, what):
        p.write_bytes(data)
        with pytest.raises(hx.Hash10xError, match=what):
            hx.read_seq_spectrum(str(p))

    figs, off, win, s, totals = result
    variant = lambda **kw: spm.sp_bytes(m.hash_number, *kw.pop("t", t), kw.pop("w", cases.WIN), kw.pop("result", result), kw.pop("copies", copies), names, **kw)   # noqa: E731
    refused(variant(magic=b"10XE"), "not a seq spectrum file")
    refused(variant(version=2), "version 2")
    refused(variant(bins=(1024, 16)), "bins")
    refused(good + b"\0", "need")
    refused(good[:-1], "need")
    refused(variant(zero=1), "reserved word")
    refused(variant(t=(3, 2, 10)), "do not ascend")
    bad = off.copy(); bad[1] += 1
    refused(variant(result=(figs, bad, win, s, totals)), "window offsets")
    refused(variant(w=cases.WIN + 1), "window offsets")
    bad = win.copy(); bad["absent"][0] += 1
    refused(variant(result=(figs, off, bad, s, totals)), "a window's moshes")
    bad = figs.copy(); bad["n1"][0] += 1
    refused(variant(result=(bad, off, win, s, totals)), "a sequence's moshes")
    bad = win.copy(); bad["depthSum"][0] += 1
    refused(variant(result=(figs, off, bad, s, totals)), "do not sum to its depthSum")
    bad = win.copy(); bad["n0"][0] += 1; bad["moshes"][0] += 1
    refused(variant(result=(figs, off, bad, s, totals)), "do not sum to its moshes")
    bad = s.copy(); bad[0, 0] += 1
    refused(variant(result=(figs, off, win, bad, totals)), "do not sum to the")
    bad = s.copy(); bad[1, 0] -= 1; bad[7, 0] += 1                                      # a hash moved from class 0 to class 2
    refused(variant(result=(figs, off, win, bad, totals)), "totals of class 0")
    bad = totals.copy(); bad[1, 1] = bad[0, 1] + 1
    refused(variant(result=(figs, off, win, s, bad)), "more hashes of a class are present")
    x = int(np.flatnonzero(copies == 1)[0])
    bad = copies.copy(); bad[x] = 0
    refused(variant(copies=bad), "copies are not those of the spectrum")
    bad = copies.copy(); bad[0] = 1
    refused(variant(copies=bad), "byte 0")
    bad = figs.copy(); bad["absent"][1] += 1; bad["moshes"][1] += 1
    wbad = win.copy(); wbad["absent"][int(off[1])] += 1; wbad["moshes"][int(off[1])] += 1
    p.write_bytes(variant(result=(bad, off, wbad, s, totals)))                         # one more absent occurrence ties to nothing else: accepted ..
    assert int(hx.read_seq_spectrum(str(p))[1]["absent"][1]) == int(figs["absent"][1]) + 1
    bad = figs.copy(); bad["nM"][1] += 1; bad["moshes"][1] += 1
    wbad = win.copy(); wbad["nM"][int(off[1])] += 1; wbad["moshes"][int(off[1])] += 1
    refused(variant(result=(bad, off, wbad, s, totals)), "the copies sum to")
    refused(good[:-1] + b"x", "does not end in NUL")


def test_qv_and_completeness():
    hx = orc.hx()
    assert hx.seq_qv(0, 0, 21) == 0.0 and hx.seq_qv(10, 0, 21) == float("inf") and "%.2f" % hx.seq_qv(10, 10, 21) == "0.00"
    assert abs(hx.seq_qv(1000, 21, 21) - 30.0) < 0.05                                    # one unsupported k-mer in a thousand: about one wrong base in a thousand
    assert spm.qv(331, 70, 21) == hx.seq_qv(331, 70, 21)
    assert spm.completeness(np.array([[5, 4, 0, 4], [5, 1, 0, 3]], dtype=np.uint64)) == 50.0 and spm.completeness(np.zeros((2, 4), np.uint64)) == 0.0


def test_usage_names_seq_spectrum():
    p = subprocess.run([os.path.join(orc.REPO, "bin", "hash10x-amd"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--seqSpectrum <copy1min> <copy2min> <copyMmin> <window> <sequence file> <sp output>" in p.stderr


# ------------------------------------------------------------------------------------ the .sp writer under ASan + UBSan (a program of its own, on the CPU)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:exitcode=67")


def _driver_window(q, j, hash_number):
    absent = (q + j) % 2
    n = ((q + j) % 3, j % 2, q % 2, (q * j) % 2) if hash_number > 1 else (0, 0, 0, 0)
    return (absent + sum(n), absent) + n + (3 * sum(n),)


@pytest.mark.parametrize("n_seq, per, slabs, hash_number", [(0, 0, 0, 1), (1, 0, 1, 2), (10, 3, 4, 1000), (9, 3, 3, 1), (100, 7, 15, 2), (5, 0, 1, (1 << 22) + 3)])
def test_sp_writer_under_sanitizers(tmp_path, n_seq, per, slabs, hash_number):
    import hash10x_amd
    drv = os.path.join(orc.REPO, "build", "sp-host-asan")
    if not os.path.exists(drv):
        subprocess.run(["make", "-C", os.path.join(orc.REPO, "hash10x_amd", "host"), "../../build/sp-host-asan"], check=True, stdout=subprocess.DEVNULL)
    p = str(tmp_path / "w.sp")
    r = subprocess.run([drv, p, str(n_seq), str(per), str(hash_number)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    assert r.returncode == 0 and b"failed to open output file" in r.stdout, (r.stdout, r.stderr)
    assert os.listdir(str(tmp_path)) == ["w.sp"]                                     # no .part, nothing of the failing runs; the old bytes kept
    # what the driver is documented to write
    wins = [[_driver_window(q, j, hash_number) for j in range(-(-(10 * q + 1) // 4))] for q in range(n_seq)]
    flat = [w for ws in wins for w in ws]
    figs = [(10 * q + 1,) + tuple(sum(w[i] for w in ws) for i in range(7)) for q, ws in enumerate(wins)]
    found = sum(w[0] - w[1] for w in flat)
    hashes = hash_number - 1
    x = np.arange(hash_number, dtype=np.int64)
    copies = np.zeros(hash_number, dtype=np.int64)
    if hashes:
        copies[1:] = found // hashes + (x[1:] <= found % hashes)
    depth = np.where(x % 500 == 499, 2000, x % 9)
    spectrum = np.zeros((1024, 8), dtype=np.uint64)
    np.add.at(spectrum, (np.minimum(depth[1:], 1023), np.minimum(copies[1:], 7)), 1)
    q = (depth[1:] >= 2).astype(np.int64) + (depth[1:] >= 4) + (depth[1:] >= 6)
    totals = np.stack([np.bincount(q, minlength=4), np.bincount(q[copies[1:] >= 1], minlength=4)]).astype(np.uint64)
    info, rfigs, off, win, s, rtotals, held, names = hash10x_amd.read_seq_spectrum(p)
    assert info == {"version": 1, "hashNumber": hash_number, "copy1min": 2, "copy2min": 4, "copyMmin": 6, "window": 4, "depthBins": 1024, "copyBins": 8,
                    "nSeq": n_seq, "windows": len(flat), "nameBytes": sum(len("s%d" % i) + 1 for i in range(n_seq))}
    assert names == ["s%d" % i for i in range(n_seq)] and [tuple(int(v) for v in r) for r in rfigs.tolist()] == figs
    assert [tuple(int(v) for v in r) for r in win.tolist()] == flat and off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in wins])]).tolist()
    assert np.array_equal(s, spectrum) and np.array_equal(rtotals, totals) and np.array_equal(held, np.minimum(copies, 255))
    moshes, absent, n0 = (sum(w[i] for w in flat) for i in (0, 1, 2))
    tail = "%d slabs, %d windows, %d moshes, %d absent, %d found, present %d of %d, QV %.2f\n" % (
        slabs, len(flat), moshes, absent, found, int(totals[1].sum()), hashes, spm.qv(moshes, absent + n0, 21))
    assert tail.encode() in r.stdout, r.stdout[-400:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("SEQ_SPECTRUM  ")]
    assert lines == ["SEQ_SPECTRUM  s%d len %d moshes %d absent %d copy0 %d copy1 %d copy2 %d copyM %d meanDepth %.1f QV %.2f" % (
        (i,) + f[:7] + (f[7] / (f[1] - f[2]) if f[1] > f[2] else 0.0, spm.qv(f[1], f[2] + f[3], 21))) for i, f in enumerate(figs)]
