"""The sequence spectrum on the GPU (csrc/stage_s.hip): Hash10x.seq_spectrum against the plain-Python model of the definition
(tests/seqspectrum_model.py) on the scripted cases (tests/seqspectrum_cases.py) and the golden `small` state; independence of "seq_slab" and of how
the sequences are split over add calls; the kept copies and their release; the refusals; the command line and the .sp file. Every comparison of
integers is exact equality."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import seqblocks_cases as sbc
import seqblocks_model as sbm
import seqspans_model as ssm
import seqspectrum_cases as cases
import seqspectrum_model as spm

pytestmark = pytest.mark.gpu

K = cases.K
T = (cases.C1, cases.C2, cases.CM)
_hx = orc.hx


def _rows(a):
    return [tuple(int(v) for v in r) for r in a.tolist()]


def _same(got, exp, what):
    figs, off, win, s, totals = got
    efigs, eoff, ewin, es, etotals = exp
    assert figs.dtype.names == efigs.dtype.names and _rows(figs) == _rows(efigs), (what, "figures")
    assert off.dtype == np.uint64 and np.array_equal(off, eoff), (what, "win_offsets")
    assert win.dtype.names == ewin.dtype.names and _rows(win) == _rows(ewin), (what, "windows")
    assert s.dtype == np.uint64 and s.shape == (1024, 8) and np.array_equal(s, es), (what, "spectrum")
    assert totals.dtype == np.uint64 and totals.shape == (2, 4) and np.array_equal(totals, etotals), (what, "totals")


def _check(h, seqs, prm, exp, what):
    result, copies, info = exp
    _same(h.seq_spectrum(seqs, *prm), result, (what,) + tuple(prm))
    got = h.seq_copies()
    assert got.dtype == np.uint32 and np.array_equal(got, copies), (what, prm, "copies")
    assert h.seq_spectrum_info == info, (what, prm)


@pytest.fixture(scope="module")
def scripted(tmp_path_factory):
    z, data, m = cases.script()
    p = tmp_path_factory.mktemp("sp") / "scripted.hash"
    p.write_bytes(data)
    h = _hx().Hash10x(B=20)
    h.read_hash(str(p))                                        # no depth range: the command needs none
    seqs = cases.sequences(z)
    exp = {prm: m.seq_spectrum(seqs, *prm) for prm in cases.params(z)}
    yield h, z, m, seqs, exp
    h.close()


def _run_all(h, seqs, exp, what):
    for prm, e in exp.items():
        _check(h, seqs, prm, e, what)


def test_cases_against_model(scripted):
    """the classes at their edges and the four other threshold sets, the depth bins 1022 .. 1024, every window case; on a state without a range"""
    h, z, m, seqs, exp = scripted
    _run_all(h, seqs, exp, "default")
    _run_all(h, seqs, exp, "twice in one process")
    sub = cases.sequences(z, ["w1", "k-1", "empty", "cls"])    # W = 1: a window per base
    _check(h, sub, T + (1,), m.seq_spectrum(sub, *T, 1), "W = 1")
    assert h.seq_spectrum_info["windows"] == 100 + (K - 1) + 2000
    text = ["".join("ACGT"[c] for c in s).encode() for s in seqs]   # text goes in as code arrays do
    _same(h.seq_spectrum(text, *T, cases.WIN), exp[T + (cases.WIN,)][0], "text")
    got = h.seq_spectrum([], *T, 10)
    assert len(got[0]) == 0 and got[1].tolist() == [0] and len(got[2]) == 0 and int(got[3].sum()) == m.hash_number - 1 and not h.seq_copies().any()


def test_copies(scripted):
    """one hash 7, 8 and 9 times: a segment repeated within one sequence and again in sequences that fall into other slabs; u32 beyond the clip"""
    h, z, m, seqs, exp = scripted
    x = m.occurrences(z.seqs["rep7"])[z.rep][1]
    for slab in (0, len(z.seqs["rep7"])):                      # (the second: rep8 and rep9 each in a slab of their own)
        h.set_option("seq_slab", slab)
        for names, n in ((["rep7"], 7), (["rep7", "rep8"], 8), (["rep7", "rep8", "rep9"], 9)):
            sub = cases.sequences(z, names)
            _check(h, sub, T + (0,), m.seq_spectrum(sub, *T, 0), (slab, n))
            assert int(h.seq_copies(x, 1)[0]) == n == h.seq_spectrum_info["maxCopies"] and h.seq_copies(x - 1, 3).tolist() == h.seq_copies()[x - 1:x + 2].tolist()
    h.set_option("seq_slab", 0)


def _c_run(h, parts, prm):
    """begin, one add per part, finish, through the C ABI: (figures, win_offsets, windows, spectrum, totals) of all parts"""
    hx, hip, ctx = _hx(), h._hip, h._ctx()
    h._chk_ctx(hip.h10x_seq_spectrum_begin(ctx, *prm))
    figs, wins, counts = [], [], []
    z = np.zeros(1, dtype=hx._SEQ_SPECTRUM_INFO)
    for part in parts:
        codes, start = h._flatten_seqs(part)
        n = len(part)
        fig = np.zeros(max(n, 1), dtype=hx._SEQ_SPECTRUM_FIGURES)
        h._chk_ctx(hip.h10x_seq_spectrum_add(ctx, codes.ctypes.data, start.ctypes.data, n, fig.ctypes.data, z.ctypes.data))
        assert int(z["sequences"][0]) == n and int(z["bases"][0]) == len(codes)       # add's figures are of its own call
        m = int(z["windows"][0])
        off = np.zeros(n + 1, dtype=np.uint64); win = np.zeros(max(m, 1), dtype=hx._SEQ_SPECTRUM_WINDOW)
        h._chk_ctx(hip.h10x_seq_spectrum_windows_get(ctx, off.ctypes.data, win.ctypes.data, m))
        assert int(off[-1]) == m
        figs.append(fig[:n]); wins.append(win[:m]); counts.append(np.diff(off.astype(np.int64)))
    s = np.zeros((1024, 8), dtype=np.uint64); totals = np.zeros((2, 4), dtype=np.uint64)
    h._chk_ctx(hip.h10x_seq_spectrum_finish(ctx, s.ctypes.data, totals.ctypes.data, z.ctypes.data))
    off = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.uint64)
    return (np.concatenate(figs), off, np.concatenate(wins), s, totals), {k: int(z[k][0]) for k in hx._SEQ_SPECTRUM_INFO.names}


def test_independence(scripted):
    h, z, m, seqs, exp = scripted
    i = z.names.index("short")
    start = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    between = int(start[i + 3] - start[i])                     # a slab that holds short, k-1 and the empty one holds rep8 behind them no more ..
    together = int(start[i + 4] - start[i])                    # .. and this one does; at 1 every sequence goes alone
    few = {p: exp[p] for p in (T + (cases.WIN,), T + (z.pos("main", z.unit + 1),), T + (0,), (0, 0, 0, cases.WIN))}
    for slab in (between, together, 1):
        h.set_option("seq_slab", slab)
        _run_all(h, seqs, few, ("seq_slab", slab))
    h.set_option("seq_slab", 0)
    prm = T + (cases.WIN,)
    result, copies, info = exp[prm]
    for cut in (1, 5, len(seqs)):                              # one call against two add calls (the second may be empty)
        got, ginfo = _c_run(h, [seqs[:cut], seqs[cut:]], prm)
        _same(got, result, ("two adds", cut))
        assert np.array_equal(h.seq_copies(), copies) and ginfo == info
    got, ginfo = _c_run(h, [seqs, seqs], prm)                  # property 7: the list twice within one run doubles the copies
    assert np.array_equal(h.seq_copies(), 2 * copies) and ginfo["maxCopies"] == 2 * info["maxCopies"] and ginfo["moshes"] == 2 * info["moshes"]
    assert _rows(got[0]) == 2 * _rows(result[0]) and _rows(got[2]) == 2 * _rows(result[2])
    double = m.spectrum(2 * copies, *T)
    assert np.array_equal(got[3], double[0]) and np.array_equal(got[4], double[1])
    got2 = h.seq_spectrum(seqs + seqs, *prm)                   # (and as one list given twice)
    assert np.array_equal(got2[3], double[0]) and np.array_equal(got2[4], double[1]) and np.array_equal(h.seq_copies(), 2 * copies)
    rc = [sbm.revcomp(s) for s in seqs]                        # property 6: reverse complements
    figs, _, _, s, totals = h.seq_spectrum(rc, *prm)
    assert _rows(figs) == _rows(result[0]) and np.array_equal(s, result[3]) and np.array_equal(totals, result[4]) and np.array_equal(h.seq_copies(), copies)


def test_cross_check_with_seq_spans(scripted):
    """property 8: with the range lo hi on the state, n2 at (lo, lo, hi) is the inRange figure of seq_spans; and a new range keeps the copies"""
    h, z, m, seqs, exp = scripted
    lo, hi = cases.RANGE
    figs = h.seq_spectrum(seqs, lo, lo, hi)[0]
    copies = h.seq_copies()
    h.depth_range(lo, hi)
    assert np.array_equal(h.seq_copies(), copies)              # not released by a new range
    h.seq_spans(seqs, 1)
    spans = h.seq_spans_info["figures"]
    assert figs["n2"].tolist() == spans["inRange"].tolist() and int(figs["n2"].sum()) > 0 and not figs["n1"].any()
    assert figs["moshes"].tolist() == spans["moshes"].tolist() and (figs["moshes"] - figs["absent"]).tolist() == spans["found"].tolist()   # property 1
    _, _, hfig = h.seq_hashes(seqs)
    assert figs["moshes"].tolist() == hfig["moshes"].tolist() and (figs["moshes"] - figs["absent"]).tolist() == hfig["found"].tolist()
    _check(h, seqs, T + (cases.WIN,), exp[T + (cases.WIN,)], "with a range in force")


@pytest.fixture(scope="module")
def small():
    recs = sbc.small_records()
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(*sbc.SMALL_RANGE)
    m = spm.SeqSpectrumModel(ssm.SeqSpansModel(sbm.SeqBlocksModel.from_state(h)))
    yield h, m, recs, [s for s, _ in sbc.sequences(recs)]
    h.close()


def test_small_against_model(small):
    h, m, recs, seqs = small
    for prm in ((3, 6, 10, 0), (3, 6, 10, 40), (1, 2, 3, 1000), (0, 7, 2 ** 31 - 1, 2 ** 31 - 1)):
        e = m.seq_spectrum(seqs, *prm)
        for slab in (0, 400):
            h.set_option("seq_slab", slab)
            _check(h, seqs, prm, e, ("small", slab))
    h.set_option("seq_slab", 0)
    assert h.seq_spectrum_info["maxCopies"] >= 2


def test_kept_result_and_release(small):
    h, m, recs, seqs = small
    ctx = h._ctx()
    copies_get = lambda: h._hip.h10x_seq_spectrum_copies_get(ctx, 0, 0, None)          # noqa: E731
    a = h.seq_spectrum(seqs, 3, 6, 10, 40)
    b = h.seq_spectrum(seqs, 3, 6, 10, 40)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))                        # two runs give equal bytes
    copies = h.seq_copies()
    assert copies_get() == 0 and int(copies.sum()) == int(a[0]["moshes"].sum()) - int(a[0]["absent"].sum())   # property 3
    n = h.sizes()["hashNumber"]
    assert h._hip.h10x_seq_spectrum_copies_get(ctx, n - 1, 2, None) != 0 and len(h.seq_copies(n)) == 0
    # the run is closed: add and finish need a new begin, the copies stay
    z = np.zeros(16, np.uint64)
    assert h._hip.h10x_seq_spectrum_add(ctx, None, None, 0, None, z.ctypes.data) != 0 and "no run is open" in h._hip.h10x_last_error(ctx).decode()
    assert h._hip.h10x_seq_spectrum_finish(ctx, None, None, z.ctypes.data) != 0 and np.array_equal(h.seq_copies(), copies)
    # the kept results of seq_spans and seq_blocks survive a spectrum run, and the copies survive them
    spans = [x.copy() for x in h.seq_spans(seqs, 2, 30, 50)]
    sb = [x.copy() for x in h.seq_blocks(seqs, 2)[:3]]
    h.seq_spectrum(seqs[:5], 1, 2, 3, 10)
    cols = [np.zeros_like(x) for x in spans[:5]]
    h._chk_ctx(h._hip.h10x_seq_spans_get(ctx, *[c.ctypes.data for c in cols], len(cols[1])))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(cols, spans[:5]))
    off, blk, cnt = (np.zeros_like(x) for x in sb)
    h._chk_ctx(h._hip.h10x_list_share_get(ctx, off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, len(blk)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip((off, blk, cnt), sb))
    part = h.seq_copies()
    h.seq_spans(seqs[:3], 1); h.seq_blocks(seqs[:3], 1)
    h.depth_range(*sbc.SMALL_RANGE)                                                    # a new range keeps the copies
    assert np.array_equal(h.seq_copies(), part) and np.array_equal(part, m.copies(seqs[:5]))
    with pytest.raises(_hx().Hash10xError, match="!! seqSpectrum window -1 must be >= 0"):
        h.seq_spectrum(seqs[:3], 1, 2, 3, -1)
    assert copies_get() != 0 and "no result is kept" in h._hip.h10x_last_error(ctx).decode()   # a refused begin keeps nothing behind
    h.seq_spectrum(seqs[:3], 1, 2, 3)
    h.cluster(1, 0, 2)
    assert copies_get() == 0                                                           # --cluster keeps it
    _check(h, seqs, (3, 6, 10, 40), m.seq_spectrum(seqs, 3, 6, 10, 40), "after --cluster")
    h.cluster_split()
    assert copies_get() != 0                                                           # --clusterSplit releases it
    _same(h.seq_spectrum(seqs, 3, 6, 10, 40), a, "after --clusterSplit, before a new range")   # (hashDepth[] is as it was)
    assert copies_get() == 0
    h.read_fqb(recs)                                                                   # a new state releases it (and is the fixture's state again)
    assert h._hip.h10x_seq_spectrum_copies_get(h._ctx(), 0, 0, None) != 0
    h.depth_range(*sbc.SMALL_RANGE)


def test_refusals(small):
    h, m, recs, seqs = small
    err = _hx().Hash10xError
    order = "!! seqSpectrum needs 0 <= copy1min <= copy2min <= copyMmin"
    for args, msg in (((-1, 2, 3), order), ((3, 2, 5), order), ((1, 5, 4), order), ((1, 2, 3, -1), "!! seqSpectrum window -1 must be >= 0"), ((2, 1, 0, -1), order)):
        with pytest.raises(err, match=re.escape(msg)):
            h.seq_spectrum(seqs[:2], *args)
    ctx = h._ctx()
    z = np.zeros(16, np.uint64)
    for call in (lambda: h._hip.h10x_seq_spectrum_add(ctx, None, None, 0, None, z.ctypes.data), lambda: h._hip.h10x_seq_spectrum_windows_get(ctx, None, None, 0),
                 lambda: h._hip.h10x_seq_spectrum_finish(ctx, None, None, z.ctypes.data), lambda: h._hip.h10x_seq_spectrum_copies_get(ctx, 0, 0, None)):
        assert call() != 0 and "seqSpectrum: no " in h._hip.h10x_last_error(ctx).decode()   # each without a begin (the refused one above released)
    codes, starts = np.zeros(100, np.uint8), np.array([0, 60, 40, 100], dtype=np.uint64)
    assert h._hip.h10x_seq_spectrum_begin(ctx, 1, 2, 3, 0) == 0
    assert h._hip.h10x_seq_spectrum_add(ctx, codes.ctypes.data, starts.ctypes.data, 3, None, z.ctypes.data) != 0
    assert "seqSpectrum: the sequence starts do not ascend at sequence 1" in h._hip.h10x_last_error(ctx).decode()
    starts = np.array([0, 2 ** 33], dtype=np.uint64)            # more than 2^32 - 1 windows in one sequence: refused before anything is read
    assert h._hip.h10x_seq_spectrum_begin(ctx, 1, 2, 3, 1) == 0
    assert h._hip.h10x_seq_spectrum_add(ctx, codes.ctypes.data, starts.ctypes.data, 1, None, z.ctypes.data) != 0
    assert "more than 2^32 - 1 windows" in h._hip.h10x_last_error(ctx).decode()
    e = _hx().Hash10x(B=20)
    with pytest.raises(err, match="no hash state loaded"):
        e.seq_spectrum([b"ACGT"], 1, 2, 3)
    e.read_fqb(recs)                                            # straight after --readFQB, without a range: accepted
    _same(e.seq_spectrum(seqs, 3, 6, 10, 40), m.seq_spectrum(seqs, 3, 6, 10, 40)[0], "no range")
    e.close()
    w = _hx().Hash10x(B=20, r=18)                                # a hasher whose seed the context does not hold
    w.read_fqb(recs)
    assert w._hip.h10x_set_option(w._ctx(), b"seqhash_seed", 17) == 0
    with pytest.raises(err, match="seqSpectrum: option seqhash_seed 17 does not give the context's hash multiplier"):
        w.seq_spectrum(seqs[:2], 1, 2, 3)
    w.close()


# ------------------------------------------------------------------------------------ the command through bin/hash10x-amd
EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
C, WIN = (3, 6, 10), 40
SUMMARY = re.compile(r"^  seq spectrum at copy1min (\d+) copy2min (\d+) copyMmin (\d+), window (\d+): (\d+) sequences, (\d+) bases, (\d+) moshes, (\d+) absent, copy0 (\d+) "
                     r"copy1 (\d+) copy2 (\d+) copyM (\d+), QV (\S+), present (\d+) of (\d+) copy1, (\d+) of (\d+) copy2, (\d+) of (\d+) copyM, completeness (\S+) %$", re.M)
LINE = re.compile(r"SEQ_SPECTRUM  (\S+) len (\d+) moshes (\d+) absent (\d+) copy0 (\d+) copy1 (\d+) copy2 (\d+) copyM (\d+) meanDepth (\S+) QV (\S+)$", re.M)


@pytest.fixture(scope="module")
def cli(tmp_path_factory, small):
    """small.fqb and its test sequences as plain and gzipped FASTA, with the model"""
    h, m, recs, seqs = small
    d = str(tmp_path_factory.mktemp("spcli"))
    recs.tofile(os.path.join(d, "x.fqb"))
    seqs = [s for s in seqs if len(s)]
    names = ["seq%d" % i for i in range(len(seqs))]
    text = ["".join("ACGT"[c] for c in s) for s in seqs]
    fa = "".join(">%s read %d\tmore\n%s\n" % (n, i, "\n".join(t[a:a + 60] for a in range(0, len(t), 60))) for i, (n, t) in enumerate(zip(names, text)))
    with open(os.path.join(d, "s.fa"), "w") as f:
        f.write(fa)
    with gzip.open(os.path.join(d, "s.fa.gz"), "wb") as f:
        f.write(fa.encode())
    return d, h, m, seqs, names


def _run(d, *args):
    p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _near(text, value):
    return text == "inf" if value == float("inf") else abs(float(text) - value) <= 0.01


def _check_text(text, result, info, names, verbose):
    figs, _, _, _, totals = result
    got = SUMMARY.findall(text)
    assert len(got) == 1, text[-600:]
    g = got[0]
    t = [int(v) for v in totals.reshape(-1)]
    assert [int(v) for v in g[:12] + g[13:19]] == list(C) + [WIN, len(names)] + [info[k] for k in ("bases", "moshes", "absent", "n0", "n1", "n2", "nM")] + [
        t[5], t[1], t[6], t[2], t[7], t[3]]
    assert _near(g[12], spm.qv(info["moshes"], info["absent"] + info["n0"], K)) and _near(g[19], spm.completeness(totals))
    lines = LINE.findall(text)
    assert len(lines) == (len(names) if verbose else 0)
    for ln, n, f in zip(lines, names, _rows(figs)):
        assert ln[0] == n and [int(v) for v in ln[1:8]] == list(f[:7])
        assert abs(float(ln[8]) - (f[7] / (f[1] - f[2]) if f[1] > f[2] else 0.0)) <= 0.051   # (one printed decimal)
        assert _near(ln[9], spm.qv(f[1], f[2] + f[3], K))


def test_cli(cli):
    d, h, m, seqs, names = cli
    result, copies, info = m.seq_spectrum(seqs, *C, WIN)
    _check(h, seqs, C + (WIN,), (result, copies, info), "the Python call")
    expected = spm.sp_bytes(m.hash_number, *C, WIN, result, copies, names)
    base = ["-B", 20, "--readFQB", "x.fqb"]                                           # no --hashDepthRange: the command needs none
    rc, out, err = _run(d, "-o", "v.out", *base, "--verbose", "--seqSpectrum", *C, WIN, "s.fa", "x.sp")
    assert rc == 0, err
    image = open(os.path.join(d, "x.sp"), "rb").read()
    assert image == expected
    got = _hx().read_seq_spectrum(os.path.join(d, "x.sp"))
    _same(got[1:6], result, "the file")
    assert np.array_equal(got[6], np.minimum(copies, 255)) and got[7] == names and got[0]["hashNumber"] == m.hash_number
    _check_text(open(os.path.join(d, "v.out")).read(), result, info, names, True)
    rc, out, err = _run(d, *base, "--hashDepthRange", *sbc.SMALL_RANGE, "--seqSpectrum", *C, WIN, "s.fa.gz", "y.sp")   # gzip, with a range: the same file
    assert rc == 0 and open(os.path.join(d, "y.sp"), "rb").read() == image, err
    _check_text(out, result, info, names, False)
    assert not [n for n in os.listdir(d) if n.endswith(".part")]
    h.set_option("seq_slab", 400)                                                    # the session call, in slabs of 400 bases: the same bytes
    h.write_seq_spectrum(*C, WIN, os.path.join(d, "s.fa"), os.path.join(d, "z.sp"), out=os.path.join(d, "z.out"), verbose=True)
    h.set_option("seq_slab", 0)
    assert open(os.path.join(d, "z.sp"), "rb").read() == image
    _check_text(open(os.path.join(d, "z.out")).read(), result, info, names, True)
    assert np.array_equal(h.seq_copies(), copies)                                    # the command leaves its copies kept
    rc, out, err = _run(d, *base, "--seqSpectrum", 0, 0, 0, 0, "s.fa", "i.sp")         # all M: nothing found is unsupported
    assert rc == 0 and re.search(r"copy0 0 copy1 0 copy2 0 copyM %d, QV (\S+)," % (info["moshes"] - info["absent"]), out), (out, err)


def test_cli_refusals(cli):
    d = cli[0]
    gone = lambda name: not os.path.exists(os.path.join(d, name)) and not os.path.exists(os.path.join(d, name + ".part"))   # noqa: E731
    base = ["-B", 20, "--readFQB", "x.fqb"]
    rc, out, err = _run(d, "--seqSpectrum", 1, 2, 3, 0, "s.fa", "none.sp")            # no state
    assert rc == 0 and "!! seqSpectrum: no hash state loaded: use readFQB or readHash first\n" in out and gone("none.sp")
    rc, out, err = _run(d, *base, "--seqSpectrum", 3, 2, 5, 0, "s.fa", "a.sp", "--seqSpectrum", -1, 2, 5, 0, "s.fa", "b.sp", "--seqSpectrum", 1, 2, 3, -1, "s.fa", "c.sp")
    assert rc == 0, err
    assert out.count("!! seqSpectrum needs 0 <= copy1min <= copy2min <= copyMmin\n") == 2 and "!! seqSpectrum window -1 must be >= 0\n" in out
    assert all(gone(n) for n in ("a.sp", "b.sp", "c.sp"))
    rc, out, err = _run(d, *base, "--seqSpectrum", 1, 2, 3, 0, "nosuch.fa", "f.sp")
    assert rc == 255 and "FATAL ERROR: " in err and "failed to open sequence file nosuch.fa\n" in err and gone("f.sp")
    with open(os.path.join(d, "old.sp"), "wb") as f:
        f.write(b"old bytes")
    os.mkdir(os.path.join(d, "old.sp.part"))                                         # the .part cannot be opened: the old file keeps its bytes
    rc, out, err = _run(d, *base, "--seqSpectrum", 1, 2, 3, 0, "s.fa", "old.sp")
    assert rc == 255 and "FATAL ERROR: failed to open output file old.sp\n" in err and open(os.path.join(d, "old.sp"), "rb").read() == b"old bytes"
    os.rmdir(os.path.join(d, "old.sp.part"))
    rc, out, err = _run(d, *base, "--seqSpectrum", 3, 2, 5, 0, "s.fa", "old.sp")      # a refusal over a file that stands there
    assert rc == 0 and open(os.path.join(d, "old.sp"), "rb").read() == b"old bytes"
    rc, out, err = _run(d, *base, "--seqSpectrum", 1, 2, 3, 0, "s.fa", "nodir/b.sp")
    assert rc == 255 and "FATAL ERROR: failed to open output file nodir/b.sp\n" in err and not os.path.exists(os.path.join(d, "nodir"))
    rc, out, err = _run(d, "--gpus", 2, *base, "--seqSpectrum", 1, 2, 3, 0, "s.fa", "s.sp")
    assert rc == 255 and "FATAL ERROR: --seqSpectrum does not run on a sharded session (--gpus 2)" in err and gone("s.sp")
