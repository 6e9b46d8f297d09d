"""Sequence spans on the GPU (csrc/stage_r.hip): Hash10x.seq_spans against the plain-Python model of the definition (tests/seqspans_model.py) on the
scripted cases (tests/seqspans_cases.py) and the golden `small` state; independence of "seq_slab" and "neighbour_budget"; the kept result and its
release; the refusals; the command line and the .ss file. Every comparison is exact equality."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import seqblocks_cases as sbc
import seqblocks_model as sbm
import seqspans_cases as cases
import seqspans_model as ssm

pytestmark = pytest.mark.gpu

K = cases.K
NAMES = ("offsets", "block", "first", "last", "hits", "cover_offsets", "cover")
_hx, _budget = orc.hx, orc.set_budget


def _same(got, exp, what):
    assert len(got) == len(exp) == 7
    for g, e, name in zip(got, exp, NAMES):
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, name)


def _figures(h):
    return [tuple(int(v) for v in r) for r in h.seq_spans_info["figures"].tolist()]


def _info_equal(h, info):
    got = h.seq_spans_info
    assert {k: got[k] for k in info} == info


@pytest.fixture(scope="module")
def scripted(tmp_path_factory):
    z, data, m = cases.script()
    p = tmp_path_factory.mktemp("ss") / "scripted.hash"
    p.write_bytes(data)
    h = _hx().Hash10x(B=20)
    h.read_hash(str(p))
    h.depth_range(*cases.RANGE)
    seqs = cases.sequences(z)
    exp = {prm: m.seq_spans(seqs, *prm) for prm in cases.params(z)}
    yield h, z, m, seqs, exp
    h.close()


def _run_all(h, seqs, exp, what):
    for (t, g, w), (result, figs, info) in exp.items():
        got = h.seq_spans(seqs, t, g, w)
        _same(got, result, (what, t, g, w))
        assert _figures(h) == figs, (what, t, g, w)
        _info_equal(h, info)


def test_cases_against_model(scripted):
    h, z, m, seqs, exp = scripted
    _run_all(h, seqs, exp, "default")
    assert (h.seq_spans_info["batches"], h.seq_spans_info["windows"], h.seq_spans_info["nBlocks"]) == (1, 0, cases.B_HEAVY + 1)
    _run_all(h, seqs, exp, "twice in one process")
    # the heavy block stands in the rows
    off, blk = h.seq_spans(seqs, 1)[:2]
    assert cases.B_HEAVY in blk[int(off[0]):int(off[1])].tolist()
    # text goes in as code arrays do
    text = ["".join("ACGT"[c] for c in s).encode() for s in seqs]
    _same(h.seq_spans(text, 1, 0, 700), h.seq_spans(seqs, 1, 0, 700), "text")


def test_orientation(scripted):
    h, z, m, seqs, exp = scripted
    rc = [sbm.revcomp(s) for s in seqs]
    for t, g, w in ((1, 0, 0), (1, 100, 700), (2, 40, 1)):
        off, blk, first, last, hits = h.seq_spans(seqs, t, g, w)[:5]
        roff, rblk, rfirst, rlast, rhits = h.seq_spans(rc, t, g, w)[:5]
        assert np.array_equal(off, roff)
        for i, s in enumerate(seqs):
            a, b = int(off[i]), int(off[i + 1])
            fwd = list(zip(blk[a:b].tolist(), first[a:b].tolist(), last[a:b].tolist(), hits[a:b].tolist()))
            assert list(zip(rblk[a:b].tolist(), rfirst[a:b].tolist(), rlast[a:b].tolist(), rhits[a:b].tolist())) == ssm.mirrored(fwd, len(s), K), (i, t, g)


def test_independence_of_the_options(scripted):
    h, z, m, seqs, exp = scripted
    i = z.names.index("edge1")
    start = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    between = int(start[i + 5] - start[i]) - 1                 # edge1 .. k fit, edge2 does not: the slab is cut between the two neighbours
    together = int(start[i + 5] - start[i])                    # edge1 .. edge2 in one slab
    for slab in (between, together, 1):
        h.set_option("seq_slab", slab)
        _run_all(h, seqs, exp, ("seq_slab", slab))
    h.set_option("seq_slab", 0)
    per_seq = [sum(len(p) for p in m.hits(s)[0].values()) for s in seqs]
    second = sorted(per_seq)[-2]
    assert sorted(per_seq)[-1] > second + 1 and second > 0
    h.neighbour_stats(reset=True)
    _budget(h, second + 1)                                     # the sequence of most hits alone is above it: block windows; the others in several batches
    _run_all(h, seqs, exp, "budget below one sequence's hits")
    assert h.seq_spans_info["windows"] > 0 and h.seq_spans_info["batches"] > 1
    s = h.neighbour_stats(reset=True)
    assert s["windows"] > 0 and s["batches"] > len(exp)
    _budget(h, max(per_seq))                                   # several batches of whole sequences, no window
    _run_all(h, seqs, exp, "budget of the largest sequence")
    assert h.seq_spans_info["windows"] == 0 and h.seq_spans_info["batches"] > 1
    _budget(h, 1)                                              # every window down to one block
    h.set_option("seq_slab", 1000)
    _run_all(h, seqs, {k: v for k, v in exp.items() if k in ((1, 0, 0), (2, 0, 700), (1, 100, 0))}, "budget 1, slab 1000")
    assert h.seq_spans_info["windows"] > 0
    _budget(h, 0)
    h.set_option("seq_slab", 0)


@pytest.fixture(scope="module")
def small():
    recs = sbc.small_records()
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(*sbc.SMALL_RANGE)
    m = ssm.SeqSpansModel(sbm.SeqBlocksModel.from_state(h))
    yield h, m, recs, [s for s, _ in sbc.sequences(recs)]
    h.close()


def test_small_against_model(small):
    h, m, recs, seqs = small
    for prm in ((1, 0, 0), (5, 0, 100), (2, 30, 50), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        result, figs, info = m.seq_spans(seqs, *prm)
        for slab, budget in ((0, 0), (400, 64)):
            h.set_option("seq_slab", slab); _budget(h, budget)
            _same(h.seq_spans(seqs, *prm), result, (prm, slab, budget))
            assert _figures(h) == figs
            _info_equal(h, info)
    h.set_option("seq_slab", 0); _budget(h, 0)
    # property 1 on the device: at G = 0 the (block, hits) of a sequence without a repeated in-range hash are its --seqBlocks row
    off, blk, first, last, hits = h.seq_spans(seqs, 5)[:5]
    boff, bblk, bcnt, _ = h.seq_blocks(seqs, 5)
    checked = 0
    for i, s in enumerate(seqs):
        xs = [x for _, x in m.occurrences(s) if x and m.sb.within[x]]
        if len(set(xs)) == len(xs):
            a, b, c, d = int(off[i]), int(off[i + 1]), int(boff[i]), int(boff[i + 1])
            assert blk[a:b].tolist() == bblk[c:d].tolist() and hits[a:b].tolist() == bcnt[c:d].tolist()
            checked += 1
    assert checked >= 40 and len(blk) > 100


def test_kept_result_and_release(small):
    h, m, recs, seqs = small
    a = h.seq_spans(seqs, 2, 30, 50)
    b = h.seq_spans(seqs, 2, 30, 50)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))                    # two calls give equal bytes
    sb = [x.copy() for x in h.seq_blocks(seqs, 2)[:3]]                               # the rows of --seqBlocks and the extents do not release each other
    ctx = h._ctx()
    get = lambda: h._hip.h10x_seq_spans_get(ctx, None, None, None, None, None, 0)    # noqa: E731
    cover_get = lambda: h._hip.h10x_seq_spans_cover_get(ctx, None, None, 0)          # noqa: E731
    assert get() == 0 and cover_get() == 0
    n = h.seq_spans_info["extents"]
    cols = [np.zeros(5, np.uint32) for _ in range(4)]
    assert n > 20 and h._hip.h10x_seq_spans_get_range(ctx, 7, 5, *[c.ctypes.data for c in cols]) == 0
    assert [c.tolist() for c in cols] == [x[7:12].tolist() for x in a[1:5]]
    assert h._hip.h10x_seq_spans_get_range(ctx, n - 2, 3, None, None, None, None) != 0
    h.seq_spans(seqs[:3], 1)
    off, blk, cnt = (np.zeros_like(x) for x in sb)
    h._chk_ctx(h._hip.h10x_list_share_get(ctx, off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, len(blk)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip((off, blk, cnt), sb))
    with pytest.raises(_hx().Hash10xError, match="!! seqSpans minShare 0 must be >= 1"):
        h.seq_spans(seqs[:3], 0)
    assert get() != 0 and "no extents are kept" in h._hip.h10x_last_error(ctx).decode()   # a refused run keeps nothing behind
    h.seq_spans(seqs[:3], 1, 0, 10)
    h.depth_range(*sbc.SMALL_RANGE)                                                  # a new range releases them
    assert get() != 0 and cover_get() != 0
    h.seq_spans(seqs[:3], 1, 0, 10)
    assert get() == 0
    h.cluster(1, 0, 2)
    assert get() == 0                                                                # --cluster keeps the blocks
    h.cluster_split()
    assert get() != 0 and cover_get() != 0                                           # --clusterSplit renumbers them
    with pytest.raises(_hx().Hash10xError, match="!! you must set hashDepthRange before seqSpans"):
        h.seq_spans(seqs[:3], 1)
    h.read_fqb(recs)                                                                 # (the fixture's state again, for the tests behind this one)
    h.depth_range(*sbc.SMALL_RANGE)


def test_refusals(small):
    h, m, recs, seqs = small
    err = _hx().Hash10xError
    for args, msg in (((0,), "!! seqSpans minShare 0 must be >= 1"), ((1, -1), "!! seqSpans maxGap -1 must be >= 0"), ((1, 0, -1), "!! seqSpans window -1 must be >= 0"),
                      ((-3, -1, -1), "!! seqSpans minShare -3 must be >= 1")):
        with pytest.raises(err, match=msg):
            h.seq_spans(seqs[:2], *args)
    codes, starts = np.zeros(100, np.uint8), np.array([0, 60, 40, 100], dtype=np.uint64)
    z = np.zeros(16, np.uint64)
    assert h._hip.h10x_seq_spans_run(h._ctx(), 1, 0, 0, codes.ctypes.data, starts.ctypes.data, 3, None, z.ctypes.data) != 0
    assert "seqSpans: the sequence starts do not ascend at sequence 1" in h._hip.h10x_last_error(h._ctx()).decode()
    e = _hx().Hash10x(B=20)
    with pytest.raises(err, match="no hash state loaded"):
        e.seq_spans([b"ACGT"], 1)
    e.read_fqb(recs)
    with pytest.raises(err, match="!! you must set hashDepthRange before seqSpans"):
        e.seq_spans(seqs[:2], 1)
    e.close()
    w = _hx().Hash10x(B=20, r=18)                                                 # a hasher whose seed the context does not hold
    w.read_fqb(recs)
    w.depth_range(*sbc.SMALL_RANGE)
    assert w._hip.h10x_set_option(w._ctx(), b"seqhash_seed", 17) == 0
    with pytest.raises(err, match="seqSpans: option seqhash_seed 17 does not give the context's hash multiplier"):
        w.seq_spans(seqs[:2], 1)
    w.close()
    got = h.seq_spans([], 1, 0, 10)
    assert got[0].tolist() == [0] and got[5].tolist() == [0] and not len(got[1]) and not len(got[6])


# ------------------------------------------------------------------------------------ the command through bin/hash10x-amd
EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
T, G, WIN, MC = 2, 40, 50, 2
SEQ_LINES = re.compile(r"(SEQ_(?:SPANS|WEAK)  .*)$", re.M)


@pytest.fixture(scope="module")
def cli(tmp_path_factory, small):
    """small.fqb and its test sequences as plain FASTA, gzipped FASTA and FASTQ, with the model's result"""
    h, m, recs, seqs = small
    d = str(tmp_path_factory.mktemp("sscli"))
    recs.tofile(os.path.join(d, "x.fqb"))
    seqs = [s for s in seqs if len(s)]
    names = ["seq%d" % i for i in range(len(seqs))]
    text = ["".join("ACGT"[c] for c in s) for s in seqs]
    fa = "".join(">%s read %d\tmore\n%s\n" % (n, i, "\n".join(t[a:a + 60] for a in range(0, len(t), 60))) for i, (n, t) in enumerate(zip(names, text)))
    with open(os.path.join(d, "s.fa"), "w") as f:
        f.write(fa)
    with gzip.open(os.path.join(d, "s.fa.gz"), "wb") as f:
        f.write(fa.encode())
    with open(os.path.join(d, "s.fq"), "w") as f:
        f.write("".join("@%s x\n%s\n+\n%s\n" % (n, t, "I" * len(t)) for n, t in zip(names, text)))
    return d, h, m, seqs, names


def _run(d, *args, stdin=None):
    p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def _lines(result, figs, info, names):
    off, blk, first, last, hits, coff, cover = result
    out, weak_all = [], 0
    for i, (n, f) in enumerate(zip(names, figs)):
        c = cover[int(coff[i]):int(coff[i + 1])].tolist()
        weak = sum(v < MC for v in c)
        weak_all += weak
        out.append("SEQ_SPANS  %s len %d moshes %d found %d inRange %d extents %d boundaries %d weak %d" % ((n,) + f + (len(c), weak)))
        out += ["SEQ_WEAK  %s from %d to %d min %d" % ((n,) + run) for run in ssm.weak_runs(c, WIN, MC)]
    summary = ("  seq spans at minShare %d, maxGap %d, window %d: %d sequences, %d bases, %d moshes, %d found, %d in range, %d hits, %d extents, mean span %s, "
               "max span %d, %d boundaries, %d below minCover %d" % (T, G, WIN, len(names), info["bases"], info["moshes"], info["found"], info["inRange"], info["hits"],
                                                                   info["extents"], ssm.mean_span(info["sumSpan"], info["extents"]), info["maxSpan"], info["boundaries"],
                                                                   weak_all, MC))
    return out, summary


def test_cli(cli):
    d, h, m, seqs, names = cli
    result, figs, info = m.seq_spans(seqs, T, G, WIN)
    _same(h.seq_spans(seqs, T, G, WIN), result, "the Python call")
    expected = ssm.ss_bytes(m.sb.n_blocks, T, G, WIN, MC, result, figs, names)
    lines, summary = _lines(result, figs, info, names)
    assert any(ln.startswith("SEQ_WEAK") for ln in lines) and len(result[1]) > 50 and len(result[6]) > 50
    base = ["-B", 20, "--readFQB", "x.fqb", "--hashDepthRange", *sbc.SMALL_RANGE]
    rc, out, err = _run(d, "-o", "v.out", *base, "--verbose", "--seqSpans", T, G, WIN, MC, "s.fa", "x.ss")
    assert rc == 0, err
    image = open(os.path.join(d, "x.ss"), "rb").read()
    assert image == expected
    got = _hx().read_seq_spans(os.path.join(d, "x.ss"))
    _same(got[1:8], result, "the file")
    assert got[9] == names and got[0]["minCover"] == MC
    text = open(os.path.join(d, "v.out")).read()
    assert SEQ_LINES.findall(text) == lines, text[:600]                             # (a command before may leave its last line open: a line is taken from its word)
    assert [ln for ln in text.splitlines() if ln.startswith("  seq spans at")] == [summary]
    for src in ("s.fa.gz", "s.fq"):                                                  # gzip and FASTQ give the same file; without --verbose no SEQ_ lines
        rc, out, err = _run(d, *base, "--seqSpans", T, G, WIN, MC, src, "y.ss")
        assert rc == 0 and open(os.path.join(d, "y.ss"), "rb").read() == image and "SEQ_" not in out and summary in out.splitlines(), (src, err)
    assert not [n for n in os.listdir(d) if n.endswith(".part")]
    h.set_option("seq_slab", 400)                                                    # the session call, in slabs of 400 bases: the same bytes
    h.write_seq_spans(T, G, WIN, MC, os.path.join(d, "s.fa"), os.path.join(d, "z.ss"), out=os.path.join(d, "z.out"), verbose=True)
    h.set_option("seq_slab", 0)
    assert open(os.path.join(d, "z.ss"), "rb").read() == image
    assert [ln for ln in open(os.path.join(d, "z.out")).read().splitlines() if ln.startswith(("SEQ_", "  seq spans"))] == lines + [summary]
    rc, out, err = _run(d, *base, "--seqSpans", 2 ** 31 - 1, 0, 0, 0, "s.fa", "e.ss")  # no extent: the mean as C prints it
    assert rc == 0 and re.search(r", 0 extents, mean span -nan, max span 0, 0 boundaries, 0 below minCover 0$", out, re.M), out


def test_cli_refusals(cli):
    d = cli[0]
    gone = lambda name: not os.path.exists(os.path.join(d, name)) and not os.path.exists(os.path.join(d, name + ".part"))   # noqa: E731
    base = ["-B", 20, "--readFQB", "x.fqb"]
    ranged = base + ["--hashDepthRange", *sbc.SMALL_RANGE]
    rc, out, err = _run(d, "--seqSpans", 2, 0, 0, 0, "s.fa", "none.ss")              # no state
    assert rc == 0 and "!! you must set hashDepthRange before seqSpans\n" in out and gone("none.ss")
    rc, out, err = _run(d, *base, "--seqSpans", 2, 0, 0, 0, "s.fa", "early.ss")
    assert rc == 0 and "!! you must set hashDepthRange before seqSpans\n" in out and gone("early.ss")
    rc, out, err = _run(d, *ranged, "--seqSpans", 0, 0, 0, 0, "s.fa", "a.ss", "--seqSpans", 1, -1, 0, 0, "s.fa", "b.ss", "--seqSpans", 1, 0, -1, 0, "s.fa", "c.ss",
                        "--seqSpans", 1, 0, 0, -1, "s.fa", "d.ss")
    assert rc == 0, err
    for msg in ("!! seqSpans minShare 0 must be >= 1\n", "!! seqSpans maxGap -1 must be >= 0\n", "!! seqSpans window -1 must be >= 0\n",
                "!! seqSpans minCover -1 must be >= 0\n"):
        assert msg in out, msg
    assert all(gone(n) for n in ("a.ss", "b.ss", "c.ss", "d.ss"))
    rc, out, err = _run(d, *ranged, "--seqSpans", 2, 0, 0, 0, "nosuch.fa", "f.ss")
    assert rc == 255 and "FATAL ERROR: " in err and "failed to open sequence file nosuch.fa\n" in err and gone("f.ss")
    with open(os.path.join(d, "old.ss"), "wb") as f:
        f.write(b"old bytes")
    os.mkdir(os.path.join(d, "old.ss.part"))                                         # the .part cannot be opened: the old file keeps its bytes
    rc, out, err = _run(d, *ranged, "--seqSpans", 2, 0, 0, 0, "s.fa", "old.ss")
    assert rc == 255 and "FATAL ERROR: failed to open output file old.ss\n" in err and open(os.path.join(d, "old.ss"), "rb").read() == b"old bytes"
    os.rmdir(os.path.join(d, "old.ss.part"))
    rc, out, err = _run(d, *ranged, "--seqSpans", 2, 0, 0, 0, "s.fa", "nodir/b.ss")
    assert rc == 255 and "FATAL ERROR: failed to open output file nodir/b.ss\n" in err and not os.path.exists(os.path.join(d, "nodir"))
    rc, out, err = _run(d, "--gpus", 2, *ranged, "--seqSpans", 2, 0, 0, 0, "s.fa", "s.ss")
    assert rc == 255 and "FATAL ERROR: --seqSpans does not run on a sharded session (--gpus 2)" in err and gone("s.ss")
