"""Sequence spans without a GPU: the plain-Python model of the definition (tests/seqspans_model.py) held to the --seqBlocks model through the
properties the definition gives, the scripted cases' own claims (tests/seqspans_cases.py), read_seq_spans and its refusals, and the .ss writer
under AddressSanitizer + UBSan behind a main of its own. Every comparison is exact equality."""
import os
import struct
import subprocess

import numpy as np
import pytest

import orc
import seqblocks_cases as sbc
import seqblocks_model as sbm
import seqspans_cases as cases
import seqspans_model as ssm

K = cases.K
TOP = 2 ** 31 - 1


# ------------------------------------------------------------------------------------ the model against the --seqBlocks model on the golden sets
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    recs = sbc.small_records()
    o = orc.Oracle(k=sbc.K, w=sbc.W, seed=sbc.R, B=20)
    o.read_fqb(recs)
    p = str(tmp_path_factory.mktemp("ss") / "small.hash")
    o.write_hash(p)
    o.close()
    sb = sbm.SeqBlocksModel.from_hash_file(orc.HashFile(open(p, "rb").read()), [sbc.SMALL_RANGE])
    return ssm.SeqSpansModel(sb), [s for s, _ in sbc.sequences(recs)]


def _tiny():
    sb = sbm.SeqBlocksModel.from_hash_file(orc.HashFile(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "tiny.hash.gz"))), [(1, 1 << 30)])
    recs = sbc.tiny_records()
    return ssm.SeqSpansModel(sb), [sbc.read2(recs, r) for r in range(len(recs))] + [np.concatenate([sbc.read2(recs, r) for r in (0, 4, 9, 0)])]


def _properties_1_2(m, seqs, thresholds):
    plain = repeated = 0
    for s in seqs:
        occ = [(p, x) for p, x in m.occurrences(s) if x and m.sb.within[x]]
        xs = [x for _, x in occ]
        row1, fig, n_all = m.row(s, 1, 0)
        assert n_all == len(row1) and fig[2] == len(occ)
        assert sum(e[3] for e in row1) == sum(int(m.sb.depth[x]) for x in xs)          # property 2
        if len(set(xs)) < len(xs):
            repeated += 1
            continue
        plain += 1
        for t in thresholds:                                                            # property 1
            blk, cnt = m.sb.row(m.sb.query(s)[0], t)
            assert [(e[0], e[3]) for e in m.row(s, t, 0)[0]] == list(zip(blk.tolist(), cnt.tolist()))
    return plain, repeated


def test_properties_on_small(small):
    m, seqs = small
    plain, repeated = _properties_1_2(m, seqs, (1, 5, TOP))
    assert plain >= 40 and repeated >= 1                       # the joined sequences hold their first read twice
    # property 4: raising G only merges extents, raising T only removes them
    for s in seqs:
        rows = [m.row(s, 1, g)[0] for g in (1, 10, 100, 10000, 0)]                      # (0 never splits: the coarsest)
        for fine, coarse in zip(rows, rows[1:]):
            assert len(coarse) <= len(fine) and sum(e[3] for e in coarse) == sum(e[3] for e in fine)
            for d, f, l, n in fine:
                assert any(cd == d and cf <= f and l <= cl for cd, cf, cl, _ in coarse)
        for g in (0, 100):
            kept = [m.row(s, t, g)[0] for t in (1, 2, 5, TOP)]
            for lo, hi in zip(kept, kept[1:]):
                assert set(hi) <= set(lo)
            assert kept[1] == [e for e in kept[0] if e[3] >= 2] and not kept[3]
    # property 3 on real reads
    for s in seqs:
        for g in (0, 30):
            assert m.row(sbm.revcomp(s), 1, g)[0] == ssm.mirrored(m.row(s, 1, g)[0], len(s), K)


def test_properties_on_tiny():
    m, seqs = _tiny()
    plain, repeated = _properties_1_2(m, seqs, (1, 2))
    assert plain >= 5 and repeated >= 1                        # (the joined sequence holds read 0 twice)


# ------------------------------------------------------------------------------------ the scripted cases: each states the edge it hits and asserts it from the model
@pytest.fixture(scope="module")
def scripted():
    return cases.script()


def _of(row, block):
    return [e[1:] for e in row if e[0] == block]


def test_gap_edges(scripted):
    z, _, m = scripted
    s = z.seqs["main"]
    g = cases.gap_of(z, "main", 4)
    a, b = z.pos("main", 4), z.pos("main", 5)
    assert b - a == g >= 2
    assert _of(m.row(s, 1, g)[0], cases.B_GAP) == [(a, b, 2)]                        # exactly G apart: one extent
    assert _of(m.row(s, 1, g - 1)[0], cases.B_GAP) == [(a, a, 1), (b, b, 1)]         # G + 1 apart: two
    first, last = z.pos("main", 0), z.pos("main", len(z.occ["main"]) - 1)
    assert last - first > 2500 and _of(m.row(s, 1, 0)[0], cases.B_ENDS) == [(first, last, 2)]   # G = 0 never splits
    u = [e[1:] for e in m.row(s, 1, 1)[0] if e[0] == cases.B_UNIT]                   # G = 1
    assert len(u) == 2 and u[0][1] - u[0][0] == 1 and u[0][2] == 2 and u[1][2] == 1 and u[1][0] - u[0][1] > 1


def test_threshold_edges(scripted):
    z, _, m = scripted
    s = z.seqs["main"]
    all_, kept = m.row(s, 1, 0)[0], m.row(s, 4, 0)[0]
    assert _of(all_, cases.B_T3)[0][2] == 3 and _of(all_, cases.B_T4)[0][2] == 4
    assert not _of(kept, cases.B_T3) and _of(kept, cases.B_T4) == _of(all_, cases.B_T4)
    inner = max(cases.gap_of(z, "main", i) for i in (30, 31, 32))
    assert z.pos("main", 60) - z.pos("main", 33) > inner
    assert [e[2] for e in _of(m.row(s, 1, inner)[0], cases.B_SPLIT)] == [4, 1]
    assert [e[2] for e in _of(m.row(s, 2, inner)[0], cases.B_SPLIT)] == [4]           # one kept, one dropped
    row, fig, n_all = m.row(z.seqs["lone"], 2, 0)
    assert row == [] and fig[2] == 1 and n_all == 1                                  # a row with no kept extent


def test_repeated_hits(scripted):
    z, _, m = scripted
    row = m.row(z.seqs["main"], 1, 5)[0]
    p = z.pos("main", 40)
    assert _of(row, cases.B_TWICE) == [(p, p, 2)]                                    # a block that holds a hash twice: gap 0
    p = z.pos("main", 41)
    assert _of(row, cases.B_257) == [(p, p, 257)]
    assert _of(m.row(z.seqs["main"], 257, 0)[0], cases.B_257) == [(p, p, 257)] and not _of(m.row(z.seqs["main"], 258, 0)[0], cases.B_257)
    long_ = m.row(z.seqs["long"], 1, 0)[0]
    assert [(e[0], e[3]) for e in long_] == [(cases.B_64, 64), (cases.B_65, 65), (cases.B_256, 256), (cases.B_257D, 257)]
    assert all(e[1] == z.pos("long", 0) for e in long_) and [e[2] for e in long_] == [z.pos("long", n - 1) for n in (64, 65, 256, 257)]
    assert len({p for p, _ in z.occ["long"][:257]}) == 257                           # at distinct positions


def test_repeated_hash(scripted):
    z, _, m = scripted
    s = z.seqs["dup"]
    p1, p2 = z.pos("dup", z.dup[0]), z.pos("dup", z.dup[1])
    assert z.occ["dup"][z.dup[0]][1] == z.occ["dup"][z.dup[1]][1] and p2 - p1 == 1300
    assert _of(m.row(s, 1, p2 - p1 - 1)[0], cases.B_DUP) == [(p1, p1, 1), (p2, p2, 1)]
    assert _of(m.row(s, 1, p2 - p1)[0], cases.B_DUP) == [(p1, p2, 2)] == _of(m.row(s, 1, 0)[0], cases.B_DUP)
    assert m.row(s, 1, 0)[1][2] == 2                                                 # inRange counts occurrences, not distinct hashes


def test_sequence_edges(scripted):
    z, _, m = scripted
    e1, e2 = z.seqs["edge1"], z.seqs["edge2"]
    assert _of(m.row(e1, 1, 0)[0], cases.B_EDGE) == [(0, len(e1) - K, 2)]            # hits at position 0 and at L - k
    names = z.names
    i = names.index("edge1")
    assert names[i:i + 5] == ["edge1", "empty", "k-1", "k", "edge2"]
    assert [len(z.seqs[n]) for n in names[i + 1:i + 4]] == [0, K - 1, K]
    # the last hit of edge1 and the first of edge2 lie 3 k - 1 slab ordinals apart, closer than G = 100: two extents all the same
    ordinal_gap = (len(e1) - z.pos("edge1", len(z.occ["edge1"]) - 1)) + 0 + (K - 1) + K + z.pos("edge2", 0)
    assert ordinal_gap == 3 * K - 1 < 100
    assert _of(m.row(e1, 1, 100)[0], cases.B_NEIGH) == [(len(e1) - K, len(e1) - K, 1)] and _of(m.row(e2, 1, 100)[0], cases.B_NEIGH) == [(0, 0, 1)]
    row, fig, _ = m.row(z.seqs["deep"], 1, 0)
    assert row == [] and fig[1] == 1 and fig[2] == 0 and fig[0] >= 1                 # found, none counting
    row, fig, _ = m.row(z.seqs["absent"], 1, 0)
    assert row == [] and fig[0] > 5 and fig[1] == 0                                  # none found at all
    assert m.row(z.seqs["k-1"], 1, 0)[1] == (0, 0, 0) and m.row(z.seqs["empty"], 1, 0)[1] == (0, 0, 0)


def test_coverage_edges(scripted):
    z, _, m = scripted
    s = z.seqs["cover"]
    row = m.row(s, 1, 0)[0]
    f, l = z.pos("cover", 2), z.pos("cover", 9)
    assert row == [(cases.B_COVER, f, l, 2)] and 1 <= f < l and len(s) == 2000
    assert m.cover(row, 2000, f + 1)[0] == 1                                         # first = b_1 - 1 and last >= b_1: spans
    assert m.cover(row, 2000, f)[0] == 0                                             # first = b_1: does not (nor a later boundary before first)
    assert m.cover(row, 2000, l)[0] == 1                                             # last = b_1: spans
    assert m.cover(row, 2000, l + 1)[0] == 0                                         # last = b_1 - 1: does not
    assert [len(m.cover(row, 2000, w)) for w in (2000, 1999, 1000)] == [0, 1, 1]     # L = W, W + 1, 2 W
    assert len(m.cover([], 3001, 1500)) == 2 and len(z.seqs["main"]) == 3001         # L = 2 W + 1
    one = m.cover(row, 2000, 1)
    assert len(one) == 1999 and one == [1 if f < j <= l else 0 for j in range(1, 2000)]   # W = 1
    assert m.cover(row, 2000, 10 ** 6) == [] and m.cover(row, 2000, 0) == []         # W > L; W = 0
    p = z.pos("main", 40)
    twice = [e for e in m.row(z.seqs["main"], 1, 0)[0] if e[0] == cases.B_TWICE]
    assert p // 700 == twice[0][2] // 700 and m.cover(twice, 3001, 700) == [0, 0, 0, 0]   # an extent inside one window adds nothing


def test_heavy_block(scripted):
    z, data, m = scripted
    hf = orc.HashFile(data)
    assert int(hf.blocks["nHash"][cases.B_HEAVY]) == cases.HEAVY_RECORDS > 65535
    assert _of(m.row(z.seqs["main"], 1, 0)[0], cases.B_HEAVY) == [(z.pos("main", 50), z.pos("main", 51), 2)]


def test_orientation(scripted):
    z, _, m = scripted
    for t, g, _ in cases.params(z):
        for name in z.names:
            s = z.seqs[name]
            assert m.row(sbm.revcomp(s), t, g)[0] == ssm.mirrored(m.row(s, t, g)[0], len(s), K), (name, t, g)


# ------------------------------------------------------------------------------------ read_seq_spans
def _file(scripted, t=1, g=0, w=700, min_cover=1):
    z, _, m = scripted
    result, figs, _ = m.seq_spans(cases.sequences(z), t, g, w)
    return result, figs, list(z.names), m.sb.n_blocks


def test_read_seq_spans(scripted, tmp_path):
    hx = orc.hx()
    result, figs, names, n_blocks = _file(scripted)
    good = ssm.ss_bytes(n_blocks, 1, 0, 700, 1, result, figs, names)
    p = tmp_path / "x.ss"
    p.write_bytes(good)
    info, off, blk, first, last, hits, coff, cover, table, rnames = hx.read_seq_spans(str(p))
    assert info == {"version": 1, "nBlocks": n_blocks, "minShare": 1, "maxGap": 0, "window": 700, "minCover": 1, "nSeq": len(names), "extents": len(result[1]),
                    "boundaries": len(result[6]), "nameBytes": sum(len(n) + 1 for n in names)}
    for got, exp in zip((off, blk, first, last, hits, coff, cover), result):
        assert got.dtype == exp.dtype and np.array_equal(got, exp)
    assert rnames == names and [(int(r["len"]), int(r["moshes"]), int(r["found"]), int(r["inRange"])) for r in table] == [f[:4] for f in figs]
    assert int(table["weak"].sum()) == int((cover < 1).sum()) > 0 and len(blk) > 10 and len(cover) > 10

    def refused(data, what):
        p.write_bytes(data)
        with pytest.raises(hx.Hash10xError, match=what):
            hx.read_seq_spans(str(p))

    off, blk, first, last, hits, coff, cover = result
    variant = lambda **kw: ssm.ss_bytes(n_blocks, kw.pop("t", 1), 0, kw.pop("w", 700), kw.pop("mc", 1), kw.pop("result", result), figs, names, **kw)   # noqa: E731
    refused(variant(magic=b"10XQ"), "not a seq spans file")
    refused(variant(version=2), "version 2")
    refused(good + b"\0", "need")
    refused(good[:-1], "need")
    refused(good[:28] + struct.pack("<I", 1) + good[32:], "reserved word")
    bad = off.copy(); bad[3] = bad[4] + 1
    refused(variant(result=(bad,) + result[1:]), "offsets do not ascend")
    bad = off.copy(); bad[-1] -= 1
    refused(variant(result=(bad,) + result[1:]), "offsets do not ascend")
    bad = coff.copy(); bad[1] += 1
    refused(variant(result=result[:5] + (bad, cover)), "cover offsets")
    refused(variant(w=500), "cover offsets")
    bad = first.copy(); bad[0] = last[0] + 1
    refused(variant(result=(off, blk, bad, last, hits, coff, cover)), "first <= last < len")
    bad = last.copy(); bad[0] = figs[0][0]
    refused(variant(result=(off, blk, first, bad, hits, coff, cover)), "first <= last < len")
    bad = blk.copy(); bad[1] = bad[0]; badf = first.copy(); badf[1] = badf[0]
    assert int(off[1]) >= 2
    refused(variant(result=(off, bad, badf, last, hits, coff, cover)), "do not ascend by")
    bad = blk.copy(); bad[-1] = n_blocks
    refused(variant(result=(off, bad, first, last, hits, coff, cover)), "beyond the")
    refused(variant(t=2), "below minShare")
    refused(variant(weak=[0] * len(names)), "weak count")
    refused(variant(mc=2, weak=[int((cover[int(a):int(b)] < 1).sum()) for a, b in zip(coff, coff[1:])]), "weak count")
    refused(good[:-1] + b"x", "does not end in NUL")


def test_usage_names_seq_spans():
    p = subprocess.run([os.path.join(orc.REPO, "bin", "hash10x-amd"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--seqSpans <minShare> <maxGap> <window> <minCover> <sequence file> <ss output>" in p.stderr


# ------------------------------------------------------------------------------------ the .ss writer under ASan + UBSan (a program of its own, on the CPU)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:exitcode=67")


@pytest.mark.parametrize("n_seq, per, slabs", [(0, 0, 0), (1, 0, 1), (10, 3, 4), (9, 3, 3), (100, 7, 15), (64, 0, 1)])
def test_ss_writer_under_sanitizers(tmp_path, n_seq, per, slabs):
    import hash10x_amd
    drv = os.path.join(orc.REPO, "build", "ss-host-asan")
    if not os.path.exists(drv):
        subprocess.run(["make", "-C", os.path.join(orc.REPO, "hash10x_amd", "host"), "asan"], check=True, stdout=subprocess.DEVNULL)
    p = str(tmp_path / "w.ss")
    r = subprocess.run([drv, p, str(n_seq), str(per)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    assert r.returncode == 0 and b"failed to open output file" in r.stdout, (r.stdout, r.stderr)
    q = np.arange(n_seq)
    n_rows, n_bounds = q % 4, 10 * q // 4
    cov = [[(i + j) % 3 for j in range(10 * i // 4)] for i in q]
    weak = [sum(c < 2 for c in cv) for cv in cov]
    spans = [i for i in q for _ in range(i % 4)]
    tail = b"%d slabs, %d extents, %d boundaries, %d weak, %d hits, sum span %d, max span %d, max hits %d\n" % (
        slabs, n_rows.sum(), n_bounds.sum(), sum(weak), 5 * n_seq, sum(spans), max(spans, default=0), max([2 * i + i % 4 for i in q if i % 4], default=0))
    assert tail in r.stdout, r.stdout[-400:]
    assert os.listdir(str(tmp_path)) == ["w.ss"]                                     # no .part, nothing of the failing runs; the old bytes kept
    info, off, blk, first, last, hits, coff, cover, table, names = hash10x_amd.read_seq_spans(p)
    assert info == {"version": 1, "nBlocks": 1000000, "minShare": 3, "maxGap": 7, "window": 4, "minCover": 2, "nSeq": n_seq, "extents": int(n_rows.sum()),
                    "boundaries": int(n_bounds.sum()), "nameBytes": sum(len("s%d" % i) + 1 for i in q)}
    assert names == ["s%d" % i for i in q] and np.array_equal(off, np.concatenate([[0], np.cumsum(n_rows)]).astype(np.uint64))
    assert np.array_equal(table["len"], 10 * q + 1) and np.array_equal(table["moshes"], q % 11) and np.array_equal(table["found"], q % 7)
    assert np.array_equal(table["inRange"], q % 3) and table["weak"].tolist() == weak and cover.tolist() == [c for cv in cov for c in cv]
    assert blk.tolist() == [i + k + 1 for i in q for k in range(i % 4)] and hits.tolist() == [2 * i + k + 1 for i in q for k in range(i % 4)]
    assert first.tolist() == [k for i in q for k in range(i % 4)] and last.tolist() == [k + i for i in q for k in range(i % 4)]
    lines = r.stdout.decode().splitlines()
    assert [ln for ln in lines if ln.startswith("SEQ_SPANS  ")] == [
        "SEQ_SPANS  s%d len %d moshes %d found %d inRange %d extents %d boundaries %d weak %d" % (i, 10 * i + 1, i % 11, i % 7, i % 3, i % 4, 10 * i // 4, weak[i]) for i in q]
    assert [ln for ln in lines if ln.startswith("SEQ_WEAK  ")] == ["SEQ_WEAK  s%d from %d to %d min %d" % ((i,) + run) for i in q for run in ssm.weak_runs(cov[i], 4, 2)]
