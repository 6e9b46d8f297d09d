"""Row links and sequence links without a GPU: the plain-numpy model of the definition (tests/seqlinks_model.py) against a brute-force all-pairs
set intersection, the cap boundary, siblings, the ends and the reverse-complement swap, ground truth on a generated genome through the oracle,
the reader of the .sl file, the usage text, and the .sl writer under AddressSanitizer + UBSan behind a main of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mosh_model as mm
import orc
import seqblocks_cases as cases
import seqblocks_model as sbm
import seqlinks_model as slm


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(q) for q in lists])
    return off, np.concatenate([np.asarray(q, dtype=np.uint32) for q in lists] + [np.zeros(0, np.uint32)])


# ------------------------------------------------------------------------------------ the row layer
def test_model_against_brute_force():
    rng = np.random.RandomState(11)
    nonempty = 0
    for trial in range(60):
        n, n_blocks = rng.randint(0, 14), rng.randint(1, 12)
        lists = [sorted(rng.choice(n_blocks, rng.randint(0, n_blocks + 1), replace=False).tolist()) for _ in range(n)]
        off, blk = _csr(lists)
        for min_blocks in (1, 2, 3):
            for max_lists in (0, 1, 2, 5):
                for sib in (False, True):
                    o, f, c, info = slm.row_links(off, blk, min_blocks, max_lists, sib)
                    exp = slm.brute_force(lists, min_blocks, max_lists, sib)
                    assert slm.as_dict(o, f, c) == exp, (trial, min_blocks, max_lists, sib)
                    assert info["links"] == len(exp) == int(o[-1]) and info["lists"] == n and info["rowEntries"] == len(blk)
                    for e in range(n):                             # the upper triangle, ascending
                        row = f[int(o[e]):int(o[e + 1])].tolist()
                        assert row == sorted(row) and all(x > e for x in row)
                    nonempty += bool(exp)
    assert nonempty > 300


def test_cap_boundary():
    """block 7 stands in exactly 4 lists, block 9 in 5: at maxLists 4 block 7 counts and block 9 does not"""
    lists = [[7, 9], [7, 9], [7, 9], [7, 9], [9], [3]]
    off, blk = _csr(lists)
    o, f, c, info = slm.row_links(off, blk, 1, 4)
    assert (info["blocksUsed"], info["skippedBlocks"], info["pairs"]) == (2, 1, 6)
    assert slm.as_dict(o, f, c) == {(a, b): 1 for a in range(4) for b in range(a + 1, 4)}
    o, f, c, info = slm.row_links(off, blk, 1, 5)
    assert (info["blocksUsed"], info["skippedBlocks"], info["pairs"]) == (3, 0, 16)
    d = slm.as_dict(o, f, c)
    assert d[(0, 1)] == 2 and d[(0, 4)] == 1 and len(d) == 10
    o, f, c, info = slm.row_links(off, blk, 1, 3)
    assert info["links"] == 0 and info["skippedBlocks"] == 2 and info["blocksUsed"] == 1
    assert slm.row_links(off, blk, 1, 0)[3] == slm.row_links(off, blk, 1, 5)[3]


def test_siblings():
    lists = [[1, 2, 3], [1, 2, 3], [1, 2], [3]]
    off, blk = _csr(lists)
    assert slm.as_dict(*slm.row_links(off, blk, 1, 0, False)[:3]) == {(0, 1): 3, (0, 2): 2, (0, 3): 1, (1, 2): 2, (1, 3): 1}
    assert slm.as_dict(*slm.row_links(off, blk, 1, 0, True)[:3]) == {(0, 2): 2, (0, 3): 1, (1, 2): 2, (1, 3): 1}   # (2, 3) share nothing anyway
    assert slm.as_dict(*slm.row_links(off, blk, 2, 0, True)[:3]) == {(0, 2): 2, (1, 2): 2}


def test_symmetric_links():
    import hash10x_amd
    lists = [[1, 2, 3], [1, 2, 3], [1, 2], [3], []]
    o, f, c, _ = slm.row_links(*_csr(lists), 1)
    so, sf, sc = hash10x_amd.symmetric_links(o, f, c)
    assert so.tolist() == [0, 3, 6, 8, 10, 10] and sf.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 0, 1] and sc.tolist() == [3, 2, 1, 3, 2, 1, 2, 2, 1, 1]
    assert so.dtype == np.uint64 and sf.dtype == np.uint32 and sc.dtype == np.uint32


# ------------------------------------------------------------------------------------ the ends
def test_cut_ends():
    s = np.arange(10, dtype=np.uint8) % 4
    for end_len, head, tail in ((0, s, s[:0]), (10, s, s), (25, s, s), (7, s[:7], s[3:]), (5, s[:5], s[5:]), (3, s[:3], s[7:])):
        h, t = slm.cut_ends([s], end_len)                          # 0; >= len; len between endLen and 2 endLen (the ends overlap); 2 endLen = len; shorter
        assert np.array_equal(h, head) and np.array_equal(t, tail), end_len
        rh, rt = slm.cut_ends([sbm.revcomp(s)], end_len)
        if end_len:                                                # the reverse complement's head is the tail's reverse complement
            assert np.array_equal(rh, sbm.revcomp(t)) and np.array_equal(rt, sbm.revcomp(h))
    assert [len(e) for e in slm.cut_ends([s[:0], s[:1]], 4)] == [0, 0, 1, 1]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """small.fqb.gz through the oracle, range 3 .. 14, and its test sequences"""
    recs = cases.small_records()
    o = orc.Oracle(k=cases.K, w=cases.W, seed=cases.R, B=20)
    o.read_fqb(recs)
    p = str(tmp_path_factory.mktemp("sl") / "small.hash")
    o.write_hash(p)
    o.close()
    hf = orc.HashFile(open(p, "rb").read())
    return sbm.SeqBlocksModel.from_hash_file(hf, [cases.SMALL_RANGE]), [s for s, _ in cases.sequences(recs)]


def test_reverse_complement_swaps_head_and_tail(small):
    m, seqs = small
    for end_len in (100, 2500):
        roff, rblk = slm.end_rows(m, seqs, 1, end_len)
        coff, cblk = slm.end_rows(m, [sbm.revcomp(s) for s in seqs], 1, end_len)
        row = lambda off, blk, e: blk[int(off[e]):int(off[e + 1])].tolist()
        for s in range(len(seqs)):
            assert row(coff, cblk, 2 * s) == row(roff, rblk, 2 * s + 1) and row(coff, cblk, 2 * s + 1) == row(roff, rblk, 2 * s)
    # end_len 0: the head is the whole sequence's --seqBlocks row, the tail is empty
    roff, rblk = slm.end_rows(m, seqs, 2, 0)
    off, blk, _, _ = m.seq_blocks(seqs, 2)
    assert np.array_equal(roff[0::2], off) and np.array_equal(roff[1::2], off[1:]) and np.array_equal(rblk, blk)
    o, f, c, info, _ = slm.seq_links(m, seqs, 1, 1, 100)
    assert info["links"] > 20 and info["lists"] == 2 * len(seqs)
    assert not np.any((np.repeat(np.arange(info["lists"]), np.diff(o.astype(np.int64))) >> 1) == (f >> 1))


# ------------------------------------------------------------------------------------ ground truth on a generated genome
PIECE, END_LEN = 10000, 2500


def test_ground_truth_on_the_oracle_state(tmp_path):
    """Two haplotypes of 600 kb, 40000 read pairs in 300 barcodes from 5 kb molecules, clustered and split by the oracle: 1697 blocks. Both
    haplotypes cut into 10 kb pieces (120), ends of 2500 bases, minShare 2, no cap: 5120 row entries in 1207 distinct blocks, 20207 pairs. Every
    one of the 118 junctions between consecutive pieces of a haplotype (tail of piece i, head of piece i + 1) shares >= 4 blocks, median 11. At
    minBlocks 3: 968 links, all 118 junctions linked. At minBlocks 5: 425 links, 417 of them between pieces at most one piece apart (either
    haplotype: the two carry the same molecules' hashes but for the SNPs), 112 of the 118 junctions linked; max shared 41."""
    d = str(tmp_path)
    recs = orc.gen_fqb(os.path.join(d, "x.fqb"), 40000, 300, 600000, 0.003, 7, 4.0, 150, 5000, fa=os.path.join(d, "x"))
    o = orc.Oracle(B=21)
    o.read_fqb(recs); o.depth_range(4, 60); o.cluster(1, 0, 3); o.cluster_split()
    o.write_hash(os.path.join(d, "x.hash"))
    o.close()
    m = sbm.SeqBlocksModel.from_hash_file(orc.HashFile(open(os.path.join(d, "x.hash"), "rb").read()), [(4, 60)])
    hap = [mm.parse_seq_bytes(open(os.path.join(d, "x.%s.fa" % a), "rb").read())[0][0] for a in "AB"]
    pieces = [h[a:a + PIECE] for h in hap for a in range(0, len(h), PIECE)]
    per = len(pieces) // 2
    roff, rblk = slm.end_rows(m, pieces, 2, END_LEN)
    assert (m.n_blocks, len(pieces), len(rblk), len(np.unique(rblk))) == (1697, 120, 5120, 1207)
    junctions = [(2 * (h * per + i) + 1, 2 * (h * per + i + 1)) for h in range(2) for i in range(per - 1)]
    assert len(junctions) == 118
    links = {}
    for mb in (1, 3, 5):
        off, other, shared, info = slm.row_links(roff, rblk, mb, 0, True)
        links[mb] = slm.as_dict(off, other, shared), info
    js = sorted(links[1][0].get(j, 0) for j in junctions)
    assert js[0] == 4 and js[len(js) // 2] == 11 and links[1][1]["pairs"] == 20207
    assert links[3][1]["links"] == 968 and all(j in links[3][0] for j in junctions)
    dct, info = links[5]
    near = sum(abs((e >> 1) % per - (f >> 1) % per) <= 1 for e, f in dct)
    linked = sum(j in dct for j in junctions)
    assert (info["links"], near, linked, info["maxShared"]) == (425, 417, 112, 41)
    assert near >= 0.95 * len(dct) and linked >= 0.9 * len(junctions)


# ------------------------------------------------------------------------------------ the .sl file and its reader
def test_read_seq_links(small, tmp_path):
    import hash10x_amd
    err = hash10x_amd.Hash10xError
    m, seqs = small
    names = ["seq%d" % i for i in range(len(seqs))]
    off, other, shared, info, roff = slm.seq_links(m, seqs, 1, 2, 100, 0)
    lens = [len(s) for s in seqs]
    good = slm.sl_bytes(m.n_blocks, 1, 2, 100, 0, lens, roff, off, other, shared, info["skippedBlocks"], names)
    p = str(tmp_path / "t.sl")

    def read(data):
        with open(p, "wb") as f:
            f.write(data)
        return hash10x_amd.read_seq_links(p)

    rinfo, o, f, c, table, rnames = read(good)
    n, links = len(seqs), len(other)
    assert rinfo == {"version": 1, "nBlocks": m.n_blocks, "minShare": 1, "minBlocks": 2, "endLen": 100, "maxEnds": 0, "nSeq": n, "links": links,
                     "skippedBlocks": 0, "nameBytes": sum(len(x) + 1 for x in names)}
    assert np.array_equal(o, off) and np.array_equal(f, other) and np.array_equal(c, shared) and rnames == names and links > 10
    rows = np.diff(roff.astype(np.int64))
    assert [(int(r["len"]), int(r["headRows"]), int(r["tailRows"])) for r in table] == [(lens[i], rows[2 * i], rows[2 * i + 1]) for i in range(n)]
    empty = read(slm.sl_bytes(7, 1, 1, 0, 0, [], np.zeros(1, np.uint64), np.zeros(1, np.uint64), [], [], 0, []))
    assert empty[0]["nSeq"] == 0 and empty[1].tolist() == [0] and empty[5] == []
    # every check of the reader fires on a file damaged in that one place
    at_off = 64 + 16 * n
    at_links = at_off + 8 * (2 * n + 1)
    at_name_off = at_links + 8 * links
    e0 = int(np.flatnonzero(np.diff(off.astype(np.int64)) >= 2)[0])   # a row of at least two links
    r0 = int(off[e0])

    def patched(at, fmt, value):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    for data, what in ((b"10XQ" + good[4:], "not a seq links file"), (good[:50], "not a seq links file"), (patched(4, "<I", 2), "version 2"),
                       (good[:-1], "bytes"), (good + b"\0", "bytes"), (patched(32, "<Q", n + 1), "bytes"), (patched(40, "<Q", links + 1), "bytes"),
                       (patched(28, "<I", 1), "reserved"),
                       (patched(at_off, "<Q", 1), "the offsets do not ascend"), (patched(at_off + 8 * 2 * n, "<Q", links - 1), "the offsets do not ascend"),
                       (patched(at_off + 8 * (e0 + 1), "<Q", int(off[e0 + 2]) + 1), "the offsets do not ascend"),
                       (patched(at_name_off + 8, "<Q", 0), "the name offsets do not ascend"), (good[:-1] + b"x", "does not end in NUL"),
                       (patched(at_links + 8 * r0, "<I", 2 * n), "beyond the %d ends" % (2 * n)),
                       (patched(at_links + 8 * r0, "<I", e0), "not above its row's own end"),
                       (patched(at_links + 8 * r0, "<I", e0 ^ 1 if e0 % 2 == 0 else 2 * n), "the two ends of one sequence" if e0 % 2 == 0 else "beyond"),
                       (patched(at_links + 8 * (r0 + 1), "<I", int(other[r0])), "do not ascend"),
                       (patched(at_links + 8 * r0 + 4, "<I", 1), "fewer than minBlocks 2")):
        with pytest.raises(err, match=what):
            read(data)
    # a sibling link in an even end's row, whatever e0 was
    sib = slm.sl_bytes(9, 1, 1, 5, 0, [9, 9], [0, 1, 2, 3, 4], [0, 1, 1, 1, 1], [1], [1], 0, ["a", "b"])
    with pytest.raises(err, match="the two ends of one sequence"):
        read(sib)
    assert read(slm.sl_bytes(9, 1, 1, 5, 0, [9, 9], [0, 1, 2, 3, 4], [0, 1, 1, 1, 1], [2], [1], 0, ["a", "b"]))[2].tolist() == [2]


def test_usage_names_seq_links():
    p = subprocess.run([os.path.join(orc.REPO, "bin", "hash10x-amd"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--seqLinks <minShare> <minBlocks> <endLen> <maxEnds> <sequence file> <sl output>" in p.stderr


# ------------------------------------------------------------------------------------ the .sl writer under ASan + UBSan (a program of its own, on the CPU)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:exitcode=67")   # (the HIP runtime, linked in, keeps its own allocations)


def _driver_links(n_seq):
    """what host/sl_asan_driver.c makes: end e has e % 3 links to ends e + 2 + k (those that exist), shared e + k + 1"""
    rows = [[(e + 2 + k, e + k + 1) for k in range(e % 3) if e + 2 + k < 2 * n_seq] for e in range(2 * n_seq)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    flat = [x for r in rows for x in r]
    return off, [x[0] for x in flat], [x[1] for x in flat], len({e >> 1 for e, r in enumerate(rows) if r} | {x[0] >> 1 for x in flat})


@pytest.mark.parametrize("n_seq, per, pieces", [(0, 0, 0), (1, 0, 0), (2, 0, 1), (10, 3, 6), (9, 5, 3), (100, 7, 29), (64, 0, 1)])
def test_sl_writer_under_sanitizers(tmp_path, n_seq, per, pieces):
    import hash10x_amd
    drv = os.path.join(orc.REPO, "build", "sl-host-asan")
    if not os.path.exists(drv):
        subprocess.run(["make", "-C", os.path.join(orc.REPO, "hash10x_amd", "host"), "asan"], check=True, stdout=subprocess.DEVNULL)
    p = str(tmp_path / "w.sl")
    r = subprocess.run([drv, p, str(n_seq), str(per)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    off, other, shared, with_links = _driver_links(n_seq)
    assert r.returncode == 0 and b"failed to open output file" in r.stdout, (r.stdout, r.stderr)
    assert r.stdout.startswith(b"%d pieces, %d links, %d with links, max shared %d\n" % (pieces, len(other), with_links, max(shared, default=0))), r.stdout
    assert os.listdir(str(tmp_path)) == ["w.sl"]                                     # no .part, nothing of the failing runs
    q = np.arange(n_seq)
    names = ["s%d" % i for i in q]
    info, roff, rother, rshared, table, rnames = hash10x_amd.read_seq_links(p)
    assert info == {"version": 1, "nBlocks": 1000000, "minShare": 3, "minBlocks": 2, "endLen": 2500, "maxEnds": 8, "nSeq": n_seq, "links": len(other),
                    "skippedBlocks": 5, "nameBytes": sum(len(x) + 1 for x in names)}
    assert rnames == names and np.array_equal(roff, off) and rother.tolist() == other and rshared.tolist() == shared
    assert np.array_equal(table["len"], q % 5 + 1) and np.array_equal(table["headRows"], q % 4) and np.array_equal(table["tailRows"], q % 3)
    row_off = np.concatenate([[0], np.cumsum(np.stack([q % 4, q % 3], axis=1).reshape(-1))])
    assert open(p, "rb").read() == slm.sl_bytes(1000000, 3, 2, 2500, 8, (q % 5 + 1).tolist(), row_off, off, other, shared, 5, names)
