"""From sequences to blocks without a GPU: the plain-Python model of the definition (tests/seqblocks_model.py) on the golden states, against
the reference's moshutils where it is built, the block identity with the share graph's model on hand-made states, the usage text, the reader of
the .sb file, and the .sb writer under AddressSanitizer + UBSan behind a main of its own."""
import os

import numpy as np
import pytest

import mosh_model as mm
import orc
import seqblocks_cases as cases
import seqblocks_model as sbm
import share_model
import statemosh_model

REF_MOSHUTILS = os.path.join(orc.REF_DIR, "moshutils")
K, W, R = cases.K, cases.W, cases.R


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """small.fqb.gz through the oracle, range 3 .. 14: (model, [(sequence, block)])"""
    recs = cases.small_records()
    o = orc.Oracle(k=K, w=W, seed=R, B=20)
    o.read_fqb(recs)
    p = str(tmp_path_factory.mktemp("sb") / "small.hash")
    o.write_hash(p)
    o.close()
    hf = orc.HashFile(open(p, "rb").read())
    return sbm.SeqBlocksModel.from_hash_file(hf, [cases.SMALL_RANGE]), cases.sequences(recs)


def test_model_on_small(small):
    m, seqs = small
    assert all(len(m.barcode_list(x)) == m.depth[x] for x in range(1, m.hash_number))   # hashDepth is the length of the barcode list
    reads = [(s, c) for s, c in seqs if c]
    assert len(reads) == 41 and len(seqs) == 47
    for s, c in reads:
        q, (moshes, found, query, entries) = m.query(s)
        assert found == moshes, "the state was built from this read"
        assert query == len(q) and entries == sum(len(m.barcode_list(x)) for x in q)
        blk, cnt = m.row(q, 1)
        assert query == 0 or c in blk.tolist(), c
        assert int(cnt.sum()) == entries
    # the inputs are not trivial
    occ = [m.lookup(s) for s, _ in seqs]
    figs = [m.query(s)[1] for s, _ in seqs]
    assert any(f[2] > 64 for f in figs)                                             # more than 64 distinct in-range hashes
    assert any(len({v for v, _ in o}) < len(o) for o in occ)                        # a repeated mosh
    assert any(any(x and not m.within[x] for _, x in o) for o in occ)               # found, out of range
    assert any(any(not x for _, x in o) for o in occ)                               # absent
    assert [f for (s, _), f in zip(seqs, figs) if len(s) < K + W - 1][:3] == [(0, 0, 0, 0)] * 3   # empty, k - 1, k: no window
    # the tallies, pinned
    only = [s for s, _ in seqs]
    assert sum(f[2] for f in figs) == 415
    rows = {t: m.seq_blocks(only, t) for t in (1, 5, 2 ** 31 - 1)}
    assert [len(rows[t][1]) for t in (1, 5, 2 ** 31 - 1)] == [335, 141, 0] and int(rows[1][2].max()) == 103
    # the reverse complement has the same Q and so the same row
    for s in only:
        assert np.array_equal(m.query(sbm.revcomp(s))[0], m.query(s)[0])


def test_model_on_tiny():
    """a state the reference wrote (tiny.hash.gz) and the reads it was built from (tiny.fqb), every hash in range"""
    hf = orc.HashFile(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "tiny.hash.gz")))
    m = sbm.SeqBlocksModel.from_hash_file(hf, [(1, 1 << 30)])
    recs = cases.tiny_records()
    blk = cases.block_of(recs)
    assert m.n_blocks == 9 and m.hash_number == 74 and int(blk[-1]) == 8
    n = 0
    for r in range(len(recs)):
        if blk[r] == blk[-1]:
            continue                                                                 # the trailing block is never hashed
        q, (moshes, found, query, entries) = m.query(cases.read2(recs, r))
        assert found == moshes == len(m.lookup(cases.read2(recs, r))) and query <= found
        if query:
            assert int(blk[r]) in m.row(q, 1)[0].tolist()
        n += query
    assert n == 51


def test_against_reference_moshutils(small, tmp_path):
    """moshutils -c B K W S -a s.fa -d out.txt W.mosh: the MH lines give every distinct mosh of s with its depth in W (0 = absent), W = the
    model's export of the same range. The values with a non-zero depth are hashValue[Q(s)]."""
    if not (orc.have_ref() and os.path.exists(REF_MOSHUTILS)):
        pytest.skip("the reference's moshutils is not under oracle/_ref")
    m, seqs = small
    d = str(tmp_path)
    ms, _ = statemosh_model.state_mosh(m.value, m.depth, m.within, 2, 5, 100, 20, K, W, R)
    with open(os.path.join(d, "W.mosh"), "wb") as f:
        f.write(ms.to_bytes())
    picked = [s for s, c in seqs if not c and len(s) > 1000] + [s for s, c in seqs if c][:6]
    some = 0
    for i, s in enumerate(picked):
        with open(os.path.join(d, "s%d.fa" % i), "w") as f:
            f.write(">s%d\n%s\n" % (i, "".join("ACGT"[c] for c in s)))
        r = orc.run_ref(["-c", 20, K, W, R, "-a", "s%d.fa" % i, "-d", "out%d.txt" % i, "W.mosh"], d, binary="moshutils")
        assert r.returncode == 0, r.stderr[-400:]
        hit = []
        for ln in open(os.path.join(d, "out%d.txt" % i)):
            w = ln.split("\t")
            assert w[0] == "MH"
            if int(w[4]):
                hit.append(int(w[1], 16))
        q, fig = m.query(s)
        assert sorted(hit) == sorted(int(v) for v in m.value[q]) and len(hit) == fig[2]
        some += fig[2]
    assert some > 200


# ------------------------------------------------------------------------------------ the block identity on hand-made states
def _hand_made():
    """block 1 holds hash 1 twice; block 3 has more than 65535 records (no good hashes of its own, yet it stands in the lists); hashes 1, 2
    and 5 are in the range 2 .. 100, hash 5 only inside block 4"""
    filler = np.arange(10, 10 + 65538)
    return [[1, 1, 2, 3], [1, 2, 2, 4], np.concatenate([[1, 2], filler]), [5, 5, 5, 6]]


def test_block_identity():
    hf = orc.HashFile(orc.hash_image(_hand_made()))
    rng = [(2, 100)]
    m = sbm.SeqBlocksModel.from_hash_file(hf, rng)
    sm = share_model.ShareModel.from_hash_file(hf, rng)
    top = int(sm.share.max())
    checked = 0
    for c in range(1, m.n_blocks):
        good = m.good_hashes(c)
        own = sum(int((m.barcode_list(int(x)) == c).sum()) for x in good)            # sum over x of G[c,x] M[c,x]
        for t in (1, 2, top, top + 1):
            d, n = sm.row(c, t)
            exp = {int(a): int(b) for a, b in zip(d, n)}
            if own >= t:
                exp[c] = own
            for order in (good, good[::-1]):
                blk, cnt = m.row(order, t)
                assert dict(zip(blk.tolist(), cnt.tolist())) == exp and blk.tolist() == sorted(exp), (c, t)
            checked += len(exp)
    assert checked > 10 and len(m.good_hashes(3)) == 0 and m.row([1], 1)[0].tolist() == [1, 2, 3]
    assert m.row([1], 1)[1].tolist() == [2, 1, 1] and m.row([1, 1], 2)[1].tolist() == [4, 2, 2]   # a hash given twice counts twice
    assert m.row([5], 3) == m.row([5], 1) and m.row([5], 4)[0].tolist() == []


def test_figures_of_a_list_sum_to_its_entries(small):
    m, seqs = small
    off, hsh, fig = m.seq_hashes([s for s, _ in seqs])
    _, _, cnt = m.list_share(off, hsh, 1)
    assert int(cnt.sum()) == sum(f[3] for f in fig) == int(m.depth[hsh].sum())
    assert int(off[-1]) == len(hsh) == sum(f[2] for f in fig)
    assert mm.factors(R)[0] == m._mosh.factor1


# ------------------------------------------------------------------------------------ the .sb file and its reader
def test_read_seq_blocks(small, tmp_path):
    import struct
    import hash10x_amd
    err = hash10x_amd.Hash10xError
    m, seqs = small
    only = [s for s, _ in seqs]
    names = ["seq%d" % i for i in range(len(only))]
    off, blk, cnt, fig = m.seq_blocks(only, 2)
    good = sbm.sb_bytes(m.n_blocks, 2, [len(s) for s in only], off, blk, cnt, fig, names)
    p = str(tmp_path / "t.sb")

    def read(data):
        with open(p, "wb") as f:
            f.write(data)
        return hash10x_amd.read_seq_blocks(p)

    info, roff, rblk, rcnt, table, rnames = read(good)
    assert info == {"version": 1, "nBlocks": m.n_blocks, "minShare": 2, "nSeq": len(only), "rows": len(blk), "nameBytes": sum(len(n) + 1 for n in names)}
    assert np.array_equal(roff, off) and np.array_equal(rblk, blk) and np.array_equal(rcnt, cnt) and rnames == names and len(blk) > 100
    assert [(int(r["len"]), int(r["moshes"]), int(r["found"]), int(r["query"])) for r in table] == [(len(s),) + f[:3] for s, f in zip(only, fig)]
    empty = read(sbm.sb_bytes(7, 1, [], np.zeros(1, np.uint64), [], [], [], []))
    assert empty[0]["nSeq"] == 0 and empty[1].tolist() == [0] and empty[5] == []
    # every check of the reader fires on a file damaged in that one place
    rows, n = len(blk), len(only)
    at_table, at_off = 40 + 8 * rows, 40 + 8 * rows + 24 * n
    at_names_off = at_off + 8 * (n + 1)
    first = int(np.flatnonzero(np.diff(off.astype(np.int64)) >= 2)[0])                 # a row of at least two entries
    r0 = int(off[first])

    def patched(at, fmt, value):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    for data, what in ((b"10XG" + good[4:], "not a seq blocks file"), (good[:30], "not a seq blocks file"), (patched(4, "<I", 2), "version 2"),
                       (good[:-1], "bytes"), (good + b"\0", "bytes"), (patched(16, "<Q", n + 1), "bytes"),
                       (patched(at_off, "<Q", 1), "the offsets do not ascend"), (patched(at_off + 8 * n, "<Q", rows + 1), "the offsets do not ascend"),
                       (patched(at_names_off + 8, "<Q", 0), "the name offsets do not ascend"), (good[:-1] + b"x", "does not end in NUL"),
                       (patched(40 + 8 * r0, "<I", m.n_blocks), "beyond the %d blocks" % m.n_blocks), (patched(40 + 8 * r0 + 4, "<I", 1), "below minShare 2"),
                       (patched(40 + 8 * (r0 + 1), "<I", int(blk[r0])), "do not ascend"), (patched(at_table + 20, "<I", 9), "reserved")):
        with pytest.raises(err, match=what):
            read(data)


def test_usage_names_seq_blocks():
    import subprocess
    p = subprocess.run([os.path.join(orc.REPO, "bin", "hash10x-amd"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--seqBlocks <minShare> <sequence file> <sb output>" in p.stderr


# ------------------------------------------------------------------------------------ the .sb writer under ASan + UBSan (a program of its own, on the CPU)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:exitcode=67")   # (the HIP runtime, linked in, keeps its own allocations)


@pytest.mark.parametrize("n_seq, per, slabs", [(0, 0, 0), (1, 0, 1), (10, 3, 4), (9, 3, 3), (100, 7, 15), (64, 0, 1)])
def test_sb_writer_under_sanitizers(tmp_path, n_seq, per, slabs):
    import subprocess
    import hash10x_amd
    drv = os.path.join(orc.REPO, "build", "sb-host-asan")
    if not os.path.exists(drv):
        subprocess.run(["make", "-C", os.path.join(orc.REPO, "hash10x_amd", "host"), "asan"], check=True, stdout=subprocess.DEVNULL)
    p = str(tmp_path / "w.sb")
    r = subprocess.run([drv, p, str(n_seq), str(per)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    q = np.arange(n_seq)
    n_rows = q % 4
    assert r.returncode == 0 and b"failed to open output file" in r.stdout, (r.stdout, r.stderr)
    assert r.stdout.startswith(b"%d slabs, %d rows, %d with rows, max count %d\n" % (slabs, n_rows.sum(), (n_rows > 0).sum(), max([2 * i + i % 4 for i in q if i % 4], default=0)))
    assert os.listdir(str(tmp_path)) == ["w.sb"]                                     # no .part, nothing of the failing runs
    info, off, blk, cnt, table, names = hash10x_amd.read_seq_blocks(p)
    assert info == {"version": 1, "nBlocks": 1000000, "minShare": 3, "nSeq": n_seq, "rows": int(n_rows.sum()), "nameBytes": sum(len("s%d" % i) + 1 for i in q)}
    assert names == ["s%d" % i for i in q] and np.array_equal(off, np.concatenate([[0], np.cumsum(n_rows)]).astype(np.uint64))
    assert np.array_equal(table["len"], q % 5 + 1) and np.array_equal(table["moshes"], q % 11) and np.array_equal(table["found"], q % 7) and np.array_equal(table["query"], q % 3)
    assert blk.tolist() == [i + k + 1 for i in q for k in range(i % 4)] and cnt.tolist() == [2 * i + k + 1 for i in q for k in range(i % 4)]
