"""From sequences to blocks on the GPU (csrc/stage_p.hip): Hash10x.seq_hashes / list_share / seq_blocks against the plain-Python model of the
definition (tests/seqblocks_model.py) on hand-made states, the golden sets and the generated set; both key widths; batching of both layers;
the kept results; the refusals; the command line and the .sb file. Every comparison is exact equality."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import mosh_model as mm
import orc
import seqblocks_cases as cases
import seqblocks_model as sbm
import share_model

pytestmark = pytest.mark.gpu

TOP = 2 ** 31 - 1
K, W = cases.K, cases.W
_hx, _budget = orc.hx, orc.set_budget


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("offsets", "block", "count")):
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, name)


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(q) for q in lists])
    return off, np.concatenate([np.asarray(q, dtype=np.uint32) for q in lists] + [np.zeros(0, np.uint32)])


# ------------------------------------------------------------------------------------ the list layer on a hand-made state
HEAVY = 67                                                     # the block of more than 65535 records


def _hand_made():
    """hash 1: 64 entries (blocks 1 .. 63 and the heavy block), hash 2: 65 entries (blocks 1 .. 64 and the heavy block), hash 3: 257 entries,
    all of block 66; hashes 100 .. 170 in two or three blocks each; block 67 holds 65540 records"""
    blocks = [[] for _ in range(HEAVY)]
    for b in range(1, 64):
        blocks[b - 1].append(1)
    for b in range(1, 65):
        blocks[b - 1].append(2)
    blocks[66 - 1] += [3] * 257
    for i in range(71):
        for b in {i % 60 + 1, i * 7 % 60 + 1, i * 11 % 59 + 2}:
            blocks[b - 1].append(100 + i)
    blocks[HEAVY - 1] = np.concatenate([[1, 2], np.arange(1000, 1000 + 65538)])
    return blocks


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    h = orc.load_image(tmp_path_factory.mktemp("sbh"), _hand_made(), 2, 100)
    m = sbm.SeqBlocksModel.from_state(h)
    assert [len(m.barcode_list(x)) for x in (1, 2, 3)] == [64, 65, 257] and h.export_blocks()["nHash"][HEAVY] == 65540
    yield h, m
    h.close()


LISTS = [[], [3], list(range(100, 163)), [], list(range(100, 164)), list(range(170, 105, -1)), [1], [2], [1, 1], [1000], [3, 2, 1], [120], []]


def test_lists_against_model(hand):
    h, m = hand
    assert sorted(len(q) for q in LISTS)[:8] == [0, 0, 0, 1, 1, 1, 1, 1] and {63, 64, 65} <= {len(q) for q in LISTS}
    off, hsh = _csr(LISTS)
    results = {}
    for budget in (0, 40):
        _budget(h, budget)
        h.neighbour_stats(reset=True)
        for t in (1, 2, 257, 258, TOP):
            got = h.list_share(off, hsh, t)
            info = h.seq_blocks_info
            _same(got, m.list_share(off, hsh, t), (budget, t))
            _same(h.list_share(off, hsh, t), got, ("a second identical call", budget, t))
            assert info["rows"] == len(got[1]) == int(got[0][-1]) and info["lists"] == len(LISTS) and info["listHashes"] == len(hsh)
            assert info["listEntries"] == int(m.depth[hsh].sum()) and info["nBlocks"] == HEAVY + 1 and info["wideBatches"] == 0
            assert info["maxCount"] == (int(got[2].max()) if len(got[2]) else 0)
            results[(budget, t)] = got
        s = h.neighbour_stats(reset=True)
        if budget:                                             # the 65-hash list alone is above it: windows of block index
            assert h.seq_blocks_info["windows"] >= 2 and h.seq_blocks_info["batches"] > 3 and s["windows"] >= 2 and s["batches"] > 3, s
        else:
            assert s["windows"] == 0 and s["batches"] == 10 and s["gathered"] == 10 * int(m.depth[hsh].sum()), s
    _budget(h, 0)
    for t in (1, 2, 257, 258, TOP):
        _same(results[(40, t)], results[(0, t)], t)
    off1, blk1, cnt1 = results[(0, 1)]
    row = lambda q: (blk1[int(off1[q]):int(off1[q + 1])].tolist(), cnt1[int(off1[q]):int(off1[q + 1])].tolist())
    assert row(0) == ([], []) and row(1) == ([66], [257]) and row(12) == ([], [])
    assert row(6) == (list(range(1, 64)) + [HEAVY], [1] * 64)                        # the heavy block stands in the row
    assert row(8) == (row(6)[0], [2] * 64) and row(9) == ([HEAVY], [1])              # a hash given twice counts twice
    assert int(cnt1.sum()) == int(m.depth[hsh].sum())                               # at T = 1 the counts sum to the entries
    assert results[(0, 257)][1].tolist() == [66, 66] and results[(0, 258)][1].tolist() == [] and not results[(0, TOP)][0].any()


def test_block_identity_with_the_share_graph(hand):
    h, m = hand
    sm = share_model.ShareModel.from_state(h)
    lists = [m.good_hashes(c)[::-1] for c in range(1, m.n_blocks)]
    off, hsh = _csr(lists)
    for t in (1, 2, 3):
        goff, gblk, gcnt = h.share_graph(t)
        loff, lblk, lcnt = h.list_share(off, hsh, t)
        for c in range(1, m.n_blocks):
            own = sum(int((m.barcode_list(int(x)) == c).sum()) for x in lists[c - 1])
            exp = dict(zip(gblk[int(goff[c - 1]):int(goff[c])].tolist(), gcnt[int(goff[c - 1]):int(goff[c])].tolist()))
            assert exp == dict(zip(*[a.tolist() for a in sm.row(c, t)]))
            if own >= t:
                exp[c] = own
            a, b = int(loff[c - 1]), int(loff[c])
            assert dict(zip(lblk[a:b].tolist(), lcnt[a:b].tolist())) == exp and lblk[a:b].tolist() == sorted(exp), (c, t)
    assert len(lists[HEAVY - 1]) == 0 and {1, 2} <= set(lists[0].tolist())


def test_list_refusals(hand):
    h, m = hand
    err = _hx().Hash10xError
    off, hsh = _csr([[1], [5, 2, 0]])
    with pytest.raises(err, match="!! listShare minShare 0 must be >= 1"):
        h.list_share(off, _csr([[1], [5, 2, 3]])[1], 0)
    h.list_share(*_csr([[1]]), 1)
    assert h._hip.h10x_list_share_get(h._ctx(), None, None, None, 0) == 0
    with pytest.raises(err, match="!! listShare list 1 entry 2: hash index 0 is not in 1 .. %d" % (m.hash_number - 1)):
        h.list_share(off, hsh, 1)
    assert h._hip.h10x_list_share_get(h._ctx(), None, None, None, 0) != 0           # a refused run keeps no rows behind
    with pytest.raises(err, match="!! listShare list 0 entry 0: hash index %d is not in 1 .. %d" % (m.hash_number, m.hash_number - 1)):
        h.list_share(*_csr([[m.hash_number]]), 1)
    got = h.list_share(*_csr([]), 1)
    assert got[0].tolist() == [0] and len(got[1]) == 0
    codes, starts = np.zeros(100, np.uint8), np.array([0, 60, 40, 100], dtype=np.uint64)   # sequence starts that descend: refused before the scan
    assert h._hip.h10x_seq_hashes(h._ctx(), codes.ctypes.data, starts.ctypes.data, 3, None) != 0
    assert "the sequence starts do not ascend at sequence 1" in h._hip.h10x_last_error(h._ctx()).decode()
    e = _hx().Hash10x(B=20)
    with pytest.raises(err, match="no hash state loaded"):
        e.list_share(*_csr([[1]]), 1)
    with pytest.raises(err, match="no hash state loaded"):
        e.seq_blocks([b"ACGT"], 1)
    e.close()


# ------------------------------------------------------------------------------------ both key widths
def test_both_key_widths(tmp_path):
    """One-hash lists cycling through the hashes of a state of 5001 blocks (13 key bits): 2^19 + 1 lists in one batch need 13 + 20 = 33 bits
    and take 64-bit keys, 2^18 lists need 31 and take 32-bit keys. A one-hash list's row is its barcode list's run lengths."""
    n_blocks, n_hash = 5000, 2000
    blocks = [[b % n_hash + 1, b * 7 % n_hash + 1, b * 7 % n_hash + 1, b * 13 % n_hash + 1] for b in range(1, n_blocks + 1)]
    h = orc.load_image(tmp_path, blocks, 2, 100)
    m = sbm.SeqBlocksModel.from_state(h)
    assert m.n_blocks == n_blocks + 1 and m.n_blocks.bit_length() == 13
    rows = [np.unique(m.barcode_list(x), return_counts=True) for x in range(n_hash + 1)]
    length = np.array([len(r[0]) for r in rows]); start = np.concatenate([[0], np.cumsum(length)])
    flat_b = np.concatenate([r[0] for r in rows]).astype(np.uint32); flat_c = np.concatenate([r[1] for r in rows]).astype(np.uint32)
    assert int(flat_c.max()) >= 2 and length[1:].min() >= 1
    for nq, wide in (((1 << 19) + 1, 1), (1 << 18, 0)):
        xs = (np.arange(nq, dtype=np.int64) * 17 % n_hash + 1).astype(np.uint32)
        off = np.arange(nq + 1, dtype=np.uint64)
        for t in (1, 2):
            goff, gblk, gcnt = h.list_share(off, xs, t)
            info = h.seq_blocks_info
            assert (info["wideBatches"], info["batches"], info["windows"], info["lists"]) == (wide, 1, 0, nq)
            assert (n_blocks + 1).bit_length() + (nq - 1).bit_length() == (33 if wide else 31)
            # the expected rows: every list's stretch of the per-hash table, thresholded
            n = length[xs]
            idx = np.repeat(start[xs] - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
            eb, ec = flat_b[idx], flat_c[idx]
            keep = ec >= t
            per = np.add.reduceat(keep.astype(np.int64), np.concatenate([[0], np.cumsum(n)[:-1]]))
            assert np.array_equal(goff, np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)), (nq, t)
            assert np.array_equal(gblk, eb[keep]) and np.array_equal(gcnt, ec[keep]), (nq, t)
            assert info["listEntries"] == int(m.depth[xs].sum()) and info["rows"] == int(keep.sum()) > 0
    h.close()


# ------------------------------------------------------------------------------------ run lengths at the steps of the run search
RUN_LENGTHS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17)                # the search probes at head + 2^j - 1


def test_run_lengths(tmp_path):
    """Hash i + 1 stands RUN_LENGTHS[i] times in block i + 1 and RUN_LENGTHS[(i + 3) % 10] times in block i + 11, and nowhere else: the row of the
    one-hash list [i + 1] is those two blocks with those counts, where they reach the threshold. Ten lists, rotated so that each in turn is the last:
    its second run then ends the batch's key array. Thresholds c - 1, c, c + 1 around that run's length c; every list is checked at each. Budget 2 is
    below every list: each runs alone in windows of block index, its two runs in different windows, so its row count is added to twice."""
    n = len(RUN_LENGTHS)
    table = {i + 1: ((i + 1, RUN_LENGTHS[i]), (i + 1 + n, RUN_LENGTHS[(i + 3) % n])) for i in range(n)}
    blocks = [[] for _ in range(2 * n)]
    for x, runs in table.items():
        for b, c in runs:
            blocks[b - 1] += [x] * c
    h = orc.load_image(tmp_path, blocks, 1, 100)
    seen = set()
    for last in range(n):
        lists = [(last + 1 + j) % n + 1 for j in range(n)]     # one-hash lists, hash last + 1 the last
        off, hsh = _csr([[x] for x in lists])
        c_last = table[lists[-1]][1][1]
        for t in (c_last - 1, c_last, c_last + 1):
            if t < 1:
                continue
            seen.add(t)
            rows = [[(b, c) for b, c in table[x] if c >= t] for x in lists]
            exp = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64),
                   np.array([b for r in rows for b, _ in r], dtype=np.uint32), np.array([c for r in rows for _, c in r], dtype=np.uint32))
            for budget in (0, 2):
                _budget(h, budget)
                _same(h.list_share(off, hsh, t), exp, (last, t, budget))
                info = h.seq_blocks_info
                assert info["rows"] == len(exp[1]) and info["maxCount"] == (int(exp[2].max()) if len(exp[2]) else 0), (last, t, budget)
                assert info["listEntries"] == 2 * sum(RUN_LENGTHS) and info["wideBatches"] == 0
                if budget:
                    assert info["windows"] >= 2 * n and info["batches"] >= 2 * n, info
                else:
                    assert (info["batches"], info["windows"]) == (1, 0), info
    assert seen == {t for c in RUN_LENGTHS for t in (c - 1, c, c + 1) if t >= 1}
    _budget(h, 0)
    h.close()


# ------------------------------------------------------------------------------------ the sequence layer
def _check_sequences(h, m, seqs, thresholds, slabs):
    exp_h = m.seq_hashes(seqs)
    exp = {t: m.seq_blocks(seqs, t) for t in thresholds}
    rc = [sbm.revcomp(s) for s in seqs]
    for slab in slabs:
        h.set_option("seq_slab", slab)
        off, hsh, fig = h.seq_hashes(seqs)
        _same((off, hsh), exp_h[:2], ("seq_hashes", slab))
        assert sbm.figures_equal(fig, exp_h[2]), slab
        roff, rhsh, _ = h.seq_hashes(rc)
        _same((roff, rhsh), (off, hsh), ("reverse complement", slab))
        for t in thresholds:
            got = h.seq_blocks(seqs, t)
            _same(got[:3], exp[t][:3], ("seq_blocks", slab, t))
            assert sbm.figures_equal(got[3], exp[t][3])
            info = h.seq_blocks_info
            assert info["lists"] == len(seqs) and info["listHashes"] == len(hsh) and info["rows"] == len(got[1])
            assert info["listEntries"] == sum(f[3] for f in exp_h[2])
            _same(h.seq_blocks(rc, t)[:3], got[:3], ("rows of the reverse complement", slab, t))
    h.set_option("seq_slab", 0)
    return exp


def test_sequences_on_small():
    recs = cases.small_records()
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(*cases.SMALL_RANGE)
    m = sbm.SeqBlocksModel.from_state(h)
    pairs = cases.sequences(recs)
    seqs = [s for s, _ in pairs]
    assert max(len(s) for s in seqs) > 5000
    # slab 400: a boundary between two reads of 150 bases, and the joined sequences exceed it; 0: everything in one batch
    exp = _check_sequences(h, m, seqs, (1, 5, TOP), (0, 400, 151))
    assert [len(exp[t][1]) for t in (1, 5, TOP)] == [335, 141, 0]                    # the tallies test_seq_blocks_cpu.py pins
    off, blk, cnt, fig = h.seq_blocks(seqs, 1)
    for i, (s, c) in enumerate(pairs):
        if c:
            assert int(fig["found"][i]) == int(fig["moshes"][i])
            assert not fig["query"][i] or c in blk[int(off[i]):int(off[i + 1])].tolist()
    # text goes in as code arrays do
    text = ["".join("ACGT"[c] for c in s).encode() for s in seqs[:5]]
    _same(h.seq_blocks(text, 1)[:3], h.seq_blocks(seqs[:5], 1)[:3], "text")
    # the list census of the lists seq_hashes gives is the row seq_blocks gives; under a small budget too
    qoff, qh, _ = h.seq_hashes(seqs)
    _same(h.list_share(qoff, qh, 5), exp[5][:3], "layer 1 into layer 2 by hand")
    _budget(h, 64)
    h.neighbour_stats(reset=True)
    _same(h.seq_blocks(seqs, 5)[:3], exp[5][:3], "budget 64")
    assert h.seq_blocks_info["windows"] >= 2 and h.neighbour_stats()["batches"] > 3
    _budget(h, 0)
    h.close()


def test_sequences_through_read_hash(tmp_path):
    """a state the reference wrote, through --readHash, works as one from --readFQB"""
    p = tmp_path / "tiny.hash"
    p.write_bytes(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "tiny.hash.gz")))
    h = _hx().Hash10x(B=20)
    h.read_hash(str(p))
    h.depth_range(1, 1 << 30)
    m = sbm.SeqBlocksModel.from_state(h)
    recs = cases.tiny_records()
    seqs = [cases.read2(recs, r) for r in range(len(recs))] + [np.concatenate([cases.read2(recs, r) for r in (0, 4, 9, 0)])]
    exp = _check_sequences(h, m, seqs, (1, 2), (0, 300))
    assert sum(f[2] for f in exp[1][3]) > 51 and len(exp[1][1]) > len(exp[2][1]) > 0
    h.close()


def test_sequences_on_generated_molecules(tmp_path):
    d = str(tmp_path)
    recs = orc.gen_fqb(os.path.join(d, "x.fqb"), *orc.GEN_MOLECULES, fa=os.path.join(d, "x"))
    h = orc.molecules(recs)
    with pytest.raises(_hx().Hash10xError, match="!! you must set hashDepthRange before seqBlocks"):
        h.seq_blocks([np.zeros(100, np.uint8)], 1)                                   # after --clusterSplit until a new range is set
    h.depth_range(2, 40)
    m = sbm.SeqBlocksModel.from_state(h)
    hap = [mm.parse_seq_bytes(open(os.path.join(d, "x.%s.fa" % a), "rb").read())[0][0] for a in "AB"]
    assert len(hap[0]) >= 300000
    seqs = [hap[1][218000:218000 + n] for n in (K - 1, K, K + W - 1, 1000)] + [hap[1][200000:300000], hap[0][0:1000]]
    exp = _check_sequences(h, m, seqs, (1, 50), (0, 2500))
    fig = exp[1][3]
    assert fig[0] == (0, 0, 0, 0) and fig[1] == (1, 1, 1, 2) and fig[2] == (4, 4, 4, 8) and fig[3] == (34, 31, 31, 62)
    assert fig[4] == (3227, 2037, 627, 1399)                                         # the long stretch: many hashes, some absent
    assert len(exp[1][1]) > len(exp[50][1]) > 0
    h.close()



def test_gapped_contig(tmp_path):
    """a contig with an assembly gap lists more moshes than the estimate its batch's list is sized by (moshScanWith with no accumulators): every batch that
    holds it is scanned twice, and its hash list and row are those of the same contig with the gap cut down to 30 bases (the list is a set)"""
    d = str(tmp_path)
    h, m, seqs, left, right = cases.gapped_state(d)
    assert h.counters()["scan_retries"] == 0
    plain = [seqs["control"], seqs["N30"], right]
    _check_sequences(h, m, plain, (1, 5), (0, 50000))
    assert h.counters()["scan_retries"] == 0                                         # random sequence of the same length does not overflow
    gapped = [seqs["N"], seqs["N30"], right, seqs["T"], seqs["T30"], left[:K - 1]]
    exp = _check_sequences(h, m, gapped, (1, 5), (0, 50000, 300000))
    # slab 0: one batch; 50000: the two gapped contigs alone; 300000: [N, N30, right], [T, T30, left]; 2 + 2 * 2 scans of sequences and of their reverse complements each
    assert h.counters()["scan_retries"] == 6 * (1 + 2 + 2)
    off, hsh, fig = h.seq_hashes(gapped)
    rows = h.seq_blocks(gapped, 1)
    for a, b in ((0, 1), (3, 4)):
        assert hsh[int(off[a]):int(off[a + 1])].tolist() == hsh[int(off[b]):int(off[b + 1])].tolist() and int(off[a + 1] - off[a]) > 100
        ra, rb = [(x[int(rows[0][i]):int(rows[0][i + 1])].tolist() for x in rows[1:3]) for i in (a, b)]
        assert [list(x) for x in ra] == [list(x) for x in rb]
        assert int(fig["moshes"][a]) - int(fig["moshes"][b]) == 100000 - 30 and int(fig["query"][a]) == int(fig["query"][b])
    ix = orc.value0_depth(orc.HashFile(cases.state_bytes(h, d)))[0]
    assert ix in hsh[int(off[0]):int(off[1])].tolist()                               # the gap's own hash is in the state and in range: it is in the list, once
    # the command: SEQ_BLOCKS prints moshes larger by the gap
    names = ["gapN", "shortN", "right", "gapT", "shortT", "tiny"]
    with open(os.path.join(d, "c.fa"), "w") as f:
        f.write("".join(">%s\n%s\n" % (n, "".join("ACGT"[c] for c in s) if "N" not in n else "".join("ACGT"[c] for c in s[:20000]) + "N" * (len(s) - 40000) +
                                       "".join("ACGT"[c] for c in s[-20000:])) for n, s in zip(names, gapped)))
    before = h.counters()["scan_retries"]
    h.write_seq_blocks(1, os.path.join(d, "c.fa"), os.path.join(d, "c.sb"), out=os.path.join(d, "c.out"), verbose=True)
    assert h.counters()["scan_retries"] == before + 1
    lines = {ln[0]: [int(v) for v in ln[1:]] for ln in VERBOSE.findall(open(os.path.join(d, "c.out")).read())}
    assert lines["gapN"][1] - lines["shortN"][1] == 100000 - 30 == lines["gapT"][1] - lines["shortT"][1]
    assert lines["gapN"][2] - lines["shortN"][2] == 100000 - 30                      # value 0 is in the state: every mosh of the gap is found
    assert lines["gapN"][3:] == lines["shortN"][3:] and lines["gapT"][3:] == lines["shortT"][3:] and lines["gapN"][3] > 100   # query, rows, best, count
    info, roff, rblk, rcnt, table, rnames = _hx().read_seq_blocks(os.path.join(d, "c.sb"))
    _same((roff, rblk, rcnt), exp[1][:3], "the .sb file")
    h.close()


# ------------------------------------------------------------------------------------ kept results
def test_kept_results():
    recs = cases.small_records()
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(*cases.SMALL_RANGE)
    seqs = [s for s, _ in cases.sequences(recs)]
    hc = h.hash_copies(5).copy()
    sg = [a.copy() for a in h.share_graph(5)]
    a = h.seq_blocks(seqs, 2)
    b = h.seq_blocks(seqs, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))                    # two calls give equal bytes
    h.seq_hashes(seqs)
    h.list_share(*_csr([[1, 2]]), 1)
    n = h.sizes()["hashNumber"]
    out = np.zeros((n, 4), dtype=np.uint16)
    h._chk_ctx(h._hip.h10x_hash_copies_get(h._ctx(), out.ctypes.data, 0, n))
    assert out.tobytes() == hc.tobytes()
    off, blk, cnt = np.zeros_like(sg[0]), np.zeros_like(sg[1]), np.zeros_like(sg[2])
    h._chk_ctx(h._hip.h10x_share_graph_get(h._ctx(), off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, len(blk)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip((off, blk, cnt), sg))
    assert h._hip.h10x_list_share_get(h._ctx(), None, None, None, 0) == 0 and h._hip.h10x_seq_hashes_get(h._ctx(), None, None, 0) == 0
    h.depth_range(*cases.SMALL_RANGE)                                                # a new range releases the rows and the lists
    assert h._hip.h10x_list_share_get(h._ctx(), None, None, None, 0) != 0 and h._hip.h10x_seq_hashes_get(h._ctx(), None, None, 0) != 0
    with pytest.raises(_hx().Hash10xError, match="!! seqBlocks minShare 0 must be >= 1"):
        h.seq_blocks(seqs[:2], 0)
    h.read_fqb(recs)
    with pytest.raises(_hx().Hash10xError, match="!! you must set hashDepthRange before seqBlocks"):
        h.seq_blocks(seqs[:2], 1)
    h.close()


# ------------------------------------------------------------------------------------ the command through bin/hash10x-amd
EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
SUMMARY = re.compile(r"^  seq blocks at minShare (\d+): (\d+) sequences, (\d+) bases, (\d+) moshes, (\d+) found, (\d+) in range, (\d+) rows, "
                     r"(\d+) sequences with rows, max count (\d+)$", re.M)
VERBOSE = re.compile(r"^SEQ_BLOCKS  (\S+) len (\d+) moshes (\d+) found (\d+) query (\d+) rows (\d+) best (\d+) count (\d+)$", re.M)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """small.fqb and its test sequences as plain FASTA, gzipped FASTA and FASTQ (the joins written as Ns), with the model's result at T = 2"""
    d = str(tmp_path_factory.mktemp("sbcli"))
    recs = cases.small_records()
    recs.tofile(os.path.join(d, "x.fqb"))
    seqs = [s for s, _ in cases.sequences(recs) if len(s)]
    names = ["seq%d" % i for i in range(len(seqs))]
    text = []
    for s in seqs:
        t = "".join("ACGT"[c] for c in s)
        text.append(t.replace("AAAAA", "NNNNN", 1) if len(s) > 1000 else t)
    fa = "".join(">%s read %d\tmore\n%s\n" % (n, i, "\n".join(t[a:a + 60] for a in range(0, len(t), 60))) for i, (n, t) in enumerate(zip(names, text)))
    with open(os.path.join(d, "s.fa"), "w") as f:
        f.write(fa)
    with gzip.open(os.path.join(d, "s.fa.gz"), "wb") as f:
        f.write(fa.encode())
    with open(os.path.join(d, "s.fq"), "w") as f:
        f.write("".join("@%s x\n%s\n+\n%s\n" % (n, t, "I" * len(t)) for n, t in zip(names, text)))
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(*cases.SMALL_RANGE)
    m = sbm.SeqBlocksModel.from_state(h)
    coded = [_hx().Hash10x._flatten_seqs([t.encode()])[0] for t in text]
    yield d, h, m.seq_blocks(coded, 2), names, [len(s) for s in seqs], m.n_blocks
    h.close()


def _run(d, *args, stdin=None):
    p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_cli(cli):
    d, h, (off, blk, cnt, fig), names, lens, n_blocks = cli
    base = ["-B", 20, "--readFQB", "x.fqb", "--hashDepthRange", 3, 14]
    rc, out, err = _run(d, *base, "--verbose", "--seqBlocks", 2, "s.fa", "x.sb")
    assert rc == 0, err
    info, roff, rblk, rcnt, table, rnames = _hx().read_seq_blocks(os.path.join(d, "x.sb"))
    assert info == {"version": 1, "nBlocks": n_blocks, "minShare": 2, "nSeq": len(names), "rows": len(blk), "nameBytes": sum(len(n) + 1 for n in names)}
    _same((roff, rblk, rcnt), (off, blk, cnt), "cli")
    assert rnames == names and len(blk) > 100
    assert [(int(r["len"]), int(r["moshes"]), int(r["found"]), int(r["query"])) for r in table] == [(n,) + f[:3] for n, f in zip(lens, fig)]
    expected = sbm.sb_bytes(n_blocks, 2, lens, off, blk, cnt, fig, names)
    image = open(os.path.join(d, "x.sb"), "rb").read()
    assert image == expected
    n_rows = np.diff(off.astype(np.int64))
    m = SUMMARY.search(out)
    assert m and [int(v) for v in m.groups()] == [2, len(names), sum(lens), sum(f[0] for f in fig), sum(f[1] for f in fig), sum(f[2] for f in fig),
                                                 len(blk), int((n_rows > 0).sum()), int(cnt.max())]
    lines = VERBOSE.findall(out)
    assert len(lines) == len(names)
    for i, ln in enumerate(lines):
        a, b = int(off[i]), int(off[i + 1])
        best = (int(blk[a + int(np.argmax(cnt[a:b]))]), int(cnt[a:b].max())) if b > a else (0, 0)   # argmax: the lowest block on ties
        assert (ln[0],) + tuple(int(v) for v in ln[1:]) == (names[i], lens[i]) + fig[i][:3] + (b - a,) + best, i
    # gzip and FASTQ give the same file; without --verbose there are no SEQ_BLOCKS lines
    for src in ("s.fa.gz", "s.fq"):
        rc, out, err = _run(d, *base, "--seqBlocks", 2, src, "y.sb")
        assert rc == 0 and open(os.path.join(d, "y.sb"), "rb").read() == image and "SEQ_BLOCKS" not in out and SUMMARY.search(out), (src, err)
    assert not [n for n in os.listdir(d) if n.endswith(".part")]
    # the session call, in slabs of 400 bases: the same bytes
    h.set_option("seq_slab", 400)
    h.write_seq_blocks(2, os.path.join(d, "s.fa"), os.path.join(d, "z.sb"), out=os.path.join(d, "z.out"), verbose=True)
    h.set_option("seq_slab", 0)
    assert open(os.path.join(d, "z.sb"), "rb").read() == image and len(VERBOSE.findall(open(os.path.join(d, "z.out")).read())) == len(names)
    # --interactive takes it too
    rc, out, err = _run(d, "-B", 20, "--interactive", stdin=b"readFQB x.fqb\nhashDepthRange 3 14\nseqBlocks 2 s.fa i.sb\nquit\n")
    assert rc == 0 and open(os.path.join(d, "i.sb"), "rb").read() == image


def test_cli_refusals(cli):
    d = cli[0]
    gone = lambda name: not os.path.exists(os.path.join(d, name)) and not os.path.exists(os.path.join(d, name + ".part"))
    base = ["-B", 20, "--readFQB", "x.fqb"]
    rc, out, err = _run(d, "--seqBlocks", 2, "s.fa", "none.sb")                      # no state
    assert rc == 0 and "!! you must set hashDepthRange before seqBlocks\n" in out and gone("none.sb")
    rc, out, err = _run(d, *base, "--seqBlocks", 2, "s.fa", "early.sb")
    assert rc == 0 and "!! you must set hashDepthRange before seqBlocks\n" in out and gone("early.sb")
    rc, out, err = _run(d, "-o", "soft.out", *base, "--hashDepthRange", 3, 14, "--seqBlocks", 0, "s.fa", "zero.sb", "--cluster", 1, 0, "--clusterSplit",
                        "--seqBlocks", 5, "s.fa", "late.sb")
    assert rc == 0, err
    for msg in ("!! seqBlocks minShare 0 must be >= 1\n", "!! you must set hashDepthRange before seqBlocks\n"):
        assert msg in err and msg in open(os.path.join(d, "soft.out")).read()
    assert gone("zero.sb") and gone("late.sb")
    rc, out, err = _run(d, *base, "--hashDepthRange", 3, 14, "--seqBlocks", 2, "nosuch.fa", "a.sb")
    assert rc == 255 and "FATAL ERROR: " in err and "failed to open sequence file nosuch.fa\n" in err and gone("a.sb")
    rc, out, err = _run(d, *base, "--hashDepthRange", 3, 14, "--seqBlocks", 2, "s.fa", "nodir/b.sb")
    assert rc == 255 and "FATAL ERROR: failed to open output file nodir/b.sb\n" in err and not os.path.exists(os.path.join(d, "nodir"))
    rc, out, err = _run(d, "--gpus", 2, *base, "--hashDepthRange", 3, 14, "--seqBlocks", 2, "s.fa", "s.sb")
    assert rc == 255 and "FATAL ERROR: --seqBlocks does not run on a sharded session (--gpus 2)" in err and gone("s.sb")
