"""Row links and sequence links on the GPU (csrc/stage_q.hip): Hash10x.row_links / seq_links against the plain-numpy model of the definition
(tests/seqlinks_model.py) on hand-made rows, the small golden set and a generated genome; the cut into add calls, the batching, both key
widths, the kept results, the refusals, the command line and the .sl file. Every comparison is exact equality."""
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
import seqlinks_model as slm

pytestmark = pytest.mark.gpu

TOP = 2 ** 31 - 1
K, W = cases.K, cases.W
_hx, _budget = orc.hx, orc.set_budget
FIGURES = ("lists", "rowEntries", "blocksUsed", "skippedBlocks", "pairs", "links", "maxShared")


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("offsets", "other", "shared")):
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, name)


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(q) for q in lists])
    return off, np.concatenate([np.asarray(q, dtype=np.uint32) for q in lists] + [np.zeros(0, np.uint32)])


def _check(h, off, blk, n_blocks, min_blocks, max_lists, sib, what=None):
    got = h.row_links(off, blk, min_blocks, max_lists, sib, n_blocks=n_blocks)
    exp = slm.row_links(off, blk, min_blocks, max_lists, sib)
    _same(got, exp[:3], what or (min_blocks, max_lists, sib))
    assert {k: h.row_links_info[k] for k in FIGURES} == exp[3], (what, h.row_links_info, exp[3])
    return got


# ------------------------------------------------------------------------------------ hand-made rows
N_BLOCKS = 1000


def _hand_rows():
    """blocks 10, 11, 12 and 13 stand in the first 63, 64, 65 and 257 lists (the wave and workgroup edges of the pair gather); block 0 in
    lists 3 and 5, block 999 in lists 5, 7 and 300; lists 257 .. 299 are empty; lists 301 and 302 are identical; 303 is empty"""
    lists = [[] for _ in range(304)]
    for d, n in ((10, 63), (11, 64), (12, 65), (13, 257)):
        for e in range(n):
            lists[e].append(d)
    for e in (3, 5):
        lists[e].insert(0, 0)
    for e in (5, 7, 300):
        lists[e].append(N_BLOCKS - 1)
    lists[301] = [0, 500, N_BLOCKS - 1]
    lists[302] = [0, 500, N_BLOCKS - 1]
    return lists


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    """a small hand-made state: the row layer needs a context, and add_kept the rows of a list census"""
    blocks = [[b % 7 + 1, b % 5 + 1, b % 3 + 8] for b in range(1, 41)]
    h = orc.load_image(tmp_path_factory.mktemp("slh"), blocks, 2, 100)
    yield h
    h.close()


def test_hand_made_rows(hand):
    h = hand
    lists = _hand_rows()
    assert sorted({len(q) for q in lists})[:2] == [0, 1] and lists[301] == lists[302]
    off, blk = _csr(lists)
    results = {}
    for sib in (False, True):
        for max_lists in (0, 2, 63, 64, 65, 256, 257):         # at 64: block 11 stands in exactly maxLists lists, block 12 in maxLists + 1
            for min_blocks in (1, 2, 3, 4, TOP):
                results[(sib, max_lists, min_blocks)] = _check(h, off, blk, N_BLOCKS, min_blocks, max_lists, sib)
    info = h.row_links_info
    assert info["links"] == 0 and info["lists"] == 304 and info["batches"] == 1 and info["windows"] == 0 and info["wideBatches"] == 0
    o, f, c = results[(False, 0, 1)]
    row = lambda e: (f[int(o[e]):int(o[e + 1])].tolist(), c[int(o[e]):int(o[e + 1])].tolist())
    assert row(0) == (list(range(1, 257)), [4] * 62 + [3, 2] + [1] * 192)            # lists 1 .. 62 hold all four blocks, 63 three, 64 two
    assert row(5)[0][-3:] == [300, 301, 302] and row(300) == ([301, 302], [1, 1]) and row(301) == ([302], [3]) and row(303) == ([], [])
    assert row(3)[0][-2:] == [301, 302] and row(256) == ([], []) and row(280) == ([], [])
    assert row(0)[1] == results[(False, 257, 1)][2][:256].tolist() and results[(False, 256, 1)][2][:64].tolist() == [3] * 62 + [2, 1]
    assert results[(True, 0, 1)][1][:3].tolist() == [2, 3, 4]                        # list 1 is list 0's sibling
    assert len(results[(False, 0, 4)][1]) == 63 * 62 // 2 and not results[(False, 0, TOP)][0].any()
    # the cap boundary in the figures: at 64 blocks 10, 11 (and 0, 500, 999) are used, 12 and 13 are not
    h.row_links(off, blk, 1, 64, n_blocks=N_BLOCKS)
    assert (h.row_links_info["blocksUsed"], h.row_links_info["skippedBlocks"]) == (5, 2)
    h.row_links(off, blk, 1, 65, n_blocks=N_BLOCKS)
    assert (h.row_links_info["blocksUsed"], h.row_links_info["skippedBlocks"]) == (6, 1)
    # no lists at all, and lists that are all empty
    got = h.row_links(*_csr([]), 1, n_blocks=5)
    assert got[0].tolist() == [0] and len(got[1]) == 0 and h.row_links_info["lists"] == 0
    got = h.row_links(*_csr([[], [], []]), 1, n_blocks=5)
    assert got[0].tolist() == [0, 0, 0, 0] and h.row_links_info["lists"] == 3 and h.row_links_info["rowEntries"] == 0


def test_list_refusals(hand):
    h = hand
    err = _hx().Hash10xError
    ok = _csr([[1, 2], [2, 3]])
    assert h.row_links(*ok, 1, n_blocks=4)[1].tolist() == [1]
    with pytest.raises(err, match="!! rowLinks list 1 entry 2: block 4 is not ascending"):
        h.row_links(*_csr([[1], [3, 4, 4]]), 1, n_blocks=5)
    assert h._hip.h10x_row_links_get(h._ctx(), None, None, None, 0) != 0             # a begin releases the links kept before
    with pytest.raises(err, match="!! rowLinks list 1 entry 1: block 2 is not ascending"):
        h.row_links(*_csr([[1], [3, 2]]), 1, n_blocks=5)
    with pytest.raises(err, match="!! rowLinks list 0 entry 1: block 5 is not below 5"):
        h.row_links(*_csr([[1, 5]]), 1, n_blocks=5)
    with pytest.raises(err, match="!! seqLinks minBlocks 0 must be >= 1"):
        h.row_links(*ok, 0, n_blocks=4)
    # the list number counts over all lists added, and a refused add appends nothing
    ctx, hip = h._ctx(), h._hip
    assert hip.h10x_row_links_begin(ctx, 5) == 0 and hip.h10x_row_links_add(ctx, ok[0].ctypes.data, ok[1].ctypes.data, 2) == 0
    bad = _csr([[0], [4, 3]])
    assert hip.h10x_row_links_add(ctx, bad[0].ctypes.data, bad[1].ctypes.data, 2) != 0
    assert "!! rowLinks list 3 entry 1: block 3 is not ascending" in hip.h10x_last_error(ctx).decode()
    info, got = h._row_links_finish(ctx, 1, 0, False)
    assert info["lists"] == 2 and got[1].tolist() == [1]
    e = _hx().Hash10x(B=20)
    with pytest.raises(err, match="no hash state loaded"):
        e.row_links(*ok, 1, n_blocks=4)
    with pytest.raises(err, match="no hash state loaded"):
        e.seq_links([b"ACGT"], 1, 1, 100)
    e.close()


# ------------------------------------------------------------------------------------ independence of the cut and of the budget
def _by_hand(h, parts, n_blocks, min_blocks, max_lists=0, sib=False, kept=None):
    """begin, one add per part ((offsets, block) or the word "kept": kept() runs the list census, then add_kept), finish"""
    ctx, hip = h._ctx(), h._hip
    h._chk_ctx(hip.h10x_row_links_begin(ctx, n_blocks))
    for p in parts:
        if isinstance(p, str):
            kept()
            h._chk_ctx(hip.h10x_row_links_add_kept(ctx))
        else:
            h._chk_ctx(hip.h10x_row_links_add(ctx, p[0].ctypes.data, p[1].ctypes.data, len(p[0]) - 1))
    return h._row_links_finish(ctx, min_blocks, max_lists, sib)


def test_independence_of_the_cut(hand):
    h = hand
    lists = _hand_rows()
    off, blk = _csr(lists)
    whole = {mb: h.row_links(off, blk, mb, 64, True, n_blocks=N_BLOCKS) for mb in (1, 2)}
    for mb in (1, 2):
        info, got = _by_hand(h, [_csr([q]) for q in lists], N_BLOCKS, mb, 64, True)
        _same(got, whole[mb], ("one add per list", mb))
        info, got = _by_hand(h, [_csr(lists[:100]), _csr([]), _csr(lists[100:257]), _csr(lists[257:])], N_BLOCKS, mb, 64, True)
        _same(got, whole[mb], ("four adds", mb))
        assert info["lists"] == 304 and info["rowEntries"] == len(blk)
    # through add_kept: the rows of a list census on the hand-made state are the lists
    n_blocks = h.sizes()["nBlocks"]
    qs = [[1, 2], [3], [], [8, 9, 10], [1, 2, 3, 4, 5, 6, 7], [10]]
    qoff, qh = _csr(qs)
    roff, rblk, _ = h.list_share(qoff, qh, 1)
    assert len(rblk) > 40 and all(np.all(np.diff(rblk[int(a):int(b)].astype(np.int64)) > 0) for a, b in zip(roff[:-1], roff[1:]))
    extra = _csr([[1, 5, 40], [5, 40]])
    both_off = np.concatenate([roff, roff[-1] + extra[0][1:], roff[-1] + extra[0][-1] + roff[1:]])
    both_blk = np.concatenate([rblk, extra[1], rblk])
    for mb, cap, sib in ((1, 0, False), (2, 0, True), (3, 5, False)):
        exp = slm.row_links(both_off, both_blk, mb, cap, sib)
        info, got = _by_hand(h, ["kept", extra, "kept"], n_blocks, mb, cap, sib, kept=lambda: h.list_share(qoff, qh, 1))
        _same(got, exp[:3], ("add_kept", mb, cap, sib))
        assert {k: info[k] for k in FIGURES} == exp[3] and info["lists"] == 14
        _same(h.row_links(both_off, both_blk, mb, cap, sib), got, ("the same rows from the host", mb))
    # add_kept without kept rows, and with rows of more blocks than the accumulator takes
    h.depth_range(2, 100)                                         # a new range releases the kept rows
    ctx, hip = h._ctx(), h._hip
    assert hip.h10x_row_links_begin(ctx, n_blocks) == 0 and hip.h10x_row_links_add_kept(ctx) != 0
    assert "no rows are kept" in hip.h10x_last_error(ctx).decode()
    h.list_share(qoff, qh, 1)
    assert hip.h10x_row_links_begin(ctx, n_blocks - 1) == 0 and hip.h10x_row_links_add_kept(ctx) != 0
    assert hip.h10x_row_links_begin(ctx, n_blocks) == 0 and hip.h10x_row_links_add_kept(ctx) == 0


def test_budget_batches_and_windows(hand):
    h = hand
    off, blk = _csr(_hand_rows())
    exp = {(mb, cap): h.row_links(off, blk, mb, cap, n_blocks=N_BLOCKS) for mb in (1, 3) for cap in (0, 64)}
    assert h.row_links_info["batches"] == 1 and h.row_links_info["windows"] == 0
    for budget in (40, 300):                                      # list 0 alone gathers 256 + 64 + 63 + 62 = 445 pairs, 125 under the cap of 64
        _budget(h, budget)
        h.neighbour_stats(reset=True)
        for (mb, cap), e in exp.items():
            _same(h.row_links(off, blk, mb, cap, n_blocks=N_BLOCKS), e, (budget, mb, cap))
            info = h.row_links_info
            assert info["batches"] > 3 and info["wideBatches"] == 0 and (info["windows"] >= 2 or (budget == 300 and cap == 64)), info
        s = h.neighbour_stats(reset=True)
        assert s["windows"] >= 2 and s["batches"] > 6, s
    _budget(h, 0)


# ------------------------------------------------------------------------------------ both key widths
def test_both_key_widths(hand):
    """n lists of one block each, block = i mod 3000: list e is linked to e + 3000, e + 6000, ... with shared 1. 65537 lists need 17 bits of
    list and 17 of slot: 64-bit pair keys; 32768 lists need 15 + 15: 32-bit keys."""
    h = hand
    for n, wide in ((65537, 1), (32768, 0)):
        blk = (np.arange(n, dtype=np.int64) % 3000).astype(np.uint32)
        off = np.arange(n + 1, dtype=np.uint64)
        goff, gother, gshared = h.row_links(off, blk, 1, n_blocks=3000)
        info = h.row_links_info
        assert (info["wideBatches"] >= 1) == bool(wide) and info["batches"] == 1 and info["windows"] == 0 and info["lists"] == n, info
        per = (n - 1 - np.arange(n, dtype=np.int64)) // 3000       # the later lists of the same residue
        eoff = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
        e = np.repeat(np.arange(n, dtype=np.int64), per)
        eother = (e + 3000 * (np.arange(len(e), dtype=np.int64) - eoff[:-1].astype(np.int64)[e] + 1)).astype(np.uint32)
        assert np.array_equal(goff, eoff) and np.array_equal(gother, eother) and np.array_equal(gshared, np.ones(len(e), np.uint32))
        assert info["links"] == info["pairs"] == len(e) > 100000 and info["blocksUsed"] == 3000 and info["maxShared"] == 1
        got2 = h.row_links(off, blk, 2, n_blocks=3000)
        assert not got2[0].any() and len(got2[1]) == 0
        if wide:
            cap = h.row_links(off, blk, 1, 21, n_blocks=3000)      # residues 0 .. 2536 stand in 22 lists, the others in 21
            keep = (e % 3000) > 2536
            assert np.array_equal(cap[1], eother[keep]) and h.row_links_info["skippedBlocks"] == 2537


# ------------------------------------------------------------------------------------ sequences
def _swap(dct):
    """the links with every end replaced by its sequence's other end"""
    return {(min(e ^ 1, f ^ 1), max(e ^ 1, f ^ 1)): c for (e, f), c in dct.items()}


def _check_sequences(h, m, seqs, cases_, slabs):
    rc = [sbm.revcomp(s) for s in seqs]
    out = {}
    for min_share, min_blocks, end_len, max_ends in cases_:
        exp = slm.seq_links(m, seqs, min_share, min_blocks, end_len, max_ends)
        for slab in slabs:
            h.set_option("seq_slab", slab)
            got = h.seq_links(seqs, min_share, min_blocks, end_len, max_ends)
            _same(got, exp[:3], ("seq_links", min_share, min_blocks, end_len, max_ends, slab))
            assert {k: h.seq_links_info[k] for k in FIGURES} == exp[3]
        if end_len:
            got_rc = h.seq_links(rc, min_share, min_blocks, end_len, max_ends)
            assert slm.as_dict(*got_rc) == _swap(slm.as_dict(*got)), ("reverse complement", end_len)
        out[(min_share, min_blocks, end_len, max_ends)] = got
    h.set_option("seq_slab", 0)
    return out


def test_sequences_on_small():
    recs = cases.small_records()
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(*cases.SMALL_RANGE)
    m = sbm.SeqBlocksModel.from_state(h)
    seqs = [s for s, _ in cases.sequences(recs)]
    got = _check_sequences(h, m, seqs, [(1, 1, 0, 0), (1, 1, 100, 0), (1, 1, 100, 8), (2, 1, 2500, 0), (1, 2, 2500, 8), (1, TOP, 100, 0)], (0, 400, 151))
    assert len(got[(1, 1, 100, 0)][1]) > len(got[(1, 1, 100, 8)][1]) > len(got[(1, 2, 2500, 8)][1]) > 0 and len(got[(1, TOP, 100, 0)][1]) == 0
    # end_len 0: the even ends carry the whole sequences' rows, the odd ends nothing
    o = got[(1, 1, 0, 0)][0].astype(np.int64)
    assert len(got[(1, 1, 0, 0)][1]) > 0 and not np.any(np.diff(o)[1::2]) and not np.any(got[(1, 1, 0, 0)][1] & 1)
    # text goes in as code arrays do
    text = ["".join("ACGT"[c] for c in s).encode() for s in seqs[:8]]
    _same(h.seq_links(text, 1, 1, 100), h.seq_links(seqs[:8], 1, 1, 100), "text")
    with pytest.raises(_hx().Hash10xError, match="!! seqLinks minShare 0 must be >= 1"):
        h.seq_links(seqs[:2], 0, 1, 100)
    with pytest.raises(_hx().Hash10xError, match="!! seqLinks minBlocks 0 must be >= 1"):
        h.seq_links(seqs[:2], 1, 0, 100)
    with pytest.raises(_hx().Hash10xError, match="!! seqLinks endLen -1 must be >= 0"):
        h.seq_links(seqs[:2], 1, 1, -1)
    h.close()


def test_gapped_contigs(tmp_path):
    """the ends of contigs with an assembly gap (end_len 0: whole contigs; 70 000: each end holds half the gap) list more moshes than the estimate: the
    batch is scanned twice and the links are the model's, which are those of the contigs with the gap cut down to 30 bases"""
    d = str(tmp_path)
    h, m, seqs, left, right = cases.gapped_state(d)
    cases_ = [(1, 1, 0, 0), (1, 2, 70000, 0), (2, 1, 70000, 8)]
    _check_sequences(h, m, [seqs["control"], seqs["N30"], right, left], cases_, (0,))
    assert h.counters()["scan_retries"] == 0
    gapped = [seqs["N"], seqs["T"], right, left]
    got = _check_sequences(h, m, gapped, cases_, (0, 150000))
    # end_len 0: one batch (slab 0), then each gapped contig alone (slab 150000). end_len 70000: one batch, then the two ends of a gapped contig together
    # in a batch of their own, and the same for the reverse complements. (An end alone cannot overflow: its estimate is all of its k-mers.)
    assert h.counters()["scan_retries"] == (1 + 2) + 2 * (1 + 2 + 2)
    short = _check_sequences(h, m, [seqs["N30"], seqs["T30"], right, left], cases_[:1], (0,))
    assert slm.as_dict(*got[cases_[0]]) == slm.as_dict(*short[cases_[0]]) and len(got[cases_[0]][1]) >= 5
    h.close()


def test_sequences_on_the_generated_genome(tmp_path):
    """the set of tests/test_seq_links_cpu.py's ground truth, clustered and split on the GPU: the GPU's links meet the same conditions"""
    d = str(tmp_path)
    recs = orc.gen_fqb(os.path.join(d, "x.fqb"), 40000, 300, 600000, 0.003, 7, 4.0, 150, 5000, fa=os.path.join(d, "x"))
    h = _hx().Hash10x(B=21)
    h.read_fqb(recs)
    h.depth_range(4, 60)
    h.cluster(1, 0, 3)
    h.cluster_split()
    with pytest.raises(_hx().Hash10xError, match="!! you must set hashDepthRange before seqLinks"):
        h.seq_links([np.zeros(100, np.uint8)], 1, 1, 100)                            # after --clusterSplit until a new range is set
    h.depth_range(4, 60)
    m = sbm.SeqBlocksModel.from_state(h)
    hap = [mm.parse_seq_bytes(open(os.path.join(d, "x.%s.fa" % a), "rb").read())[0][0] for a in "AB"]
    pieces = [x[a:a + 10000] for x in hap for a in range(0, len(x), 10000)]
    per = len(pieces) // 2
    got = _check_sequences(h, m, pieces, [(2, 3, 2500, 0), (2, 5, 2500, 0), (2, 5, 2500, 8), (2, 1, 100, 0), (2, 2, 0, 8)], (0, 25000))
    assert m.n_blocks == 1697 and h.seq_links_info["lists"] == 240
    junctions = [(2 * (k * per + i) + 1, 2 * (k * per + i + 1)) for k in range(2) for i in range(per - 1)]
    at3, at5 = slm.as_dict(*got[(2, 3, 2500, 0)]), slm.as_dict(*got[(2, 5, 2500, 0)])
    assert len(junctions) == 118 and all(j in at3 for j in junctions)
    near = sum(abs((e >> 1) % per - (f >> 1) % per) <= 1 for e, f in at5)
    assert near >= 0.95 * len(at5) and sum(j in at5 for j in junctions) >= 0.9 * len(junctions) and len(at5) > 100
    h.close()


# ------------------------------------------------------------------------------------ kept results
def test_kept_results():
    recs = cases.small_records()
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(*cases.SMALL_RANGE)
    seqs = [s for s, _ in cases.sequences(recs)]
    ctx, hip = h._ctx(), h._hip
    kept = lambda: hip.h10x_row_links_get(ctx, None, None, None, 0) == 0
    assert not kept()
    assert hip.h10x_row_links_begin(ctx, 10) == 0 and not kept()                      # get before finish fails
    hc = h.hash_copies(5).copy()
    sg = [a.copy() for a in h.share_graph(5)]
    sb = [a.copy() for a in h.seq_blocks(seqs, 2)[:3]]
    a = h.seq_links(seqs, 1, 1, 100)
    b = h.seq_links(seqs, 1, 1, 100)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[1]) > 0 and kept()   # two calls give equal bytes
    # a second finish on the same accumulator, with other arguments
    info, c2 = h._row_links_finish(ctx, 2, 0, True)
    assert info["lists"] == 2 * len(seqs) and 0 < len(c2[1]) < len(a[1])
    # the device copy is the host copy (device memory from the HIP runtime the library itself is linked to)
    import ctypes
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]; hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    dev = [ctypes.c_void_p() for _ in range(3)]
    for p, x in zip(dev, c2):
        assert hip.hipMalloc(ctypes.byref(p), x.nbytes) == 0
    h._chk_ctx(hip.h10x_row_links_get_device(ctx, dev[0], dev[1], dev[2], len(c2[1])))
    for p, x in zip(dev, c2):
        back = np.zeros_like(x)
        assert hip.hipMemcpy(back.ctypes.data, p, x.nbytes, 2) == 0 and np.array_equal(back, x)   # 2 = hipMemcpyDeviceToHost
        assert hip.hipFree(p) == 0
    part_o, part_s = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    h._chk_ctx(hip.h10x_row_links_get_range(ctx, 2, 3, part_o.ctypes.data, part_s.ctypes.data))
    assert np.array_equal(part_o, c2[1][2:5]) and np.array_equal(part_s, c2[2][2:5])
    assert hip.h10x_row_links_get_range(ctx, len(c2[1]) - 1, 2, part_o.ctypes.data, part_s.ctypes.data) != 0
    # the other kept results survive: hash copies, the share graph (seq_links itself replaces the seqBlocks rows: it runs seq_blocks)
    n = h.sizes()["hashNumber"]
    out = np.zeros((n, 4), dtype=np.uint16)
    h._chk_ctx(hip.h10x_hash_copies_get(ctx, out.ctypes.data, 0, n))
    assert out.tobytes() == hc.tobytes()
    off, blk, cnt = np.zeros_like(sg[0]), np.zeros_like(sg[1]), np.zeros_like(sg[2])
    h._chk_ctx(hip.h10x_share_graph_get(ctx, off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, len(blk)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip((off, blk, cnt), sg))
    # the row layer from the host leaves the kept seqBlocks rows alone
    h.seq_blocks(seqs, 2)
    h.row_links(*_csr([[1, 2], [2]]), 1)
    off, blk, cnt = np.zeros_like(sb[0]), np.zeros_like(sb[1]), np.zeros_like(sb[2])
    h._chk_ctx(hip.h10x_list_share_get(ctx, off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, len(blk)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip((off, blk, cnt), sb)) and kept()
    # begin, a new range and --clusterSplit release the links and the accumulator
    assert hip.h10x_row_links_begin(ctx, 10) == 0 and not kept()
    h.row_links(*_csr([[1, 2], [2]]), 1)
    assert kept()
    h.depth_range(*cases.SMALL_RANGE)
    assert not kept() and hip.h10x_row_links_add(ctx, _csr([[1]])[0].ctypes.data, _csr([[1]])[1].ctypes.data, 1) != 0
    assert "no accumulator is open" in hip.h10x_last_error(ctx).decode()
    h.row_links(*_csr([[1, 2], [2]]), 1)
    h.cluster(1, 0, 2)
    assert kept()
    h.cluster_split()
    assert not kept()
    h.row_links(*_csr([[1, 2], [2]]), 1)
    h.read_fqb(recs)                                               # a new state
    assert not h._hip.h10x_row_links_get(h._ctx(), None, None, None, 0) == 0
    h.close()


# ------------------------------------------------------------------------------------ the command through bin/hash10x-amd
EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
SUMMARY = re.compile(r"^  seq links at minShare (\d+), minBlocks (\d+), ends (\d+), maxEnds (\d+): (\d+) sequences, (\d+) row entries, (\d+) blocks used, "
                     r"(\d+) blocks skipped, (\d+) pairs, (\d+) links, (\d+) sequences with links, max shared (\d+)$", re.M)
VERBOSE = re.compile(r"^SEQ_LINKS  (\S+) ([HT]) (\S+) ([HT]) shared (\d+)$", re.M)
ARGS = (1, 2, 100, 16)                                            # minShare, minBlocks, endLen, maxEnds


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """small.fqb and its test sequences as plain FASTA, gzipped FASTA and FASTQ (the joins written as Ns), with the model's result"""
    d = str(tmp_path_factory.mktemp("slcli"))
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
    yield d, h, slm.seq_links(m, coded, *ARGS), names, [len(s) for s in seqs], m.n_blocks
    h.close()


def _run(d, *args, stdin=None):
    p = subprocess.run([EXE] + [str(a) for a in args], cwd=d, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_cli(cli):
    d, h, (off, other, shared, info, roff), names, lens, n_blocks = cli
    base = ["-B", 20, "--readFQB", "x.fqb", "--hashDepthRange", 3, 14]
    rc, out, err = _run(d, *base, "--verbose", "--seqLinks", *ARGS, "s.fa", "x.sl")
    assert rc == 0, err
    rinfo, goff, gother, gshared, table, rnames = _hx().read_seq_links(os.path.join(d, "x.sl"))
    assert rinfo == {"version": 1, "nBlocks": n_blocks, "minShare": 1, "minBlocks": 2, "endLen": 100, "maxEnds": 16, "nSeq": len(names), "links": len(other),
                     "skippedBlocks": info["skippedBlocks"], "nameBytes": sum(len(n) + 1 for n in names)}
    _same((goff, gother, gshared), (off, other, shared), "cli")
    assert rnames == names and len(other) > 20 and info["skippedBlocks"] > 0
    expected = slm.sl_bytes(n_blocks, *ARGS, lens, roff, off, other, shared, info["skippedBlocks"], names)
    image = open(os.path.join(d, "x.sl"), "rb").read()
    assert image == expected
    ends = np.repeat(np.arange(2 * len(names)), np.diff(off.astype(np.int64)))
    with_links = len(set((ends >> 1).tolist()) | set((other >> 1).tolist()))
    s = SUMMARY.search(out)
    assert s and [int(v) for v in s.groups()] == list(ARGS) + [len(names), info["rowEntries"], info["blocksUsed"], info["skippedBlocks"], info["pairs"],
                                                            len(other), with_links, int(shared.max())]
    lines = VERBOSE.findall(out)
    assert lines == [(names[e >> 1], "HT"[e & 1], names[f >> 1], "HT"[f & 1], str(c)) for e, f, c in zip(ends.tolist(), other.tolist(), shared.tolist())]
    # gzip and FASTQ give the same file; without --verbose there are no SEQ_LINKS lines
    for src in ("s.fa.gz", "s.fq"):
        rc, out, err = _run(d, *base, "--seqLinks", *ARGS, src, "y.sl")
        assert rc == 0 and open(os.path.join(d, "y.sl"), "rb").read() == image and "SEQ_LINKS" not in out and SUMMARY.search(out), (src, err)
    assert not [n for n in os.listdir(d) if n.endswith(".part")]
    # the session call, in slabs of 400 bases: the same bytes
    h.set_option("seq_slab", 400)
    h.write_seq_links(*ARGS, os.path.join(d, "s.fa"), os.path.join(d, "z.sl"), out=os.path.join(d, "z.out"), verbose=True)
    h.set_option("seq_slab", 0)
    assert open(os.path.join(d, "z.sl"), "rb").read() == image and len(VERBOSE.findall(open(os.path.join(d, "z.out")).read())) == len(other)
    # --interactive takes it too
    rc, out, err = _run(d, "-B", 20, "--interactive", stdin=b"readFQB x.fqb\nhashDepthRange 3 14\nseqLinks 1 2 100 16 s.fa i.sl\nquit\n")
    assert rc == 0 and open(os.path.join(d, "i.sl"), "rb").read() == image


def test_cli_refusals(cli):
    d = cli[0]
    gone = lambda name: not os.path.exists(os.path.join(d, name)) and not os.path.exists(os.path.join(d, name + ".part"))
    base = ["-B", 20, "--readFQB", "x.fqb"]
    rng = ["--hashDepthRange", 3, 14]
    rc, out, err = _run(d, "--seqLinks", *ARGS, "s.fa", "none.sl")                   # no state
    assert rc == 0 and "!! you must set hashDepthRange before seqLinks\n" in out and gone("none.sl")
    rc, out, err = _run(d, *base, "--seqLinks", *ARGS, "s.fa", "early.sl")
    assert rc == 0 and "!! you must set hashDepthRange before seqLinks\n" in out and gone("early.sl")
    rc, out, err = _run(d, "-o", "soft.out", *base, *rng, "--seqLinks", 0, 2, 100, 8, "s.fa", "a0.sl", "--seqLinks", 1, 0, 100, 8, "s.fa", "a1.sl",
                        "--seqLinks", 1, 2, -1, 8, "s.fa", "a2.sl", "--seqLinks", 1, 2, 100, -1, "s.fa", "a3.sl",
                        "--cluster", 1, 0, "--clusterSplit", "--seqLinks", *ARGS, "s.fa", "late.sl")
    assert rc == 0, err
    text = open(os.path.join(d, "soft.out")).read()
    for msg in ("!! seqLinks minShare 0 must be >= 1\n", "!! seqLinks minBlocks 0 must be >= 1\n", "!! seqLinks endLen -1 must be >= 0\n",
                "!! seqLinks maxEnds -1 must be >= 0\n", "!! you must set hashDepthRange before seqLinks\n"):
        assert msg in err and msg in text, msg
    assert all(gone(n) for n in ("a0.sl", "a1.sl", "a2.sl", "a3.sl", "late.sl"))
    rc, out, err = _run(d, *base, *rng, "--seqLinks", *ARGS, "nosuch.fa", "a.sl")
    assert rc == 255 and "FATAL ERROR: " in err and "failed to open sequence file nosuch.fa\n" in err and gone("a.sl")
    rc, out, err = _run(d, *base, *rng, "--seqLinks", *ARGS, "s.fa", "nodir/b.sl")
    assert rc == 255 and "FATAL ERROR: failed to open output file nodir/b.sl\n" in err and not os.path.exists(os.path.join(d, "nodir"))
    rc, out, err = _run(d, "--gpus", 2, *base, *rng, "--seqLinks", *ARGS, "s.fa", "s.sl")
    assert rc == 255 and "FATAL ERROR: --seqLinks does not run on a sharded session (--gpus 2)" in err and gone("s.sl")
