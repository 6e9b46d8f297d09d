"""Row links and sequence links in plain numpy / Python, straight from the definition (include/h10x.h "row links").

Ends: sequence s gives end 2s, its first min(len, endLen) bases, and end 2s + 1, its last min(len, endLen) bases; endLen 0 makes end 2s the
whole sequence and end 2s + 1 empty. Each end is a sequence of its own and its row is SeqBlocksModel's --seqBlocks row at minShare.
Row links: ends(d) = the lists that hold block d; d is used when maxLists == 0 or ends(d) <= maxLists; shared(e, f) = the used blocks in both
lists; with siblings lists 2s and 2s + 1 are never linked; the row of list e is {(f, shared) : f > e, shared >= minBlocks} ascending in f."""
import struct

import numpy as np


def cut_ends(seqs, end_len):
    """[head of s0, tail of s0, head of s1, ...] as code arrays"""
    out = []
    for s in seqs:
        s = np.asarray(s, dtype=np.uint8)
        if end_len:
            m = min(len(s), end_len)
            out += [s[:m].copy(), s[len(s) - m:].copy()]
        else:
            out += [s.copy(), s[:0].copy()]
    return out


def _csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows])
    return off


def row_links(offsets, block, min_blocks, max_lists=0, siblings=False):
    """(offsets uint64[n + 1], other uint32[], shared uint32[], info) as Hash10x.row_links and its row_links_info (the figures that do not
    depend on the batching: lists, rowEntries, blocksUsed, skippedBlocks, pairs, links, maxShared)"""
    assert min_blocks >= 1
    offsets = np.asarray(offsets, dtype=np.int64)
    block = np.asarray(block, dtype=np.int64)[:int(offsets[-1])]
    n = len(offsets) - 1
    lst = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    for a, b in zip(offsets[:-1], offsets[1:]):
        assert np.all(np.diff(block[a:b]) > 0), "a list must ascend strictly"
    order = np.lexsort((lst, block))                           # by block, then by list: a block's run is the ascending list of its ends
    sb, sl = block[order], lst[order]
    starts = np.flatnonzero(np.r_[True, sb[1:] != sb[:-1]]) if len(sb) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(sb)] if len(sb) else starts
    used = skipped = 0
    es, fs = [], []
    for a, b in zip(starts, ends):
        k = b - a
        if max_lists and k > max_lists:
            skipped += 1
            continue
        used += 1
        i, j = np.triu_indices(k, 1)
        es.append(sl[a + i]); fs.append(sl[a + j])
    e = np.concatenate(es) if es else np.zeros(0, np.int64)
    f = np.concatenate(fs) if fs else np.zeros(0, np.int64)
    key, cnt = np.unique(e * max(n, 1) + f, return_counts=True)
    ke, kf = key // max(n, 1), key % max(n, 1)
    keep = cnt >= min_blocks
    if siblings:
        keep &= (ke >> 1) != (kf >> 1)
    ke, kf, cnt = ke[keep], kf[keep], cnt[keep]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(ke, minlength=n)[:n]) if n else 0
    info = {"lists": n, "rowEntries": len(block), "blocksUsed": used, "skippedBlocks": skipped, "pairs": len(e), "links": len(kf),
            "maxShared": int(cnt.max()) if len(cnt) else 0}
    return off, kf.astype(np.uint32), cnt.astype(np.uint32), info


def brute_force(lists, min_blocks, max_lists=0, siblings=False):
    """the same from all-pairs set intersections: {(e, f): shared}"""
    count = {}
    for q in lists:
        for d in q:
            count[d] = count.get(d, 0) + 1
    sets = [{d for d in q if not max_lists or count[d] <= max_lists} for q in lists]
    out = {}
    for e in range(len(lists)):
        for f in range(e + 1, len(lists)):
            if siblings and e >> 1 == f >> 1:
                continue
            c = len(sets[e] & sets[f])
            if c >= min_blocks:
                out[(e, f)] = c
    return out


def as_dict(off, other, shared):
    off = np.asarray(off, dtype=np.int64)
    return {(e, int(other[i])): int(shared[i]) for e in range(len(off) - 1) for i in range(off[e], off[e + 1])}


def end_rows(m, seqs, min_share, end_len):
    """the --seqBlocks rows of the 2 n ends through a seqblocks_model.SeqBlocksModel: (offsets, block)"""
    off, blk, _, _ = m.seq_blocks(cut_ends(seqs, end_len), min_share)
    return off, blk


def seq_links(m, seqs, min_share, min_blocks, end_len, max_ends=0):
    """(offsets, other, shared, info, row offsets of the ends) as Hash10x.seq_links"""
    roff, rblk = end_rows(m, seqs, min_share, end_len)
    return row_links(roff, rblk, min_blocks, max_ends, True) + (roff,)


def sl_bytes(n_blocks, min_share, min_blocks, end_len, max_ends, lens, row_off, off, other, shared, skipped, names, version=1, magic=b"10XL"):
    """the bytes of a --seqLinks file (hash10x_amd.read_seq_links reads them); row_off = the row offsets of the 2 n ends"""
    blob = b"".join(n.encode() + b"\0" for n in names)
    name_off = np.zeros(len(names) + 1, dtype="<u8")
    name_off[1:] = np.cumsum([len(n.encode()) + 1 for n in names])
    rows = np.diff(np.asarray(row_off, dtype=np.int64))
    table = np.zeros(len(lens), dtype=[("len", "<u8"), ("headRows", "<u4"), ("tailRows", "<u4")])
    for i, n in enumerate(lens):
        table[i] = (n, rows[2 * i], rows[2 * i + 1])
    pairs = np.stack([np.asarray(other, dtype="<u4"), np.asarray(shared, dtype="<u4")], axis=1) if len(other) else np.zeros((0, 2), "<u4")
    head = magic + struct.pack("<IIIIIIIQQQQ", version, n_blocks, min_share, min_blocks, end_len, max_ends, 0, len(lens), len(other), skipped, len(blob))
    return head + table.tobytes() + np.asarray(off, dtype="<u8").tobytes() + pairs.tobytes() + name_off.tobytes() + blob
