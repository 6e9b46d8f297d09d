"""From a sequence to its blocks in plain Python, straight from the definition (include/h10x.h "from a sequence to its blocks").

Layer 1: the moshes of a sequence are MoshModel.moshes (the oracle's moshRCiterator, pinned to the reference by the existing tests) with the
state's k, w and seed; each is looked up by value in hashValue[1 ..] (what hashIndexFind(hash, FALSE) returns for a consistent table); Q(s) is
the distinct found indices with hashWithinRange set, ascending.
Layer 2: the barcode list of hash x holds block d once per ClusterHash record of x in d (tests/share_model.py), so count_q[d] is the number of
records of block d whose hash is in the list, a hash given twice counted twice. No block is left out."""
import numpy as np

import mosh_model as mm


class SeqBlocksModel:
    def __init__(self, hash_value, hash_depth, within, n_hash, hashes, k=21, w=31, seed=17):
        """hash_value / hash_depth / within [hashNumber]; n_hash[c] = records of block c (block 0: 0), hashes = the hash index of every
        record, blocks 1 .. back to back"""
        self.value = np.asarray(hash_value, dtype=np.uint64)
        self.depth = np.asarray(hash_depth, dtype=np.int64)[:len(self.value)]
        self.within = np.asarray(within, dtype=bool)
        self.hash_number = len(self.value)
        n_hash = np.asarray(n_hash, dtype=np.int64)
        hashes = np.asarray(hashes, dtype=np.int64)
        assert n_hash.sum() == len(hashes)
        self.n_blocks = len(n_hash)
        blk = np.repeat(np.arange(self.n_blocks), n_hash)
        order = np.argsort(hashes, kind="stable")              # the records of a hash in block order: its barcode list
        self._blk = blk[order]
        self._start = np.searchsorted(hashes[order], np.arange(self.hash_number + 1))
        self._index = {int(v): i for i, v in enumerate(self.value) if i}
        self._mosh = mm.MoshModel(20, k, w, seed)
        self.block_off = np.concatenate([[0], np.cumsum(n_hash)])
        self.hashes = hashes

    @classmethod
    def from_state(cls, h, k=21, w=31, seed=17):
        """from a loaded hash10x_amd.Hash10x with a depth range set"""
        z = h.sizes()
        v = np.zeros(z["hashNumber"], np.uint64); d = np.zeros(z["hashNumber"], np.uint32)
        h._chk_ctx(h._hip.h10x_export(h._ctx(), None, v.ctypes.data, d.ctypes.data, None, None))
        return cls(v, d, h.export_within(), h.export_blocks()["nHash"], h.export_clushash()["hash"], k, w, seed)

    @classmethod
    def from_hash_file(cls, hf, ranges, k=21, w=31, seed=17):
        """from an orc.HashFile and the --hashDepthRange pairs set on it (lo <= depth < hi, the ranges add up)"""
        depth = np.asarray(hf.hash_depth[:hf.hash_number], dtype=np.int64)
        within = np.zeros(hf.hash_number, dtype=bool)
        for lo, hi in ranges:
            within |= (depth >= lo) & (depth < hi)
        n_hash = np.asarray(hf.blocks["nHash"][:hf.blocks_max], dtype=np.int64).copy()
        n_hash[0] = 0
        return cls(hf.hash_value, depth, within, n_hash, hf.clushash["hash"], k, w, seed)

    # ---- layer 1
    def barcode_list(self, x):
        return self._blk[self._start[x]:self._start[x + 1]]

    def lookup(self, seq):
        """per mosh occurrence of the sequence: (hash value, index or 0)"""
        hs, _ = self._mosh.moshes(np.asarray(seq, dtype=np.uint8))
        return [(int(v), self._index.get(int(v), 0)) for v in hs]

    def query(self, seq):
        """(Q(s) uint32 ascending, (moshes, found, query, entries))"""
        occ = self.lookup(seq)
        found = [x for _, x in occ if x]
        q = np.array(sorted({x for x in found if self.within[x]}), dtype=np.uint32)
        return q, (len(occ), len(found), len(q), int(self.depth[q].sum()))

    def seq_hashes(self, seqs):
        """(offsets, hash, figures rows) as Hash10x.seq_hashes"""
        qs = [self.query(s) for s in seqs]
        return _csr([q for q, _ in qs]) + ([f for _, f in qs],)

    # ---- layer 2
    def counts(self, hashes):
        """count_q[0 .. nBlocks) of one list"""
        c = np.zeros(self.n_blocks, dtype=np.int64)
        for x in hashes:
            x = int(x)
            assert 1 <= x < self.hash_number
            c += np.bincount(self.barcode_list(x), minlength=self.n_blocks)
        return c

    def row(self, hashes, t=1):
        c = self.counts(hashes)
        d = np.nonzero(c >= t)[0]
        return d.astype(np.uint32), c[d].astype(np.uint32)

    def list_share(self, offsets, hashes, t):
        """(offsets, block, count) as Hash10x.list_share"""
        offsets = [int(o) for o in offsets]
        rows = [self.row(hashes[a:b], t) for a, b in zip(offsets, offsets[1:])]
        off, blk = _csr([r[0] for r in rows])
        return off, blk, _csr([r[1] for r in rows])[1]

    def seq_blocks(self, seqs, t):
        """(offsets, block, count, figures rows) as Hash10x.seq_blocks"""
        off, hsh, fig = self.seq_hashes(seqs)
        return self.list_share(off, hsh, t) + (fig,)

    def good_hashes(self, c):
        """the hash index of every good record of block c (none for a block of more than 65535 records: hash10x.c:748)"""
        rec = self.hashes[self.block_off[c]:self.block_off[c + 1]]
        return rec[self.within[rec]] if len(rec) <= 65535 else rec[:0]


def _csr(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return off, (np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32))


def revcomp(seq):
    return (3 - np.asarray(seq, dtype=np.uint8))[::-1].copy()


def figures_equal(got, exp):
    """a structured figures array of Hash10x against the model's list of tuples"""
    return [tuple(int(v) for v in r) for r in got.tolist()] == [tuple(r) for r in exp]


def sb_bytes(n_blocks, min_share, lens, off, blk, cnt, fig, names, version=1, magic=b"10XQ"):
    """the bytes of a --seqBlocks file (hash10x_amd.read_seq_blocks reads them) from a result of the model"""
    import struct
    blob = b"".join(n.encode() + b"\0" for n in names)
    name_off = np.zeros(len(names) + 1, dtype="<u8")
    name_off[1:] = np.cumsum([len(n.encode()) + 1 for n in names])
    table = np.zeros(len(lens), dtype=[("len", "<u8"), ("moshes", "<u4"), ("found", "<u4"), ("query", "<u4"), ("reserved", "<u4")])
    for i, (n, f) in enumerate(zip(lens, fig)):
        table[i] = (n, f[0], f[1], f[2], 0)
    pairs = np.stack([np.asarray(blk, dtype="<u4"), np.asarray(cnt, dtype="<u4")], axis=1) if len(blk) else np.zeros((0, 2), "<u4")
    head = magic + struct.pack("<IIIQQQ", version, n_blocks, min_share, len(lens), len(blk), len(blob))
    return head + pairs.tobytes() + table.tobytes() + np.asarray(off, dtype="<u8").tobytes() + name_off.tobytes() + blob
