"""The share graph of --shareGraph in NumPy, straight from its definition (include/h10x.h "the share graph"; codeExplore's countShare,
hash10x.c:1371-1382, for every block at once).

The barcode list of a hash x holds one entry per ClusterHash record of x, so block d occurs in it M[d, x] times, M[d, x] = the records
of x in block d. The good hashes of a block c are its records with hashWithinRange set, and none at all for a block of more than 65535
records (goodHashesBuild, hash10x.c:748): G[c, x] = M[c, x] there, else 0. Walking the lists of c's good hashes and counting the
entries d != c gives countShare_c[d] = sum over x of G[c, x] * M[d, x]: one matrix product, the diagonal left out."""
import numpy as np


class ShareModel:
    def __init__(self, n_hash, hashes, within):
        """n_hash[c] = records of block c (block 0 unused: 0), hashes = the hash index of every record, blocks 1 .. back to back,
        within[x] = hashWithinRange of hash index x"""
        n_hash = np.asarray(n_hash, dtype=np.int64)
        hashes = np.asarray(hashes, dtype=np.int64)
        within = np.asarray(within, dtype=bool)
        assert n_hash.sum() == len(hashes)
        self.n_blocks = len(n_hash)
        blk = np.repeat(np.arange(self.n_blocks), n_hash)
        keep = within[hashes]                                  # columns outside the ranges never count
        cols, col = np.unique(hashes[keep], return_inverse=True)
        m = np.zeros((self.n_blocks, max(len(cols), 1)), dtype=np.float64)   # counts far below 2^53: exact in float64
        np.add.at(m, (blk[keep], col), 1.0)
        g = m.copy()
        g[n_hash > 65535] = 0.0
        share = np.rint(g @ m.T).astype(np.int64)
        np.fill_diagonal(share, 0)
        self.share = share                                     # share[c, d] = countShare_c[d]
        self.list_entries = share.sum(axis=1)                  # per block: the entries d != c of its good hashes' lists

    @classmethod
    def from_state(cls, h):
        """from a loaded hash10x_amd.Hash10x with a depth range set"""
        return cls(h.export_blocks()["nHash"], h.export_clushash()["hash"], h.export_within())

    @classmethod
    def from_hash_file(cls, hf, ranges):
        """from an orc.HashFile and the --hashDepthRange pairs set on it (lo <= depth < hi, the ranges add up: hash10x.c:528-539)"""
        depth = np.asarray(hf.hash_depth[:hf.hash_number], dtype=np.int64)
        within = np.zeros(hf.hash_number, dtype=bool)
        for lo, hi in ranges:
            within |= (depth >= lo) & (depth < hi)
        n_hash = np.asarray(hf.blocks["nHash"][:hf.blocks_max], dtype=np.int64).copy()
        n_hash[0] = 0
        return cls(n_hash, hf.clushash["hash"], within)

    def row(self, c, t=1):
        """(block, count) of row c at threshold t, ascending in block"""
        d = np.nonzero(self.share[c] >= t)[0]
        return d.astype(np.uint32), self.share[c, d].astype(np.uint32)

    def graph(self, t, code_min=1, code_max=0):
        """(offsets, block, count) over blocks [code_min, code_max), code_max = 0: all"""
        code_max = code_max or self.n_blocks
        rows = [self.row(c, t) for c in range(code_min, max(code_min, code_max))]
        off = np.zeros(len(rows) + 1, dtype=np.uint64)
        if rows:
            off[1:] = np.cumsum([len(r[0]) for r in rows])
        cat = lambda k: np.concatenate([r[k] for r in rows]) if rows else np.zeros(0, np.uint32)
        return off, cat(0).astype(np.uint32), cat(1).astype(np.uint32)
