"""The per-hash linkage groups of --hashCopies in plain Python, straight from their definition (include/h10x.h "the per-hash linkage
groups"): per in-range hash x >= 1 the distinct blocks D(x) from the records, the share matrix of tests/share_model.py at a threshold T
restricted to them — a and b joined when share[a, b] >= T or share[b, a] >= T — and a union-find:

  distinct = |D(x)|, groups = the connected components, largest / second = the member counts of the two largest (second = 0 with one group)

Hashes outside the range, and index 0, hold four zeros."""
import numpy as np

import share_model


def groups_of(adj, blocks):
    """(groups, largest, second) of the graph adj (a boolean matrix, symmetric) restricted to the block numbers `blocks`"""
    blocks = [int(b) for b in blocks]
    parent = list(range(len(blocks)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, a in enumerate(blocks):
        for j in range(i + 1, len(blocks)):
            if adj[a, blocks[j]]:
                ra, rb = find(i), find(j)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    sizes = {}
    for i in range(len(blocks)):
        r = find(i)
        sizes[r] = sizes.get(r, 0) + 1
    top = sorted(sizes.values(), reverse=True)
    return len(top), top[0], top[1] if len(top) > 1 else 0


class CopiesModel:
    def __init__(self, n_hash, hashes, within):
        """n_hash[c] = records of block c (block 0 unused: 0), hashes = the hash index of every record, blocks 1 .. back to back,
        within[x] = hashWithinRange of hash index x"""
        n_hash = np.asarray(n_hash, dtype=np.int64)
        hashes = np.asarray(hashes, dtype=np.int64)
        self.within = np.asarray(within, dtype=bool)
        self.hash_number = len(self.within)
        self.model = share_model.ShareModel(n_hash, hashes, self.within)
        blk = np.repeat(np.arange(len(n_hash)), n_hash)
        keep = self.within[hashes] & (hashes >= 1)
        order = np.lexsort((blk[keep], hashes[keep]))             # the barcode lists: by hash, ascending block, repeats kept
        hs, bs = hashes[keep][order], blk[keep][order]
        cut = np.flatnonzero(np.diff(hs)) + 1
        self.xs = hs[np.concatenate([[0], cut])] if len(hs) else np.zeros(0, np.int64)
        self.lists = np.split(bs, cut) if len(hs) else []
        self.deepest = max((len(l) for l in self.lists), default=0)
        # an in-range hash without a record cannot be (its depth is its record count), so xs are all the in-range hashes
        assert len(self.xs) == int(self.within[1:].sum())

    @classmethod
    def from_state(cls, h):
        """from a loaded hash10x_amd.Hash10x with a depth range set"""
        return cls(h.export_blocks()["nHash"], h.export_clushash()["hash"], h.export_within())

    @classmethod
    def from_hash_file(cls, hf, ranges):
        """from an orc.HashFile and the --hashDepthRange pairs set on it"""
        depth = np.asarray(hf.hash_depth[:hf.hash_number], dtype=np.int64)
        within = np.zeros(hf.hash_number, dtype=bool)
        for lo, hi in ranges:
            within |= (depth >= lo) & (depth < hi)
        n_hash = np.asarray(hf.blocks["nHash"][:hf.blocks_max], dtype=np.int64).copy()
        n_hash[0] = 0
        return cls(n_hash, hf.clushash["hash"], within)

    def rows(self, t):
        return int((self.model.share >= t).sum())

    def table(self, t):
        """the (hashNumber, 4) uint16 array at threshold t. Hashes with the same distinct blocks have the same answer: computed once"""
        assert t >= 1
        adj = self.model.share >= t
        adj = adj | adj.T
        out = np.zeros((self.hash_number, 4), dtype=np.uint16)
        seen = {}
        for x, lst in zip(self.xs, self.lists):
            d = np.unique(lst)
            key = d.tobytes()
            if key not in seen:
                seen[key] = (len(d),) + groups_of(adj, d)
            out[x] = seen[key]
        return out

    def tallies(self, table):
        """(inRange, oneGroup, split, deepest) of a table"""
        t = table[self.xs] if len(self.xs) else np.zeros((0, 4), np.uint16)
        return len(self.xs), int((t[:, 1] == 1).sum()), int((t[:, 3] >= 2).sum()), self.deepest
