"""The molecule map and the split order of --moleculeMap / --splitFQB in numpy, over an orc.HashFile.

TEST INFRASTRUCTURE: expected values always come from a .hash the reference binary wrote (the goldens, or orc.run_ref),
never from the code under test.

  nCodes = arrayMax(clusterBlocks), slot 0 unused; base[c] = records of blocks 1 .. c-1; R = base[nCodes];
  subBefore[c] = sub-clusters of the blocks before c; M = all sub-clusters.
  Record base[c] + r is read pair r of block c. A ClusterHash record of block c counts as clustered with label cl = subCluster when
  1 <= subCluster <= nSubCluster[c] (and its read lies inside the block). A read's label is that of its FIRST clustered record in
  block order, its slot the number of clustered reads of the block with the same label whose first clustered record lies earlier
  (the reference's ++new2[clus].nRead order, hash10x.c:979-989), its molecule nCodes - 1 + subBefore[c] + label: the block number
  --clusterSplit gives the cluster. An unclustered read keeps mol = c, slot = r.
  Split order: the records of post-split block m lie at start[m] .. start[m + 1]: those of a molecule in slot order, those left in
  a parent block in file order.
"""
import numpy as np

import orc


class MolModel:
    def __init__(self, hf):
        n_codes = int(hf.blocks_max)
        blocks = hf.blocks[:n_codes]
        n_read = blocks["nRead"].astype(np.int64).copy()
        n_sub = blocks["nSubCluster"].astype(np.int64).copy()
        if n_codes:
            n_read[0] = 0                                    # slot 0 is nobody's block
        base = np.zeros(n_codes + 1, dtype=np.int64)
        base[1:] = np.cumsum(n_read)
        sub_before = np.zeros(n_codes + 1, dtype=np.int64)
        sub_before[1:] = np.cumsum(n_sub)
        R, M = int(base[n_codes]), int(sub_before[n_codes])
        mol = np.repeat(np.arange(n_codes, dtype=np.int64), n_read)
        slot = np.arange(R, dtype=np.int64) - base[mol]
        rank = slot.copy()                                   # position inside the post-split block
        count = np.zeros(n_codes + M, dtype=np.int64)
        count[:n_codes] = n_read
        for c in np.flatnonzero(n_sub[1:] > 0) + 1:
            ch = hf.block_clushash(int(c))
            sub = ch["subCluster"].astype(np.int64)
            read = ch["read"].astype(np.int64)
            cl = np.where((sub >= 1) & (sub <= n_sub[c]) & (read < n_read[c]), sub, 0)
            pos = np.flatnonzero(cl > 0)
            reads, idx = np.unique(read[pos], return_index=True)      # idx: the first clustered record of each clustered read
            first = pos[idx]
            order = np.argsort(first, kind="stable")
            reads, label = reads[order], cl[first[order]]
            ext = n_codes - 1 + int(sub_before[c])
            seen = np.zeros(256, dtype=np.int64)
            for r, l in zip(reads.tolist(), label.tolist()):
                mol[base[c] + r] = ext + l
                slot[base[c] + r] = rank[base[c] + r] = seen[l]
                seen[l] += 1
            count[ext + 1: ext + 1 + int(n_sub[c])] = seen[1: 1 + int(n_sub[c])]
            mine = slice(int(base[c]), int(base[c + 1]))
            uncl = mol[mine] == c
            rank[mine] = np.where(uncl, np.cumsum(uncl) - uncl, rank[mine])
            count[c] = int(uncl.sum())
        self.n_codes, self.R, self.M = n_codes, R, M
        self.base, self.sub_before = base, sub_before
        self.mol, self.slot = mol.astype(np.uint32), slot.astype(np.uint32)
        self.count = count
        self.start = np.zeros(n_codes + M + 1, dtype=np.uint64)
        self.start[1:] = np.cumsum(count)
        assert int(self.start[-1]) == R
        self.dest = self.start[mol].astype(np.int64) + rank
        assert np.array_equal(np.sort(self.dest), np.arange(R))
        self.n_clustered = int((mol >= n_codes).sum())
        self.info = {"nRecords": R, "nClustered": self.n_clustered, "nBlocks": n_codes, "nMolecules": M}

    def split(self, records):
        """the first R records in split order"""
        r = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 30)[:self.R]
        out = np.empty_like(r)
        out[self.dest] = r
        return out

    def mol_bytes(self):
        """the .mol file: 32-byte header, then R pairs {u32 mol, u32 slot} in file order"""
        head = (b"10XM" + (1).to_bytes(4, "little") + self.R.to_bytes(8, "little") + self.n_codes.to_bytes(4, "little")
                + self.M.to_bytes(4, "little") + self.n_clustered.to_bytes(8, "little"))
        assert len(head) == 32
        return head + np.stack([self.mol, self.slot], axis=1).astype("<u4").tobytes()

    def idx_bytes(self):
        """the .idx file beside a split .fqb"""
        return (b"10XS" + (1).to_bytes(4, "little") + self.n_codes.to_bytes(4, "little") + self.M.to_bytes(4, "little")
                + self.start.astype("<u8").tobytes())

    def check_against_split(self, split_hf):
        """the tie to the reference's state after --clusterSplit: block m >= nCodes holds start[m + 1] - start[m] reads and its
        parent is the barcode its records came from; a ClusterHash (hash, read r) of block m is record start[m] + r of the split
        file, so r stays below the block's record count"""
        assert int(split_hf.blocks_max) == self.n_codes + self.M
        b = split_hf.blocks[:split_hf.blocks_max]
        assert np.array_equal(b["nRead"][self.n_codes:].astype(np.int64), self.count[self.n_codes:])
        parent = np.zeros(self.M, dtype=np.int64)
        for c in range(1, self.n_codes):
            parent[int(self.sub_before[c]): int(self.sub_before[c + 1])] = c + 1                  # 1 + the parent's number (hash10x.c:66, 976)
        assert np.array_equal(b["clusterParent"][self.n_codes:].astype(np.int64), parent)
        assert np.array_equal(b["nRead"][1:self.n_codes].astype(np.int64), np.diff(self.base)[1:])      # a parent keeps its nRead (hash10x.c:990)
        for m in range(self.n_codes, self.n_codes + self.M):
            ch = split_hf.block_clushash(m)
            if ch.size:
                assert int(ch["read"].max()) < self.count[m]
                assert np.unique(ch["read"]).size == self.count[m]      # every record of the molecule is referred to


def load(name):
    """model over a golden .hash"""
    import os
    return MolModel(orc.HashFile(orc.read_maybe_gz(os.path.join(orc.GOLDEN, name))))


def split_refs(model, split_hf, records_in_split_order, source_records):
    """every ClusterHash record of a new block points at a record that came from its parent's barcode and carries the molecule"""
    out = np.ascontiguousarray(records_in_split_order, dtype=np.uint32).reshape(-1, 30)
    src = np.ascontiguousarray(source_records, dtype=np.uint32).reshape(-1, 30)
    for m in range(model.n_codes, model.n_codes + model.M):
        parent = int(split_hf.blocks["clusterParent"][m]) - 1
        word0 = src[int(model.base[parent]), 0]
        ch = split_hf.block_clushash(m)
        at = int(model.start[m]) + ch["read"].astype(np.int64)
        assert (at < int(model.start[m + 1])).all()
        assert (out[at, 0] == word0).all()
