"""The linkage groups of --shareComponents in plain Python, straight from their definition (include/h10x.h "the components of the share
graph"): the share graph of tests/share_model.py at a threshold T, every row entry (c, d) — share[c, d] >= T — an undirected edge {c, d},
a union-find over the blocks, and the five arrays:

  root[c]    the smallest block number in c's connected component (root[0] = 0)
  comp[c]    the components of blocks 1 .. numbered 1 .. nComponents in ascending order of their root (comp[0] = 0)
  rootOf[k], blocks[k], records[k]   per component its root, its member count and the sum of nHash of its members (entry 0 all zero)"""
import numpy as np


def components(share, n_hash, t):
    """share[c, d] = countShare_c[d] (a square integer matrix, block 0 unused), n_hash[c] = records of block c, t = minShare >= 1:
    (comp uint32[n], root uint32[n], rootOf uint32[k + 1], blocks uint32[k + 1], records uint64[k + 1])"""
    share = np.asarray(share)
    n = share.shape[0]
    assert share.shape == (n, n) and len(n_hash) == n and t >= 1
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for c, d in zip(*np.nonzero(share >= t)):                  # either direction joins: a block with an empty row stands in others'
        a, b = find(int(c)), find(int(d))
        if a != b:
            parent[max(a, b)] = min(a, b)                      # the smaller number stays the root
    root = np.array([find(c) for c in range(n)], dtype=np.uint32)
    assert n == 0 or root[0] == 0, "block 0 holds no records and stands in no list"
    roots = sorted(set(int(r) for r in root[1:]))
    number = {r: k for k, r in enumerate(roots, start=1)}
    comp = np.zeros(n, dtype=np.uint32)
    root_of = np.zeros(len(roots) + 1, dtype=np.uint32)
    blocks = np.zeros(len(roots) + 1, dtype=np.uint32)
    records = np.zeros(len(roots) + 1, dtype=np.uint64)
    for c in range(1, n):
        k = number[int(root[c])]
        comp[c] = k
        blocks[k] += 1
        records[k] += np.uint64(int(n_hash[c]))
    for r, k in number.items():
        root_of[k] = r
    return comp, root, root_of, blocks, records


def figures(result):
    """(components, largest member count, singletons, components of at least 3 blocks)"""
    blocks = result[3]
    return len(blocks) - 1, int(blocks.max()) if len(blocks) > 1 else 0, int((blocks[1:] == 1).sum()), int((blocks[1:] >= 3).sum())


class CompModel:
    """the components of a share_model.ShareModel"""

    def __init__(self, model, n_hash):
        self.model = model
        self.n_hash = np.asarray(n_hash, dtype=np.int64)
        self.n_blocks = model.n_blocks

    @classmethod
    def from_state(cls, h):
        import share_model
        return cls(share_model.ShareModel.from_state(h), h.export_blocks()["nHash"])

    def rows(self, t):
        return int((self.model.share >= t).sum())

    def components(self, t):
        return components(self.model.share, self.n_hash, t)
