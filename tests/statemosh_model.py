"""The definition of --writeMosh (include/h10x.h "the state as a mosh set") in plain Python: the in-range hashes of a state as a classed
mosh set. Insertion and serialisation are mosh_model.MoshModel's (_find_add, to_bytes): the table is the one sequential moshsetIndexFind
insertion in set-index order builds."""
import numpy as np

import mosh_model

U16MAX = 65535


def classes(depth, c1, c2, cM, table=None):
    """per hash index (base class, final class): moshutils.c:173-177 over the saturated depth, then the --hashCopies record
    (distinct, groups, largest, second): second >= 2 -> 3, otherwise largest < 2 -> 0, otherwise the base class"""
    d = np.minimum(np.asarray(depth, dtype=np.int64), U16MAX)
    base = np.where(d < c1, 0, np.where(d < c2, 1, np.where(d < cM, 2, 3))).astype(np.uint8)
    final = base.copy()
    if table is not None:
        table = np.asarray(table)
        assert table.shape == (len(d), 4)
        largest, second = table[:, 2].astype(np.int64), table[:, 3].astype(np.int64)
        final[(second < 2) & (largest < 2)] = 0
        final[second >= 2] = 3
    return base, final


def state_mosh(value, depth, within, c1, c2, cM, bits, k, w, seed, table=None, min_share=0, crib_type=None):
    """(MoshModel, info): info as Hash10x.mosh_set_info"""
    value = np.asarray(value, dtype=np.uint64)
    depth = np.asarray(depth, dtype=np.int64)
    keep = np.asarray(within).astype(bool).copy()
    assert len(value) == len(depth) == len(keep)
    keep[0] = False
    base, final = classes(depth, c1, c2, cM, table)
    xs = np.flatnonzero(keep)
    if len(xs) + 1 >= (1 << bits) >> 2:
        raise mosh_model.ModelDie("Moshset size %d is too big for %d bits" % (len(xs) + 1, bits))
    m = mosh_model.MoshModel(bits, k, w, seed)
    m.size = len(xs) + 1                                       # full, as a set read from a file
    for n, x in enumerate(xs, start=1):                        # ascending x: the k-th kept hash gets set index k
        i = m._find_add(int(value[x]))
        assert i == n, "the state's hash values are distinct"
        m.depth[i] = int(min(depth[x], U16MAX))
        m.info[i] = int(final[x])
    crib = np.zeros((5, 4), dtype=np.int64)
    if crib_type is not None:
        t = np.asarray(crib_type).astype(np.int64)
        t[t > 4] = 0
        np.add.at(crib, (t[xs], final[xs].astype(np.int64)), 1)
    info = {"kept": len(xs), "copy": np.bincount(final[xs], minlength=4).tolist(),
            "toM": int(((final[xs] == 3) & (base[xs] != 3)).sum()) if table is not None else 0,
            "to0": int(((final[xs] == 0) & (base[xs] != 0)).sum()) if table is not None else 0,
            "saturated": int((depth[xs] > U16MAX).sum()), "crib": crib.tolist(), "hashNumber": len(value), "bits": bits,
            "minShare": min_share if table is not None else 0}
    return m, info
