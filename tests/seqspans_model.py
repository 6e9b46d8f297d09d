"""Sequence spans in plain Python, straight from the definition (include/h10x.h "sequence spans"), on top of SeqBlocksModel.

Hits: every mosh occurrence of the sequence (the oracle's hash values and pos[]) whose hash the state holds within the depth range gives one hit
(d, position) per entry d of the hash's barcode list. Extents: per block the hits by position, cut where two neighbours lie more than G apart (G = 0:
never), kept at T hits, the row ascending by (block, first). Coverage: per boundary j W, j = 1 .. (L - 1) // W, the kept extents with
first < j W <= last."""
import struct

import numpy as np


class SeqSpansModel:
    def __init__(self, sb):
        self.sb = sb                                           # a seqblocks_model.SeqBlocksModel
        self.k = sb._mosh.k

    def occurrences(self, seq):
        """[(position, index or 0)] of the sequence's mosh occurrences, in the oracle's order"""
        seq = np.asarray(seq, dtype=np.uint8)
        hs, ps = self.sb._mosh.moshes(seq)
        occ = self.sb.lookup(seq)
        assert [v for v, _ in occ] == [int(v) for v in hs]
        return [(int(p), x) for p, (_, x) in zip(ps, occ)]

    def hits(self, seq):
        """({block: [positions, ascending]}, (moshes, found, inRange))"""
        occ = self.occurrences(seq)
        counting = [(p, x) for p, x in occ if x and self.sb.within[x]]
        per = {}
        for p, x in counting:
            for d in self.sb.barcode_list(x):
                per.setdefault(int(d), []).append(p)
        return {d: sorted(ps) for d, ps in per.items()}, (len(occ), sum(1 for _, x in occ if x), len(counting))

    def row(self, seq, t=1, g=0):
        """([(block, first, last, hits)] kept, ascending by (block, first); figures; extents before the threshold)"""
        per, fig = self.hits(seq)
        out, n_all = [], 0
        for d in sorted(per):
            ps = per[d]
            start = 0
            for j in range(1, len(ps) + 1):
                if j == len(ps) or (g > 0 and ps[j] - ps[j - 1] > g):
                    n_all += 1
                    if j - start >= t:
                        out.append((d, ps[start], ps[j - 1], j - start))
                    start = j
        return out, fig, n_all

    @staticmethod
    def cover(row, length, w):
        nb = (length - 1) // w if w >= 1 and length >= 1 else 0
        return [sum(1 for _, f, l, _ in row if f < j * w <= l) for j in range(1, nb + 1)]

    def seq_spans(self, seqs, t, g=0, w=0):
        """(offsets, block, first, last, hits, cover_offsets, cover) as Hash10x.seq_spans, then the figures [(len, moshes, found, inRange, extents)]
        and the info entries the model knows"""
        rows, figs, covers, n_all, n_hits = [], [], [], 0, 0
        for s in seqs:
            row, fig, a = self.row(s, t, g)
            rows.append(row); figs.append((len(s),) + fig + (len(row),)); covers.append(self.cover(row, len(s), w)); n_all += a
            n_hits += sum(len(p) for p in self.hits(s)[0].values())
        flat = [e for r in rows for e in r]
        off = np.zeros(len(seqs) + 1, dtype=np.uint64); coff = np.zeros(len(seqs) + 1, dtype=np.uint64)
        if seqs:
            off[1:] = np.cumsum([len(r) for r in rows]); coff[1:] = np.cumsum([len(c) for c in covers])
        cols = [np.array([e[i] for e in flat], dtype=np.uint32) for i in range(4)]
        spans = [e[2] - e[1] for e in flat]
        info = {"sequences": len(seqs), "bases": sum(len(s) for s in seqs), "moshes": sum(f[1] for f in figs), "found": sum(f[2] for f in figs),
                "inRange": sum(f[3] for f in figs), "hits": n_hits, "extentsAll": n_all, "extents": len(flat), "sumSpan": sum(spans),
                "boundaries": int(coff[-1]), "maxHits": max([e[3] for e in flat], default=0), "maxSpan": max(spans, default=0)}
        return (off,) + tuple(cols) + (coff, np.array([c for cv in covers for c in cv], dtype=np.uint32)), figs, info


def mirrored(row, length, k):
    """the row of the reverse complement by property 3: first' = L - k - last, last' = L - k - first, again ascending by (block, first)"""
    return sorted((d, length - k - l, length - k - f, n) for d, f, l, n in row)


def weak_runs(cover, w, min_cover):
    """[(first position, last position, lowest cover)] of the maximal runs of boundaries below min_cover"""
    out, j = [], 0
    while j < len(cover):
        if cover[j] >= min_cover:
            j += 1
            continue
        e = j
        while e + 1 < len(cover) and cover[e + 1] < min_cover:
            e += 1
        out.append(((j + 1) * w, (e + 1) * w, min(cover[j:e + 1])))
        j = e + 1
    return out


def mean_span(total, extents):
    """the summary line's mean as C prints it"""
    return "%.1f" % (total / extents) if extents else "-nan"


def ss_bytes(n_blocks, t, g, w, min_cover, result, figs, names, version=1, magic=b"10XE", weak=None):
    """the bytes of a --seqSpans file (hash10x_amd.read_seq_spans reads them) from a result of the model"""
    off, blk, first, last, hits, coff, cover = result
    blob = b"".join(n.encode() + b"\0" for n in names)
    name_off = np.zeros(len(names) + 1, dtype="<u8")
    name_off[1:] = np.cumsum([len(n.encode()) + 1 for n in names])
    table = np.zeros(len(figs), dtype=[("len", "<u8"), ("moshes", "<u4"), ("found", "<u4"), ("inRange", "<u4"), ("weak", "<u4")])
    for i, f in enumerate(figs):
        c = cover[int(coff[i]):int(coff[i + 1])]
        table[i] = (f[0], f[1], f[2], f[3], int((c < min_cover).sum()) if weak is None else weak[i])
    quad = np.stack([np.asarray(c, dtype="<u4") for c in (blk, first, last, hits)], axis=1) if len(blk) else np.zeros((0, 4), "<u4")
    head = magic + struct.pack("<IIIIIIIQQQQ", version, n_blocks, t, g, w, min_cover, 0, len(figs), len(blk), len(cover), len(blob))
    return (head + quad.tobytes() + table.tobytes() + np.asarray(off, dtype="<u8").tobytes() + np.asarray(coff, dtype="<u8").tobytes() +
            np.asarray(cover, dtype="<u4").tobytes() + name_off.tobytes() + blob)
