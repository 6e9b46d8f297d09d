"""The sequence spectrum in plain Python, straight from the definition (include/h10x.h "sequence spectrum"), on top of
SeqSpansModel.occurrences and the state's hashDepth[].

An occurrence (position, index) is absent (index 0) or of class 0, 1, 2, M by d = hashDepth[index] against copy1min, copy2min, copyMmin. Per
sequence and per window (position // W) the counts and the sum of d; copies[x] over all sequences of the run; S[min(d, 1023)][min(copies, 7)] and
total / present per class over the hashes x >= 1."""
import struct

import numpy as np

DEPTH_BINS, COPY_BINS = 1024, 8
FIELDS = ("moshes", "absent", "n0", "n1", "n2", "nM", "depthSum")
WINDOW = np.dtype([(k, "<u4") for k in FIELDS[:6]] + [("depthSum", "<u8")])
FIGURES = np.dtype([("len", "<u8")] + [(k, "<u4") for k in FIELDS[:6]] + [("depthSum", "<u8")])


def klass(d, c1, c2, cm):
    return 0 if d < c1 else 1 if d < c2 else 2 if d < cm else 3


class SeqSpectrumModel:
    def __init__(self, ss):
        self.ss = ss                                           # a seqspans_model.SeqSpansModel
        self.depth = ss.sb.depth
        self.hash_number = ss.sb.hash_number
        self.k = ss.k
        self._occ = {}

    def occurrences(self, seq):
        """[(position, index or 0)] of the sequence's mosh occurrences (kept per sequence: the model is asked often)"""
        key = np.asarray(seq, dtype=np.uint8).tobytes()
        if key not in self._occ:
            self._occ[key] = self.ss.occurrences(seq)
        return self._occ[key]

    def record(self, occ, c1, c2, cm):
        """(moshes, absent, n0, n1, n2, nM, depthSum) of a list of occurrences"""
        r = [len(occ), 0, 0, 0, 0, 0, 0]
        for _, x in occ:
            if not x:
                r[1] += 1
            else:
                d = int(self.depth[x])
                r[2 + klass(d, c1, c2, cm)] += 1
                r[6] += d
        return tuple(r)

    def windows(self, seq, c1, c2, cm, w):
        if w < 1:
            return []
        occ = self.occurrences(seq)
        return [self.record([o for o in occ if o[0] // w == j], c1, c2, cm) for j in range(-(-len(seq) // w))]

    def copies(self, seqs):
        c = np.zeros(self.hash_number, dtype=np.uint32)
        for s in seqs:
            for _, x in self.occurrences(s):
                if x:
                    c[x] += 1
        return c

    def spectrum(self, copies, c1, c2, cm):
        s = np.zeros((DEPTH_BINS, COPY_BINS), dtype=np.uint64)
        totals = np.zeros((2, 4), dtype=np.uint64)
        d = self.depth[1:self.hash_number].astype(np.int64)
        cp = copies[1:self.hash_number].astype(np.int64)
        np.add.at(s, (np.minimum(d, DEPTH_BINS - 1), np.minimum(cp, COPY_BINS - 1)), 1)
        q = (d >= c1).astype(np.int64) + (d >= c2) + (d >= cm)
        totals[0] = np.bincount(q, minlength=4)
        totals[1] = np.bincount(q[cp >= 1], minlength=4)
        return s, totals

    def seq_spectrum(self, seqs, c1, c2, cm, w=0):
        """((figures, win_offsets, windows, spectrum, totals) as Hash10x.seq_spectrum, copies, info)"""
        figs = np.zeros(len(seqs), dtype=FIGURES)
        wins, off = [], np.zeros(len(seqs) + 1, dtype=np.uint64)
        for i, s in enumerate(seqs):
            figs[i] = (len(s),) + self.record(self.occurrences(s), c1, c2, cm)
            wins += self.windows(s, c1, c2, cm, w)
            off[i + 1] = len(wins)
        win = np.array(wins, dtype=WINDOW) if wins else np.zeros(0, dtype=WINDOW)
        copies = self.copies(seqs)
        s, totals = self.spectrum(copies, c1, c2, cm)
        info = {"sequences": len(seqs), "bases": sum(len(x) for x in seqs), "windows": len(wins), "hashNumber": self.hash_number,
                "maxCopies": int(copies.max()) if len(copies) else 0}
        for k in FIELDS:
            info[k] = int(figs[k].astype(np.uint64).sum())
        return (figs, off, win, s, totals), copies, info


def qv(moshes, unsupported, k):
    if not moshes:
        return 0.0
    if not unsupported:
        return float("inf")
    return -10.0 * float(np.log10(1.0 - (1.0 - unsupported / moshes) ** (1.0 / k))) + 0.0


def completeness(totals):
    have, every = int(totals[1, 1:].sum()), int(totals[0, 1:].sum())
    return 100.0 * have / every if every else 0.0


def sp_bytes(hash_number, c1, c2, cm, w, result, copies, names, version=1, magic=b"10XP", bins=(DEPTH_BINS, COPY_BINS), zero=0):
    """the bytes of a --seqSpectrum file (hash10x_amd.read_seq_spectrum reads them) from a result of the model"""
    figs, off, win, s, totals = result
    blob = b"".join(n.encode() + b"\0" for n in names)
    name_off = np.zeros(len(names) + 1, dtype="<u8")
    name_off[1:] = np.cumsum([len(n.encode()) + 1 for n in names])
    head = magic + struct.pack("<IIIIIIIIIQQQ", version, hash_number, c1, c2, cm, w, bins[0], bins[1], zero, len(figs), len(win), len(blob))
    held = np.minimum(np.asarray(copies, dtype=np.uint32), 255).astype(np.uint8)
    return (head + np.asarray(win, dtype=WINDOW).tobytes() + np.asarray(figs, dtype=FIGURES).tobytes() + np.asarray(off, dtype="<u8").tobytes() +
            np.asarray(totals, dtype="<u8").tobytes() + np.asarray(s, dtype="<u8").tobytes() + held.tobytes() + name_off.tobytes() + blob)
