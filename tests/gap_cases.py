"""Inputs that make the mosh scan take its second attempt (moshScanWith of csrc/stage_g.hip, rsAddBatch of csrc/stage_h.hip): the list of a
batch is sized by an estimate, min(k-mers, 2 * (k-mers / w) + 65536), and the batch is scanned again at the exact size when it lists more.
The reader turns N into code 0, which is A; A^k hashes to 0 and T^k to 0 by its reverse strand, and 0 is a mosh for every w: an assembly
gap or a homopolymer run of 100 kb lists every one of its k-mers. Shared by the GPU tests of the five entry points that scan."""
import numpy as np

FLANK, GAP = 20000, 100000
_CODES = bytes.maketrans(b"ACGTN", bytes([0, 1, 2, 3, 0]))


def scan_cap(lens, k, w):
    """the estimate for a batch of sequences of these lengths"""
    nK = sum(max(0, n - k + 1) for n in lens)
    return min(nK, 2 * (nK // w) + 65536)


def gap_seqs(fill, seed=1906):
    """(left flank, left + run + right, right flank) as letters; fill = "N", "A", "T", or None for the control: random sequence of the same length"""
    rs = np.random.RandomState(seed)
    L = np.array(list("ACGT"))
    left, right, mid = ("".join(L[rs.randint(0, 4, n)]) for n in (FLANK, FLANK, GAP))
    return left, left + (fill * GAP if fill else mid) + right, right


def to_codes(s):
    """letters to the reader's codes: N is 0, as A"""
    return np.frombuffer(s.encode().translate(_CODES), np.uint8)


def write_fa(path, seqs, names=None):
    with open(path, "w") as f:
        f.write("".join(">%s\n" % (names[i] if names else "s%d" % i) + "".join(s[j:j + 100] + "\n" for j in range(0, len(s), 100)) for i, s in enumerate(seqs)))
