"""The test sequences of --seqBlocks on the golden sets, shared by test_seq_blocks_cpu.py and test_seq_blocks_gpu.py: second reads of chosen
records, decoded from the record words, and sequences joined from the reads of several blocks with a random tail."""
import os

import numpy as np

import orc
from gap_cases import scan_cap

K, W, R = 21, 31, 17                                           # the session's defaults: the hasher of every state in these tests
SMALL_RANGE = (3, 14)


def small_records():
    return np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32).reshape(-1, 30)


def tiny_records():
    return np.fromfile(os.path.join(orc.GOLDEN, "tiny.fqb"), dtype=np.uint32).reshape(-1, 30)


def read2(recs, r):
    """the 150 hashed bases of the second read of record r as codes 0 .. 3 (the state hashes bases 0 .. 149: tests/golden/make_golden.py)"""
    s = np.zeros(160, np.uint8)
    orc.lib().orc_unpack160(np.ascontiguousarray(recs[r, 15:25]).ctypes.data, s.ctypes.data)
    return s[:150].copy()


def block_of(recs):
    """block number of every record: the barcode runs from 1 (the last run is the file's unhashed trailing block)"""
    w0 = recs[:, 0]
    return np.cumsum(np.r_[True, w0[1:] != w0[:-1]])


def sequences(recs, step=97, joined=((0, 45), (1, 30)), tail=600, seed=5):
    """[(sequence, block of its read or 0)]: the second read of every step-th record outside the trailing block; per `joined` entry
    (first, n) the second reads of n records spread over the file from `first`, the first of them twice, joined with 5 Ns (code 0) and
    followed by `tail` random bases; then the edge lengths: empty, k - 1, k and one base short of the first window's end"""
    blk = block_of(recs)
    last = int(blk[-1])
    out = [(read2(recs, r), int(blk[r])) for r in range(0, len(recs), step) if blk[r] != last]
    rng = np.random.RandomState(seed)
    usable = np.flatnonzero(blk != last)
    for first, n in joined:
        pick = usable[first::max(len(usable) // n, 1)][:n]
        parts = []
        for r in [pick[0]] + list(pick):
            parts += [read2(recs, r), np.zeros(5, np.uint8)]
        parts.append(rng.randint(0, 4, tail).astype(np.uint8))
        out.append((np.concatenate(parts), 0))
    one = out[0][0]
    out += [(one[:0], 0), (one[:K - 1], 0), (one[:K], 0), (one[:K + W - 2], 0)]
    return out


def state_bytes(h, d):
    h.write_hash(os.path.join(d, "state.hash"))
    with open(os.path.join(d, "state.hash"), "rb") as f:
        return f.read()


def gapped_state(d):
    """(Hash10x, its model, contigs, left flank, right flank): the state of orc.poly_a_set (hash value 0 is in it and in range), and contigs cut from
    haplotype A: two flanks of 20 kb around a run of 100 kb (tests/gap_cases.py) or of 30 bases of code 0 (N or A) or 3 (T), or around 100 kb of
    random sequence (the control)"""
    import mosh_model as mm
    import seqblocks_model as sbm
    recs = orc.poly_a_set(os.path.join(d, "x.fqb"), fa=os.path.join(d, "x"))
    h = orc.hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(3, 60)
    ix, depth = orc.value0_depth(orc.HashFile(state_bytes(h, d)))
    assert ix >= 1 and 3 <= depth < 60
    hap = mm.parse_seq_bytes(open(os.path.join(d, "x.A.fa"), "rb").read())[0][0]
    left, right = hap[:20000], hap[25000:45000]
    contig = lambda mid: np.concatenate([left, mid, right]).astype(np.uint8)          # noqa: E731
    seqs = {"N": contig(np.zeros(100000, np.uint8)), "N30": contig(np.zeros(30, np.uint8)), "T": contig(np.full(100000, 3, np.uint8)),
            "T30": contig(np.full(30, 3, np.uint8)), "control": contig(np.random.RandomState(3).randint(0, 4, 100000))}
    assert scan_cap([len(seqs["N"])], K, W) == 74566 < 100000 - K
    return h, sbm.SeqBlocksModel.from_state(h), seqs, left, right
