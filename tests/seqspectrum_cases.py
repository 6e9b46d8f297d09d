"""The scripted state for --seqSpectrum, shared by test_seq_spectrum_cpu.py and test_seq_spectrum_gpu.py: built as seqspans_cases.Script builds its
own (random sequences, the oracle's moshes as hashValue[], a script of which block holds which hash how often), so that every edge of the
definition lies where its case says. A hash's depth is the number of records that hold it. k = 21, w = 31, seed 17, B = 20."""
import numpy as np

import orc
import seqblocks_model as sbm
import seqspans_cases as ssc
import seqspans_model as ssm
import seqspectrum_model as spm

K, W, R = ssc.K, ssc.W, ssc.R
C1, C2, CM = 3, 6, 10                                          # the thresholds the depths of "cls" stand around
RANGE = (C1, CM)                                               # the range of the cross-check with seq_spans (property 8): thresholds (lo, lo, hi)
CLS_DEPTHS = (C1 - 1, C1, C2 - 1, C2, CM - 1, CM, 1022, 1023, 1024)
WIN = 1500                                                     # "main" has 2 W + 1 bases, "even" 2 W, "short" W - 1

(B_A, B_B, B_BIN0, B_BIN1, B_BIN2, B_REP, B_MAIN, B_LONG, B_HEAVY) = range(1, 10)

_built = []


def script():
    """the one scripted state: (Script, image bytes, SeqSpectrumModel)"""
    if _built:
        return _built[0]
    z = ssc.Script()
    cls = z.add("cls", ssc.random_seq(2000, 41))
    assert len(cls) > len(CLS_DEPTHS) + 3 and len({v for _, v in cls}) == len(cls)
    for i, d in enumerate(CLS_DEPTHS[:6]):                     # occurrence i has depth CLS_DEPTHS[i]: two blocks share the records
        z.hold(B_A, "cls", (i,), times=d // 2); z.hold(B_B, "cls", (i,), times=d - d // 2)
    for b, i in ((B_BIN0, 6), (B_BIN1, 7), (B_BIN2, 8)):       # depths 1022, 1023, 1024: the last two exact bins and the clipped one
        z.hold(b, "cls", (i,), times=CLS_DEPTHS[i])
    # occurrences 9 .. of "cls" are in no block: absent
    seg = ssc.random_seq(400, 43)
    rep = z.add("rep7", np.concatenate([seg] * 7))             # a segment seven times in one sequence ..
    values = [v for _, v in rep]
    seven = [i for i, v in enumerate(values) if values.count(v) == 7]
    assert seven
    z.rep = seven[0]
    z.hold(B_REP, "rep7", (z.rep,), times=4)
    main = z.add("main", ssc.with_unit_gap(2 * WIN + 1, 100))
    d = np.diff([p for p, _ in main]).tolist()
    z.unit = d.index(1)                                        # occurrences unit and unit + 1 start one base apart
    z.hold(B_MAIN, "main", range(0, len(main), 2), times=CM)
    z.add("even", ssc.random_seq(2 * WIN, 47)); z.add("short", ssc.random_seq(WIN - 1, 53))
    z.add("k-1", ssc.random_seq(K - 1, 2)); z.add("empty", ssc.random_seq(0, 1))
    assert not z.occ["empty"] and not z.occ["k-1"]
    once = z.add("rep8", seg.copy())                           # .. an eighth time in a sequence that another slab can hold ..
    assert rep[z.rep][1] in [v for _, v in once]
    w1 = z.add("w1", ssc.random_seq(100, 59))
    assert w1
    z.hold(B_LONG, "w1", (0,), times=C2)
    s65 = z.add("s65", ssc.random_seq(2400, 61)); s257 = z.add("s257", ssc.random_seq(9000, 67))
    assert 65 <= len(s65) < 257 <= len(s257)                   # one window of at least 65 and one of at least 257 occurrences (W above 9000; a mosh per 32 bases at this w)
    z.hold(B_LONG, "s65", range(0, len(s65), 3), times=C1); z.hold(B_LONG, "s257", range(1, len(s257), 2), times=C2 - 1)
    z.add("rep9", seg.copy())                                  # .. and a ninth
    z.hold(B_HEAVY, "main", (1,))
    data, values = z.image()
    hf = orc.HashFile(data)
    sb = sbm.SeqBlocksModel.from_hash_file(hf, [RANGE], K, W, R)
    _built.append((z, data, spm.SeqSpectrumModel(ssm.SeqSpansModel(sb))))
    return _built[0]


def sequences(z, names=None):
    return [z.seqs[n] for n in (names or z.names)]


def threshold_sets():
    """the main thresholds; class 1 empty; class 2 empty; all M; all above the deepest hash: all class 0"""
    return [(C1, C2, CM), (C1, C1, CM), (C1, CM, CM), (0, 0, 0), (5000, 5000, 5000)]


def windows(z):
    """every window a case runs at over all sequences: none; L = 2 W + 1, 2 W, W - 1, L < k; a boundary between the two moshes one base apart;
    one window per sequence (65 and 257 occurrences in one segment); W > every L"""
    return [0, WIN, z.pos("main", z.unit + 1), 10000, 10 ** 6]


def params(z):
    return [(C1, C2, CM, w) for w in windows(z)] + [t + (WIN,) for t in threshold_sets()[1:]]
