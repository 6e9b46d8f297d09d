"""A numpy model of the barcode census and the whitelist correction of .fqb records (csrc/stage_j.hip), vectorised, and the inputs
the tests of that step share. The rule (fq2b.c:71-104): a record's candidates are its barcode word and the 48 one-substitution
neighbours that are in the whitelist; none: dropped; otherwise the candidate from the latest whitelist line wins and replaces
word 0. A barcode is record word 0 as fq2b packs it: first base in the top two bits."""
import gzip
import os
import subprocess

import numpy as np

import orc

FQ2B_REF = os.path.join(orc.REF_DIR, "fq2b")
GOLDEN = os.path.join(orc.GOLDEN, "fixfqb")
_SYM = np.zeros(256, dtype=np.uint32)
for _i, _ch in enumerate("ACGT"):
    _SYM[ord(_ch)] = _SYM[ord(_ch.lower())] = _i


def pack(words):
    """16-letter words -> packed barcodes (anything but ACGTacgt packs as A)"""
    out = np.zeros(len(words), dtype=np.uint32)
    for i, w in enumerate(words):
        assert len(w) == 16
        v = 0
        for ch in w:
            v = (v << 2) | int(_SYM[ord(ch)])
        out[i] = v
    return out


def text(codes):
    """packed barcodes -> the goodcodes text: one 16-letter line each"""
    return "".join("".join("ACGT"[(int(c) >> (2 * (15 - b))) & 3] for b in range(16)) + "\n" for c in codes)


def census(records, thresh):
    """(codes, counts, good): the distinct barcode words ascending, their counts, and those with count >= thresh"""
    r = np.asarray(records, dtype=np.uint32).reshape(-1, 30)
    codes, counts = np.unique(r[:, 0], return_counts=True)
    return codes.astype(np.uint32), counts.astype(np.uint32), codes[counts >= thresh].astype(np.uint32)


def latest_lines(whitelist):
    """(codes ascending, line): the last line (1-based) each distinct whitelist barcode stands on"""
    w = np.asarray(whitelist, dtype=np.uint32).reshape(-1)
    line = np.arange(1, w.size + 1, dtype=np.int64)
    order = np.lexsort((line, w))
    ws, ls = w[order], line[order]
    last = np.ones(ws.size, dtype=bool)
    last[:-1] = ws[1:] != ws[:-1]
    return ws[last], ls[last]


def candidates(x):
    """(n, 49): x, then for base b = 0..15 from the first base the three other letters there (column 1 + 3 b + (m - 1), m = 1..3)"""
    x = np.asarray(x, dtype=np.uint32).reshape(-1, 1)
    mask = np.zeros(49, dtype=np.uint32)
    for b in range(16):
        for m in (1, 2, 3):
            mask[1 + 3 * b + (m - 1)] = m << (2 * (15 - b))
    return x ^ mask[None, :]


def fix(records, whitelist):
    """(records_out, stats): stats = {"dropped", "corrected", "correctedAt": [16]}"""
    r = np.asarray(records, dtype=np.uint32).reshape(-1, 30)
    codes, lines = latest_lines(whitelist)
    if r.shape[0] == 0:
        return r.copy(), {"dropped": 0, "corrected": 0, "correctedAt": [0] * 16}
    cand = candidates(r[:, 0])
    if codes.size:
        at = np.minimum(np.searchsorted(codes, cand), codes.size - 1)
        ln = np.where(codes[at] == cand, lines[at], 0)
    else:
        ln = np.zeros(cand.shape, dtype=np.int64)
    best = np.argmax(ln, axis=1)                     # distinct barcodes stand on distinct lines: no ties above 0
    rows = np.arange(r.shape[0])
    keep = ln[rows, best] > 0
    fixed = keep & (best > 0)
    out = r[keep].copy()
    out[:, 0] = cand[rows, best][keep]
    at_base = np.bincount((best[fixed] - 1) // 3, minlength=16)
    return out, {"dropped": int((~keep).sum()), "corrected": int(fixed.sum()), "correctedAt": [int(v) for v in at_base]}


def _pct(num, den):
    return "-nan" if den == 0 else "%.1f" % (100.0 * num / den)     # 100.0 * 0 / 0.0 in C on x86-64: the default NaN, printed "-nan"


def stats_lines(written, stats):
    """the four lines fq2b prints after a -10x run (fq2b.c:164, 170-176), as bytes"""
    s = "written %d read pairs 151 + 151 bp packed in 30 word records\n" % written
    s += "%d (%s%%) not matching barcodes were dropped\n" % (stats["dropped"], _pct(stats["dropped"], stats["dropped"] + written))
    s += "%d (%s%%) of those that matched were error corrected\n" % (stats["corrected"], _pct(stats["corrected"], written))
    s += "by base position:" + "".join(" %d" % v for v in stats["correctedAt"]) + "\n"
    return s.encode()


# ------------------------------------------------------------------------------------------ inputs
def _sub(b, pos, c):
    return b[:pos] + c + b[pos + 1:]


def _other(ch, step=1):
    return "ACGT"[("ACGT".index(ch) + step) % 4]


def write_fastq_pairs(d, n, seed, n_codes=60):
    """n read pairs as r1.fq.gz / r2.fq.gz in d: barcodes drawn from a skewed pool that holds pairs one substitution apart,
    a share of reads with one substituted base, with an N in the barcode, and with a random barcode"""
    rng = np.random.default_rng(seed)
    pool = ["".join(rng.choice(list("ACGT"), 16)) for _ in range(n_codes)]
    for i in range(0, 12, 2):                                                        # pairs of frequent barcodes one substitution apart
        p = int(rng.integers(16))
        pool[i + 1] = _sub(pool[i], p, _other(pool[i][p], 1 + int(rng.integers(3))))
    weight = 1.0 / np.arange(1, n_codes + 1) ** 0.7
    weight /= weight.sum()
    with gzip.open(os.path.join(d, "r1.fq.gz"), "wt", compresslevel=6) as f1, gzip.open(os.path.join(d, "r2.fq.gz"), "wt", compresslevel=6) as f2:
        for i in range(n):
            bc = list(pool[rng.choice(n_codes, p=weight)])
            u = rng.random()
            if u < 0.25:
                bc[rng.integers(16)] = "ACGT"[rng.integers(4)]
            elif u < 0.32:
                bc = list(rng.choice(list("ACGT"), 16))
            elif u < 0.40:
                bc[rng.integers(16)] = "N"
            elif u < 0.44:
                p, q = rng.choice(16, 2, replace=False)
                bc[p], bc[q] = _other(bc[p]), _other(bc[q], 2)
            s1 = "".join(bc) + "".join(rng.choice(list("ACGTN"), 135, p=[.24, .24, .24, .24, .04]))
            s2 = "".join(rng.choice(list("acgtACGTN"), 151))
            q1 = "".join(chr(int(c)) for c in rng.integers(35, 75, 151))
            q2 = "".join(chr(int(c)) for c in rng.integers(35, 75, 151))
            f1.write("@read%d 1:N:0\n%s\n+\n%s\n" % (i, s1, q1))
            f2.write("@read%d 1:N:0\n%s\n+\n%s\n" % (i, s2, q2))


def run_fq2b_ref(d, out, whitelist=None):
    """the reference's fq2b on r1.fq.gz / r2.fq.gz of d -> (bytes of out, stderr)"""
    opts = ["-10x", whitelist] if whitelist else []
    r = subprocess.run([FQ2B_REF] + opts + ["-o", out, "r1.fq.gz", "r2.fq.gz"], cwd=d, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    return open(os.path.join(d, out), "rb").read(), r.stderr


FRESH_T = (1, 2, 20)


def fresh_case(d):
    """The 4000-pair input of the tests, made once per directory: raw.fqb from the reference's fq2b without a whitelist, and for
    T in FRESH_T the model's goodcodes (good<T>.txt, ascending) with the reference's `fq2b -10x` output and stderr.
    Returns {"raw": bytes, T: {"good": path, "bytes": .., "stderr": ..}}."""
    write_fastq_pairs(d, 4000, 11)
    raw, _ = run_fq2b_ref(d, "raw.fqb")
    case = {"raw": raw}
    recs = np.frombuffer(raw, dtype=np.uint32).reshape(-1, 30)
    for T in FRESH_T:
        good = census(recs, T)[2]
        assert good.size > 0
        name = "good%d.txt" % T
        with open(os.path.join(d, name), "w") as f:
            f.write(text(good))
        b, err = run_fq2b_ref(d, "ref%d.fqb" % T, name)
        case[T] = {"good": name, "codes": good, "bytes": b, "stderr": err}
    return case


def shadow_whitelist(rng):
    """A whitelist in no particular order (the construction of test_fq2b_matches_reference_bytes_and_stats): neighbours one and two
    substitutions apart, listed before AND after the barcode they shadow, and a repeated line"""
    wl = ["".join(rng.choice(list("ACGT"), 16)) for _ in range(40)]
    wl += [_sub(wl[3], 5, _other(wl[3][5])), _sub(_sub(wl[4], 2, _other(wl[4][2])), 9, _other(wl[4][9])), wl[6]]
    return [_sub(wl[8], 15, _other(wl[8][15]))] + wl


def write_fastq_for_whitelist(d, wl, n, seed):
    rng = np.random.default_rng(seed)
    with gzip.open(os.path.join(d, "r1.fq.gz"), "wt") as f1, gzip.open(os.path.join(d, "r2.fq.gz"), "wt") as f2:
        for i in range(n):
            bc = list(wl[rng.integers(len(wl))])
            u = rng.random()
            if u < 0.3:
                bc[rng.integers(16)] = "ACGT"[rng.integers(4)]
            elif u < 0.4:
                bc = list(rng.choice(list("ACGT"), 16))
            elif u < 0.45:
                bc[rng.integers(16)] = "N"
            s1 = "".join(bc) + "".join(rng.choice(list("ACGTN"), 135, p=[.24, .24, .24, .24, .04]))
            s2 = "".join(rng.choice(list("acgtACGTN"), 151))
            q1 = "".join(chr(int(c)) for c in rng.integers(35, 75, 151))
            q2 = "".join(chr(int(c)) for c in rng.integers(35, 75, 151))
            f1.write("@read%d 1:N:0\n%s\n+\n%s\n" % (i, s1, q1))
            f2.write("@read%d 1:N:0\n%s\n+\n%s\n" % (i, s2, q2))


def synthetic_records(n, n_codes, seed):
    """(records, good): n records built as arrays over about n_codes distinct good barcodes — 0x00000000 and 0xFFFFFFFF among them,
    pairs of good codes one substitution apart, records with two or more good neighbours, and a share two substitutions away"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 32, n_codes - 2 - n_codes // 4, dtype=np.uint64).astype(np.uint32)
    near = base[: n_codes // 4] ^ (rng.integers(1, 4, n_codes // 4).astype(np.uint32) << (2 * rng.integers(0, 16, n_codes // 4)).astype(np.uint32))
    good = np.unique(np.concatenate([base, near, np.array([0, 0xFFFFFFFF], dtype=np.uint32)]))
    pick = good[rng.integers(0, good.size, n)]
    pick[:50] = 0
    pick[50:100] = 0xFFFFFFFF
    u = rng.random(n)
    one = (rng.integers(1, 4, n).astype(np.uint32) << (2 * rng.integers(0, 16, n)).astype(np.uint32))
    p = rng.integers(0, 16, n)
    q = (p + 1 + rng.integers(0, 15, n)) % 16
    two = (rng.integers(1, 4, n).astype(np.uint32) << (2 * p).astype(np.uint32)) | (rng.integers(1, 4, n).astype(np.uint32) << (2 * q).astype(np.uint32))
    w0 = np.where(u < 0.35, pick ^ one, np.where(u < 0.50, pick ^ two, pick)).astype(np.uint32)
    recs = rng.integers(0, 1 << 32, (n, 30), dtype=np.uint64).astype(np.uint32)
    recs[:, 0] = w0
    return recs, good
