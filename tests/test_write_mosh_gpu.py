"""--writeMosh on the GPU (csrc/stage_o.hip): Hash10x.mosh_set / write_mosh against the plain-Python model of the definition
(tests/statemosh_model.py), on golden states, the generated set and hand-made states; the reference's own moshutils reading the file;
moshutils-amd and moshasm-amd taking it; the refusals and the command line. Every comparison is exact equality."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import copies_model
import mosh_model as mm
import orc
import statemosh_model as sm

pytestmark = pytest.mark.gpu

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
MOSHUTILS = os.path.join(orc.REPO, "bin", "moshutils-amd")
MOSHASM = os.path.join(orc.REPO, "bin", "moshasm-amd")
REF_MOSHUTILS = os.path.join(orc.REF_DIR, "moshutils")
TOP = 2 ** 31 - 1
K, W, R = 21, 31, 17                                           # the session's defaults: the hasher of every state below
THR = (4, 7, 10)                                               # thresholds that leave hashes in every class on the states below
GTHR = (3, 4, 5)                                               # the same for the generated set, whose in-range lists have 2 .. 5 entries
ALL = (1, 1 << 30)                                             # a range that holds every hash

_hx, _molecules, _load_image, GEN = orc.hx, orc.molecules, orc.load_image, orc.GEN_MOLECULES


def _small_recs():
    return np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)


def _state(h):
    """(hashIndex, hashValue, hashDepth, within) of a loaded context"""
    z = h.sizes()
    ix = np.zeros(1 << z["B"], np.uint32); v = np.zeros(z["hashNumber"], np.uint64); d = np.zeros(z["hashNumber"], np.uint32)
    h._chk_ctx(h._hip.h10x_export(h._ctx(), ix.ctypes.data, v.ctypes.data, d.ctypes.data, None, None))
    return ix, v, d, h.export_within()


def _model(h, thr, bits=0, table=None, t=0, crib=None):
    _, v, d, within = _state(h)
    return sm.state_mosh(v, d, within, *thr, bits or h.sizes()["B"], K, W, R, table=table, min_share=t, crib_type=crib)


def _bytes(ms, tmp_path, name="set.mosh"):
    p = str(tmp_path / name)
    ms.write(p)
    with open(p, "rb") as f:
        return f.read()


def _same_bytes(got, exp, what):
    if mm.mask_mosh(got) != mm.mask_mosh(exp):
        a, b = mm.MoshModel.from_bytes(got), mm.MoshModel.from_bytes(exp)
        raise AssertionError((what, len(got), len(exp), a.max, b.max, [(i, x, y) for i, (x, y) in enumerate(zip(a.info, b.info)) if x != y][:8],
                              int((a.file_index != b.file_index).sum()) if a.B == b.B else "bits differ"))


def _check(h, tmp_path, thr, bits=0, table=None, t=0, crib=None, what=""):
    """mosh_set against the model: the file's bytes and the figures; returns (bytes, info)"""
    m, info = _model(h, thr, bits, table, t, crib)
    ms = h.mosh_set(*thr, bits=bits)
    got = _bytes(ms, tmp_path)
    assert ms.max == info["kept"] and ms.info().size == info["kept"] + 1          # full, as after h10x_mosh_load
    ms.close()
    _same_bytes(got, m.to_bytes(), what)
    assert h.mosh_set_info == info, (what, h.mosh_set_info, info)
    return got, info


# ------------------------------------------------------------------------------------ whole state, depth only, bits 0
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_whole_state_is_the_states_own_table(tmp_path, name):
    h = _hx().Hash10x(B=20)
    if name == "small":
        h.read_fqb(_small_recs())
    else:                                                      # a state the reference wrote, through --readHash
        p = tmp_path / "tiny.hash"
        p.write_bytes(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "tiny.hash.gz")))
        h.read_hash(str(p))
    h.depth_range(*ALL)
    ix, v, d, within = _state(h)
    assert within[1:].all() and len(v) == {"tiny": 74, "small": 5039}[name]
    ms = h.mosh_set(2, 5, 100)
    six, sv, sd, sf = ms.export()
    assert np.array_equal(six, ix) and np.array_equal(sv[1:], v[1:]) and sv[0] == 0
    assert np.array_equal(sd[1:], np.minimum(d[1:], 65535).astype(np.uint16)) and sd[0] == 0 and sf[0] == 0
    assert np.array_equal(sf[1:], np.where(d[1:] < 2, 0, np.where(d[1:] < 5, 1, np.where(d[1:] < 100, 2, 3))))
    i = ms.info()
    f1, f2 = mm.factors(R)
    assert (i.B, i.k, i.w, i.factor1, i.factor2, i.max, i.size) == (20, K, W, f1, f2, len(v) - 1, len(v))
    ms.close()
    _check(h, tmp_path, (2, 5, 100), what=name)
    h.close()


# ------------------------------------------------------------------------------------ the generated set: a narrowed range, depth only and by linkage
@pytest.fixture(scope="module")
def gen_recs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wm"))
    return d, orc.gen_fqb(os.path.join(d, "x.fqb"), *GEN, fa=os.path.join(d, "x"))


@pytest.fixture(scope="module")
def generated(gen_recs):
    d, recs = gen_recs
    h = _molecules(recs)                                       # -B 21, --cluster 1 0 --clusterSplit
    h.depth_range(2, 40)
    cm = copies_model.CopiesModel.from_state(h)
    yield h, cm, d
    h.close()


def test_narrow_range_against_model(generated, tmp_path):
    h, cm, _ = generated
    plain, info = _check(h, tmp_path, GTHR, what="depth only")
    assert info["kept"] == 3433 and info["minShare"] == 0 and all(info["copy"]) and info["hashNumber"] == cm.hash_number
    out = {}
    for t in (1, 50, TOP):
        table = cm.table(t)
        assert np.array_equal(h.hash_copies(t), table)
        out[t], info = _check(h, tmp_path, GTHR, table=table, t=t, what=("linkage", t))
        assert info["minShare"] == t and info["toM"] == 0      # the generated set has no split hash (test_hash_copies_cpu pins the tallies)
    assert out[1] == plain and h.mosh_set_info["to0"] == info["to0"]
    top = mm.MoshModel.from_bytes(out[TOP])
    assert not any(top.info) and info["copy"] == [3433, 0, 0, 0] and info["to0"] == 3433 - mm.MoshModel.from_bytes(plain).info[1:].count(0)
    assert out[50] != out[TOP]
    h.depth_range(2, 40)                                       # (leave the shared state without a kept result)


# ------------------------------------------------------------------------------------ hand-made states
def test_two_loci(tmp_path):
    """the state of test_hash_copies_gpu.test_two_loci: blocks 1-3 hold hashes 10, 11, 12, blocks 4-6 hold 20, 21, 22, all six hold hash 1
    (block 1 also hash 30, of depth 1, out of range). Thresholds (2, 5, 100): hash 1 (depth 6) is class 2 by depth, the others class 1."""
    blocks = [[1, 10, 11, 12, 30]] + [[1, 10, 11, 12]] * 2 + [[1, 20, 21, 22]] * 3
    h = _load_image(tmp_path, blocks)
    hashes = np.concatenate([np.asarray(b) for b in blocks])
    depth = np.bincount(hashes)
    cm = copies_model.CopiesModel([0] + [len(b) for b in blocks], hashes, (depth >= 2) & (depth < 100))
    xs = [1, 10, 11, 12, 20, 21, 22]

    def classes(table, t):
        got, info = _check(h, tmp_path, (2, 5, 100), table=table, t=t, what=("two loci", t))
        m = mm.MoshModel.from_bytes(got)
        assert m.value[1:] == [31 * x for x in xs] and m.depth[1:] == [6, 3, 3, 3, 3, 3, 3]     # set indices 1 .. 7 in that order
        return m.info[1:], (info["toM"], info["to0"], info["minShare"])

    assert classes(None, 0) == ([2, 1, 1, 1, 1, 1, 1], (0, 0, 0))
    for t, exp in ((1, ([2, 1, 1, 1, 1, 1, 1], (0, 0, 1))), (2, ([3, 1, 1, 1, 1, 1, 1], (1, 0, 2))), (5, ([0] * 7, (0, 7, 5)))):
        table = h.hash_copies(t)
        assert np.array_equal(table, cm.table(t))
        assert classes(table, t) == exp, t
    h.close()


def test_wave_edges(tmp_path):
    """300 hash indices, the kept ones no multiple of 64, index 1 and hashNumber - 1 among them and gaps in between: the ballots of the
    flag kernel and the ranks of the compact kernel at the edges of a wave and of the index range"""
    n = 300
    a = np.arange(1, n)
    b = np.array([x for x in a if x in (1, n - 1) or (x % 3 != 2 and x % 64 != 0)])
    h = _load_image(tmp_path, [a, b, b[::2]])                  # depths 1, 2 and 3
    _, v, d, within = _state(h)
    assert len(v) == n and within[1] and within[n - 1] and int(within[1:].sum()) == len(b) and len(b) % 64 != 0 and not within[2]
    got, info = _check(h, tmp_path, (2, 3, 100), what="wave edges")
    assert info["kept"] == len(b) and info["copy"] == [0, len(b) - len(b[::2]), len(b[::2]), 0]
    m = mm.MoshModel.from_bytes(got)
    assert m.value[1] == 31 and m.value[-1] == 31 * (n - 1)
    h.close()


def test_saturation(tmp_path):
    """one hash in 65536 records (depth only: the linkage refuses lists above 4096): depth 65535, classed by 65535, saturated = 1"""
    h = _load_image(tmp_path, [np.concatenate([np.full(65536, 1), [2, 2, 3]])], 2, 100000)
    _, v, d, within = _state(h)
    assert d[1] == 65536 and within[1] and within[2] and not within[3]
    got, info = _check(h, tmp_path, (2, 5, 65536), what="saturated, below M")
    m = mm.MoshModel.from_bytes(got)
    assert m.depth[1:] == [65535, 2] and m.info[1:] == [2, 1] and info["saturated"] == 1
    got, info = _check(h, tmp_path, (2, 5, 65535), what="saturated, M")
    assert mm.MoshModel.from_bytes(got).info[1:] == [3, 1] and info["saturated"] == 1 and info["copy"] == [0, 1, 0, 1]
    h.close()


# ------------------------------------------------------------------------------------ bits
def test_bits_below_the_states(tmp_path):
    h = _hx().Hash10x(B=24)
    h.read_fqb(_small_recs())
    h.depth_range(3, 14)
    got, info = _check(h, tmp_path, THR, bits=20, what="bits 20 of 24")
    assert info["bits"] == 20 and len(got) == 96 + 4 * (1 << 20) + 11 * (info["kept"] + 1)
    got0, info0 = _check(h, tmp_path, THR, what="bits 0 = 24")
    assert info0["bits"] == 24 and len(got0) == 96 + 4 * (1 << 24) + 11 * (info["kept"] + 1)
    err = _hx().Hash10xError
    for bad in (19, 35, -1, 1):
        with pytest.raises(err, match=r"!! writeMosh bits %d must be 0 or 20 \.\. 34" % bad):
            h.mosh_set(*THR, bits=bad)
    h.close()


def test_bits_too_small_for_the_kept_count(tmp_path):
    """moshsetCreate's capacity rule at its edge. A state of 20 table bits holds at most 2^18 hash indices; with every one of them kept
    the set has 2^18 entries, which 20 bits refuse (kept + 1 >= 2^18) and 21 take; with one hash fewer in range 20 bits take it."""
    n = (1 << 18) - 1                                           # hash indices 1 .. n
    a = np.arange(1, n + 1)
    h = _load_image(tmp_path, [a, a])
    err = _hx().Hash10xError
    with pytest.raises(err, match="Moshset size %d is too big for 20 bits" % (n + 1)):
        h.mosh_set(1, 2, 3)
    p = tmp_path / "big.mosh"
    with pytest.raises(err, match="Moshset size %d is too big for 20 bits" % (n + 1)):
        h.write_mosh(0, 1, 2, 3, str(p))
    assert not p.exists() and not (tmp_path / "big.mosh.part").exists()
    ms = h.mosh_set(1, 2, 3, bits=21)
    assert ms.max == n and h.mosh_set_info["kept"] == n and h.mosh_set_info["copy"] == [0, 0, n, 0] and h.mosh_set_info["bits"] == 21
    q = np.array([31, 31 * n, 31 * (n + 1), 62], dtype=np.uint64)
    ix, dp = ms.lookup(q)
    assert ix.tolist() == [1, n, 0, 2] and dp.tolist() == [2, 2, 0, 2]
    six, sv, sd, sf = ms.export()
    assert int((six != 0).sum()) == n and np.array_equal(sv[1:], 31 * a.astype(np.uint64)) and (sf[1:] == 2).all()
    ms.close()
    h.close()
    h = _load_image(tmp_path, [a, a[:-1]])                     # the last hash has depth 1: out of range
    ms = h.mosh_set(1, 2, 3)
    assert ms.max == n - 1 and h.mosh_set_info["bits"] == 20 and ms.lookup(q)[0].tolist() == [1, 0, 0, 2]
    ms.close()
    h.close()


# ------------------------------------------------------------------------------------ an empty result
def test_empty_result(tmp_path):
    h = _hx().Hash10x(B=20)
    h.read_fqb(_small_recs())
    h.depth_range(1000, 2000)
    got, info = _check(h, tmp_path, THR, what="empty")
    assert info["kept"] == 0 and info["copy"] == [0, 0, 0, 0] and len(got) == 8 + 4 + 4 + 80 + 4 * (1 << 20) + 8 + 2 + 1
    p = str(tmp_path / "empty.mosh")
    h.write_mosh(0, *THR, p)
    h.close()
    assert open(p, "rb").read() == got
    ms = _hx().MoshSet.read(p)
    assert ms.max == 0
    ms.close()
    r = subprocess.run([MOSHUTILS, "-r", p], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and b"number of entries 0" in r.stdout, r.stderr


# ------------------------------------------------------------------------------------ the kept --hashCopies result
def test_kept_result_stays(tmp_path):
    h = _hx().Hash10x(B=20)
    h.read_fqb(_small_recs())
    h.depth_range(3, 14)
    table = h.hash_copies(5)
    tally = h.hash_copies_tally()
    a, _ = _check(h, tmp_path, THR, table=table, t=5, what="first")
    b, _ = _check(h, tmp_path, THR, table=table, t=5, what="second")
    assert a == b and h.mosh_set_info["minShare"] == 5
    assert np.array_equal(h.hash_copies_tally(), tally)        # neither released nor changed
    out = np.zeros_like(table)
    assert h._hip.h10x_hash_copies_get(h._ctx(), out.ctypes.data, 0, len(out)) == 0 and np.array_equal(out, table)
    h.depth_range(3, 14)                                       # a new range releases the linkage
    c, info = _check(h, tmp_path, THR, what="after a new range")
    assert info["minShare"] == 0 and (info["toM"], info["to0"]) == (0, 0)
    h.close()


def test_refusals(gen_recs):
    err = _hx().Hash10xError
    h = _hx().Hash10x(B=21)
    with pytest.raises(err, match="!! you must set hashDepthRange before writeMosh"):
        h.mosh_set(*THR)
    h.read_fqb(gen_recs[1])
    with pytest.raises(err, match="!! you must set hashDepthRange before writeMosh"):
        h.mosh_set(*THR)
    h.depth_range(2, 40)
    for bad in ((-1, 2, 3), (3, 2, 5), (1, 5, 4)):
        with pytest.raises(err, match="!! writeMosh needs 0 <= copy1min <= copy2min <= copyMmin"):
            h.mosh_set(*bad)
    h.mosh_set(0, 0, 0).close()                                # equal thresholds ascend
    h.cluster(1, 0, 3)
    h.mosh_set(*THR).close()                                   # --cluster alone leaves the range in force
    h.cluster_split()
    with pytest.raises(err, match="!! you must set hashDepthRange before writeMosh"):
        h.mosh_set(*THR)
    h.depth_range(2, 40)
    h.mosh_set(*THR).close()
    # the C ABI without the seed of the hasher: refused, not a file with a second multiplier of 0
    set_ = ctypes.c_void_p()
    assert h._hip.h10x_set_option(h._ctx(), b"seqhash_seed", R + 1) == 0
    assert h._hip.h10x_mosh_from_state(h._ctx(), 0, *THR, ctypes.byref(set_), None) != 0 and not set_.value
    assert b"seqhash_seed" in h._hip.h10x_last_error(h._ctx())
    assert h._hip.h10x_set_option(h._ctx(), b"seqhash_seed", R) == 0
    assert h._hip.h10x_mosh_from_state(h._ctx(), 0, *THR, ctypes.byref(set_), None) == 0 and set_.value
    h._hip.h10x_mosh_destroy(set_)
    h.close()


# ------------------------------------------------------------------------------------ against the reference's moshutils
COPIES = re.compile(r"copy0 (\d+) copy1 (\d+) copy2 (\d+) copyM (\d+)")


def test_against_reference_moshutils(tmp_path):
    """W.mosh = the whole state with thresholds THR. The reference reads it and writes it back byte for byte; pruned by the reference to
    lo <= depth < hi it is our export of the state read anew with --hashDepthRange lo hi; its summary counts the classes as we do."""
    if not os.path.exists(REF_MOSHUTILS):
        pytest.fail("oracle/_ref/moshutils is missing: build() makes it from the reference's sources")
    d = str(tmp_path)
    lo, hi = 3, 9
    h = _hx().Hash10x(B=20)
    h.read_fqb(_small_recs())
    h.depth_range(*ALL)
    assert int(h.export_depth().max()) < 65535
    h.write_mosh(0, *THR, os.path.join(d, "W.mosh"))
    whole = h.mosh_set_info
    h.read_fqb(_small_recs())                                  # ranges add up: the narrower one needs the state anew
    h.depth_range(lo, hi)
    h.write_mosh(0, *THR, os.path.join(d, "ours.mosh"))
    narrow = h.mosh_set_info
    h.close()
    r = orc.run_ref(["-r", "W.mosh", "-w", "W2.mosh"], d, binary="moshutils")
    assert r.returncode == 0, r.stderr[-400:]
    w = open(os.path.join(d, "W.mosh"), "rb").read()
    assert mm.mask_mosh(open(os.path.join(d, "W2.mosh"), "rb").read()) == mm.mask_mosh(w)
    m = COPIES.search(r.stdout.decode())
    assert m and [int(v) for v in m.groups()] == whole["copy"] and all(whole["copy"][:3])
    r = orc.run_ref(["-r", "W.mosh", "-p", lo, hi, "-w", "P.mosh"], d, binary="moshutils")
    assert r.returncode == 0, r.stderr[-400:]
    _same_bytes(open(os.path.join(d, "ours.mosh"), "rb").read(), open(os.path.join(d, "P.mosh"), "rb").read(), "pruned by the reference")
    m = COPIES.findall(r.stdout.decode())
    assert [int(v) for v in m[-1]] == narrow["copy"] and 0 < narrow["kept"] < whole["kept"]


# ------------------------------------------------------------------------------------ the mosh tools take the file
def test_mosh_tools_take_the_file(tmp_path):
    """moshutils-amd merges a set made by -c with the session's (k, w, seed) and calls one of another seed incompatible; moshasm-amd -m
    prints the set's summary with our four copy counts. (-r gives a full set, as the reference's does: new hashes go into a created one.)"""
    d = str(tmp_path)
    h = _hx().Hash10x(B=20)
    h.read_fqb(_small_recs())
    h.depth_range(3, 14)
    h.write_mosh(0, *THR, os.path.join(d, "x.mosh"))
    info = h.mosh_set_info
    h.close()
    rs = np.random.RandomState(5)
    with open(os.path.join(d, "g.fa"), "w") as f:
        f.write(">g\n%s\n>short\nACGTACGT\n" % "".join(np.array(list("ACGT"))[rs.randint(0, 4, 3000)]))
    with open(os.path.join(d, "s.fa"), "w") as f:
        f.write(">short\nACGTACGT\n")

    def mu(*args):
        r = subprocess.run([MOSHUTILS] + [str(a) for a in args], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        return r.returncode, r.stdout.decode(), r.stderr.decode()

    for seed, fa, out in ((R, "g.fa", "y.mosh"), (R + 1, "g.fa", "z.mosh"), (R, "s.fa", "e.mosh")):
        assert mu("-c", 21, K, W, seed, "-a", fa, "-w", out)[0] == 0
    y = mm.MoshModel.from_bytes(open(os.path.join(d, "y.mosh"), "rb").read())
    x = mm.MoshModel.from_bytes(open(os.path.join(d, "x.mosh"), "rb").read())
    assert y.max > 50 and (y.k, y.w, y.factor1, y.factor2) == (x.k, x.w, x.factor1, x.factor2)
    rc, out, err = mu("-r", "x.mosh", "-m", "e.mosh")           # read as it is, merged with a compatible (empty) set
    assert rc == 0 and "incompatible" not in err and "number of entries %d" % info["kept"] in out
    assert "copy0 %d copy1 %d copy2 %d copyM %d" % tuple(info["copy"]) in out
    rc, out, err = mu("-c", 21, K, W, R, "-m", "x.mosh", "-m", "y.mosh", "-w", "u.mosh")
    assert rc == 0 and "incompatible" not in err
    u = mm.MoshModel.from_bytes(open(os.path.join(d, "u.mosh"), "rb").read())
    assert u.max == len(set(x.value[1:]) | set(y.value[1:])) and u.value[1:x.max + 1] == x.value[1:] and u.info[1:x.max + 1] == x.info[1:]
    rc, out, err = mu("-c", 21, K, W, R, "-m", "x.mosh", "-m", "z.mosh")
    assert rc == 0 and "moshset z.mosh incompatible with current - unable to merge" in err
    r = subprocess.run([MOSHASM, "-m", "x.mosh"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    assert ("MS table size %d number of entries %d" % (1 << 20, info["kept"])) in r.stdout.decode()
    assert "copy0 %d copy1 %d copy2 %d copyM %d" % tuple(info["copy"]) in r.stdout.decode()


# ------------------------------------------------------------------------------------ the command line
SUMMARY = re.compile(r"^  mosh set of (\d+) hashes in range, bits (\d+): copy0 (\d+) copy1 (\d+) copy2 (\d+) copyM (\d+)"
                     r"(?:, by depth only|, by linkage at minShare (\d+): (\d+) to M, (\d+) to 0)(?:, (\d+) depths cut to 65535)?$", re.M)
CRIB = re.compile(r"^WRITE_MOSH  (err|htA|htB|hom|mul) copy0 (\d+) copy1 (\d+) copy2 (\d+) copyM (\d+)$", re.M)


def _figures(m):
    return [int(v) if v is not None else None for v in m.groups()]


def test_cli(generated, tmp_path):
    h, cm, d = generated
    plain, i0 = _check(h, tmp_path, GTHR, what="depth only")
    table = h.hash_copies(50)
    linked, i50 = _check(h, tmp_path, GTHR, table=table, t=50, what="linkage")
    h.depth_range(2, 40)
    base = [EXE, "-B", "21", "-ct", "3", "--readFQB", "x.fqb"]
    mol = ["--hashDepthRange", 2, 40, "--cluster", 1, 0, "--clusterSplit", "--hashDepthRange", 2, 40]

    def run(*args):
        p = subprocess.run(base + [str(a) for a in args], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return p.returncode, p.stdout.decode(), p.stderr.decode()

    def data(name):
        with open(os.path.join(d, name), "rb") as f:
            return f.read()

    # depth only, then with a kept --hashCopies result, in one run
    rc, out, err = run(*mol, "--writeMosh", 0, *GTHR, "a.mosh", "--hashCopies", 50, "a.hc", "--writeMosh", 0, *GTHR, "b.mosh")
    assert rc == 0, err
    assert data("a.mosh") == plain and data("b.mosh") == linked and not os.path.exists(os.path.join(d, "a.mosh.part"))
    ms = list(SUMMARY.finditer(out))
    assert len(ms) == 2 and "WRITE_MOSH" not in out
    assert _figures(ms[0]) == [3433, 21] + i0["copy"] + [None, None, None, None]
    assert _figures(ms[1]) == [3433, 21] + i50["copy"] + [50, 0, i50["to0"], None]
    assert out[ms[1].end():].lstrip("\n").startswith("  user")  # the resource line follows
    # with -o the line goes to the file, behind the echo of the command's arguments
    rc, out, err = run("-o", "wm.out", *mol, "--writeMosh", 0, *GTHR, "c.mosh")
    assert rc == 0 and "mosh set of" not in out
    assert (" 0 %d %d %d c.mosh" % GTHR) + ms[0].group(0) + "\n" in open(os.path.join(d, "wm.out")).read()
    assert data("c.mosh") == plain
    # soft errors: the message, nothing written, exit status 0
    soft = [(["--writeMosh", 0, *GTHR, "early.mosh"], "!! you must set hashDepthRange before writeMosh\n", "early.mosh"),
            (["--hashDepthRange", 2, 40, "--writeMosh", 0, 5, 4, 9, "desc.mosh"], "!! writeMosh needs 0 <= copy1min <= copy2min <= copyMmin\n", "desc.mosh"),
            (["--hashDepthRange", 2, 40, "--writeMosh", 19, *GTHR, "b19.mosh"], "!! writeMosh bits 19 must be 0 or 20 .. 34\n", "b19.mosh"),
            (["--hashDepthRange", 2, 40, "--writeMosh", 35, *GTHR, "b35.mosh"], "!! writeMosh bits 35 must be 0 or 20 .. 34\n", "b35.mosh"),
            (["--hashDepthRange", 2, 40, "--cluster", 1, 0, "--clusterSplit", "--writeMosh", 0, *GTHR, "late.mosh"], "!! you must set hashDepthRange before writeMosh\n", "late.mosh")]
    for args, msg, name in soft:
        rc, out, err = run(*args)
        assert rc == 0 and msg in out, (args, out, err)
        assert not os.path.exists(os.path.join(d, name)) and not os.path.exists(os.path.join(d, name + ".part"))
    p = subprocess.run([EXE, "-B", "21", "--writeMosh", "0", "3", "4", "5", "nostate.mosh"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and b"!! you must set hashDepthRange before writeMosh\n" in p.stdout and not os.path.exists(os.path.join(d, "nostate.mosh"))
    # a path that cannot be opened, a sharded session
    rc, out, err = run("--hashDepthRange", 2, 40, "--writeMosh", 0, *GTHR, "nodir/x.mosh")
    assert rc == 255 and "FATAL ERROR: failed to open output file nodir/x.mosh" in err
    p = subprocess.run([EXE, "--gpus", "2", "-B", "21", "--readFQB", "x.fqb", "--hashDepthRange", "2", "40", "--writeMosh", "0", "3", "4", "5", "s.mosh"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 255 and "FATAL ERROR: --writeMosh does not run on a sharded session (--gpus 2)" in p.stderr.decode()
    assert not os.path.exists(os.path.join(d, "s.mosh"))
    # --interactive takes it too
    script = b"readFQB x.fqb\nhashDepthRange 2 40\ncluster 1 0\nclusterSplit\nhashDepthRange 2 40\nwriteMosh 0 3 4 5 i.mosh\nquit\n"
    p = subprocess.run(base[:5] + ["--interactive"], input=script, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and data("i.mosh") == plain


def test_cli_with_crib(gen_recs, tmp_path):
    """with --cribBuild the five WRITE_MOSH lines: crib type x class, from the model over the exported crib types"""
    d, recs = gen_recs
    h = _molecules(recs, crib=os.path.join(d, "x"))
    h.depth_range(2, 40)
    types = h.export_crib_type()
    table = h.hash_copies(50)
    got, info = _check(h, tmp_path, GTHR, table=table, t=50, crib=types, what="crib")
    exp = info["crib"]
    assert sum(map(sum, exp)) == info["kept"] and sum(1 for row in exp if any(row)) >= 2 and [sum(c) for c in zip(*exp)] == info["copy"]
    h.close()
    p = subprocess.run([EXE, "-B", "21", "-ct", "3", "--readFQB", "x.fqb", "--cribBuild", "x.A.fa", "x.B.fa", "--hashDepthRange", "2", "40", "--cluster", "1", "0",
                        "--clusterSplit", "--hashDepthRange", "2", "40", "--hashCopies", "50", "crib.hc", "--writeMosh", "0", "3", "4", "5", "crib.mosh"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode()
    lines = CRIB.findall(out)
    assert [l[0] for l in lines] == ["err", "htA", "htB", "hom", "mul"] and [[int(v) for v in l[1:]] for l in lines] == exp
    m = SUMMARY.search(out)
    assert m and _figures(m) == [info["kept"], 21] + info["copy"] + [50, info["toM"], info["to0"], None]
    assert open(os.path.join(d, "crib.mosh"), "rb").read() == got
