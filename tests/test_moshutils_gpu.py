"""moshutils-amd and hash10x_amd.MoshSet on the MI355X (csrc/stage_g.hip). Every comparison is exact equality. Expected
results come from (a) the golden fixtures the reference's moshutils produced (tests/golden/make_mosh_golden.py), (b) the
reference's own iterator, oracle/_ref/seqhash_test, run here on fresh input, and (c) the model of tests/mosh_model.py, which
tests/test_moshutils_cpu.py pins to (a) byte for byte."""
import os
import subprocess
import time

import numpy as np
import pytest

import mosh_model as mm
from gap_cases import GAP, gap_seqs, scan_cap, to_codes, write_fa
import orc

pytestmark = pytest.mark.gpu
EXE = os.path.join(orc.REPO, "bin", "moshutils-amd")
MAN = mm.manifest()


def run(args, cwd, timeout=600):
    if not os.path.exists(EXE):
        pytest.fail("bin/moshutils-amd is missing: run build()")
    return subprocess.run([EXE] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


# ---- (a) every golden case through the program -----------------------------------------------------------------------
@pytest.mark.parametrize("case", MAN["cases"], ids=[c["name"] for c in MAN["cases"]])
def test_program_matches_reference_golden(case, tmp_path):
    d = str(tmp_path)
    before = mm.stage_case(MAN, case, d)
    r = run(case["args"], d)
    mm.check_case(case, d, before, r.returncode, r.stdout, r.stderr)


# ---- (b) the reference's own iterator on fresh input -------------------------------------------------------------------
def _fresh_fasta(rs):
    """multi-line, lower case, dropped bytes, sequences shorter than k, one of several hundred kb; no N"""
    recs, lens = [], [400000, 15, 16, 17, 0, 3000, 50000, 1, 31, 32, 33, 47, 48, 12000]
    for i, n in enumerate(lens):
        s = np.array(list("ACGTacgt"))[rs.randint(0, 8, n)]
        s = list(s)
        for q in rs.choice(max(n, 1), min(n, n // 40), replace=False):
            s.insert(int(q), "RYKMSWBDHV-*. \r"[rs.randint(0, 15)])          # all dropped by the reader
        s = "".join(s)
        width = int(rs.randint(20, 120))
        recs.append(">s%d desc %d\n" % (i, n) + "".join(s[j:j + width] + "\n" for j in range(0, len(s), width)))
    return "".join(recs).encode()


def test_scan_and_add_match_reference_iterator(tmp_path):
    import hash10x_amd
    ref = os.path.join(orc.REF_DIR, "seqhash_test")
    if not os.path.exists(ref):
        pytest.fail("oracle/_ref/seqhash_test is missing: build() makes it where the reference is present")
    fa = _fresh_fasta(np.random.RandomState(20260))
    path = os.path.join(str(tmp_path), "fresh.fa")
    with open(path, "wb") as f:
        f.write(fa)
    r = subprocess.run([ref], input=fa, stdout=subprocess.PIPE, check=True)
    exp, lens, s = [], [], -1
    for line in r.stdout.decode().splitlines():
        if line.startswith("read sequence"):
            s += 1
            lens.append(int(line.split()[-1]))
        elif line.startswith("\t"):
            h, p, _ = line.split()
            exp.append((int(h, 16), s, int(p)))
    assert len(exp) > 10000
    codes, start, warn = hash10x_amd.read_sequences(path)
    assert warn == "" and [int(x) for x in np.diff(start.astype(np.int64))] == lens
    h, q, p = hash10x_amd.mosh_scan(codes, start, 16, 32, 1)
    assert list(zip(h.tolist(), q.tolist(), p.tolist())) == exp
    ms = hash10x_amd.MoshSet(B=20, k=16, w=32, seed=1)
    ms.set_option("mosh_slab", 30000)                         # many batches; the long sequence goes alone
    assert ms.add(codes, start) == len(exp)
    hs = np.array([e[0] for e in exp], np.uint64)
    u, first, cnt = np.unique(hs, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    _, v, dep, info = ms.export(index=False)
    assert v[1:].tolist() == u[order].tolist() and v[0] == 0
    assert dep[1:].tolist() == np.minimum(cnt[order], 65535).tolist()
    assert not info.any()
    ms.close()


# ---- (c) randomised chains against the model ---------------------------------------------------------------------------
def _chain_files(rs, d):
    B = np.array(list("ACGT"))
    g = ["".join(B[rs.randint(0, 4, n)]) for n in (30000, 18000, 40, 9000)]
    g.append(g[0][5000:12000])                                # repeats
    fa = "".join(">g%d\n" % i + "".join(s[j:j + 71] + "\n" for j in range(0, len(s), 71)) for i, s in enumerate(g))
    reads = []
    for i in range(1500):
        c = int(rs.randint(0, 2)); n = int(rs.randint(25, 200)); p = int(rs.randint(0, len(g[c]) - n))
        s = g[c][p:p + n]
        if rs.rand() < 0.3:
            s = s[:n // 2] + "N" + s[n // 2 + 1:]
        reads.append("@q%d\n%s\n+\n%s\n" % (i, s if i % 3 else s.lower(), "#" * n))
    other = ["".join(B[rs.randint(0, 4, 20000)]), g[1][2000:15000]]
    fb = "".join(">o%d\n%s\n" % (i, s) for i, s in enumerate(other))
    for name, text in (("a.fa", fa), ("x.fq", "".join(reads[:800])), ("b.fq", "".join(reads[800:])), ("c.fa", fb)):
        with open(os.path.join(d, name), "w") as f:
            f.write(text)


def _chain_cmds(B, k, w, seed):
    c = ["-c", B, k, w, seed]
    return [[str(x) for x in c + "-a a.fa -x x.fq -a b.fq -w s1.mosh -H s1.his -p 2 0 -s 2 3 6 -w s2.mosh".split()],
            [str(x) for x in c + "-a c.fa -a b.fq -s 1 2 3 -w t.mosh".split()],
            [str(x) for x in c + "-m s2.mosh -m t.mosh -sM 4 -w u.mosh -o u.txt -d u.dep s1.mosh t.mosh".split()],
            # negative numbers are plain int comparisons: -p -3 0 keeps all, -s -2 -1 3 knows only classes 2 and M, -sM -1 marks all, -p -5 -1 keeps none
            [str(x) for x in c + "-m s1.mosh -p -3 0 -s -2 -1 3 -w n1.mosh -sM -1 -w n2.mosh -p -5 -1 -w n3.mosh".split()]]


@pytest.mark.parametrize("seed,B,k,w", [(17, 20, 19, 31), (5, 20, 21, 7), (3, 24, 16, 32)])
def test_chain_matches_model(seed, B, k, w, tmp_path):
    import hash10x_amd
    dirs = {n: os.path.join(str(tmp_path), n) for n in ("model", "prog", "slab")}
    for n, d in dirs.items():
        os.makedirs(d)
        _chain_files(np.random.RandomState(1000 + seed), d)
    for cmd in _chain_cmds(B, k, w, seed):
        st, out, err = mm.run_commands(cmd, dirs["model"])
        assert st == 0, err
        for n, pre in (("prog", []), ("slab", ["--slab", "4000"])):       # a file spans many batches, the 30 kb sequence takes one alone
            r = run(pre + cmd, dirs[n])
            assert r.returncode == 0, r.stderr.decode()
            got = mm.mask_lines(r.stdout)
            if pre:
                got.remove("user")                               # the resource line of --slab itself
            assert got == mm.mask_lines(out.encode())
            assert [ln for ln in mm.mask_lines(r.stderr) if not ln.startswith("COMMAND --slab")] == mm.mask_lines(err.encode())
    for name in ("s1.mosh", "s2.mosh", "t.mosh", "u.mosh", "n1.mosh", "n2.mosh", "n3.mosh", "s1.his", "u.dep", "u.txt"):
        files = {}
        for n, d in dirs.items():
            with open(os.path.join(d, name), "rb") as f:
                files[n] = f.read()
        exp = files["model"] if name.endswith(".mosh") else "\n".join(mm.mask_lines(files["model"])).encode()
        for n in ("prog", "slab"):
            got = files[n] if name.endswith(".mosh") else "\n".join(mm.mask_lines(files[n])).encode()
            assert got == exp, "%s (%s): %s" % (name, n, orc.describe_diff(got, exp))
    # the same chain through the Python class
    d = dirs["model"]
    seqs = {n: mm.parse_seq_bytes(open(os.path.join(d, n), "rb").read())[0] for n in ("a.fa", "x.fq", "b.fq")}
    ms = hash10x_amd.MoshSet(B=B, k=k, w=w, seed=seed)
    ms.add(*mm.flatten(seqs["a.fa"]))
    ms.add(*mm.flatten(seqs["x.fq"]), is10x=True)
    ms.add_file(os.path.join(d, "b.fq"))
    s1 = mm.MoshModel.from_bytes(open(os.path.join(d, "s1.mosh"), "rb").read())
    ix, v, dep, info = ms.export()
    assert v.tolist() == s1.value and dep.tolist() == s1.depth and info.tolist() == s1.info and np.array_equal(ix, s1.file_index)
    h, c = ms.hist()
    assert h[:len(s1.hist())].tolist() == s1.hist().tolist() and int(c.sum()) == s1.max
    ms.prune(2, 0); ms.set_copy(2, 3, 6)
    ms.write(os.path.join(d, "py_s2.mosh"))
    assert open(os.path.join(d, "py_s2.mosh"), "rb").read() == open(os.path.join(d, "s2.mosh"), "rb").read()
    un = hash10x_amd.MoshSet(B=B, k=k, w=w, seed=seed)
    assert un.merge(os.path.join(d, "s2.mosh")) and un.merge(os.path.join(d, "t.mosh"))
    un.set_copy_m(4)
    u = mm.MoshModel.from_bytes(open(os.path.join(d, "u.mosh"), "rb").read())
    ix, v, dep, info = un.export()
    assert v.tolist() == u.value and dep.tolist() == u.depth and info.tolist() == u.info and np.array_equal(ix, u.file_index)
    li, ld = ms.lookup(np.array(u.value[1:], np.uint64))
    s2 = mm.MoshModel.from_bytes(open(os.path.join(d, "s2.mosh"), "rb").read())
    assert li.tolist() == [s2.ix.get(x, 0) for x in u.value[1:]]
    assert ld.tolist() == [s2.depth[s2.ix.get(x, 0)] for x in u.value[1:]]
    other = hash10x_amd.MoshSet(B=B, k=k, w=w, seed=seed + 1)
    assert other.merge(os.path.join(d, "s2.mosh")) is False and other.max == 0
    for s in (ms, un, other):
        s.close()


# ---- the scan's second attempt: a batch that lists more moshes than the estimate its list is sized by ----------------------
# An assembly gap of N (code 0 = A) or a homopolymer run hashes to 0 at every position, and 0 is a mosh for every w: the batch lists
# every k-mer of the run, more than 2 * (k-mers / w) + 65536, and the scan runs again at the exact size (moshScanWith, stage_g.hip).
# slab 0: the three sequences of g.fa in one batch; 162000: the gapped one and the right flank together, as the issue's batch of two; 50000: the gapped one alone
@pytest.mark.parametrize("fill", ["N", "A", "T", None], ids=["N", "A", "T", "control"])
def test_add_second_attempt(fill, tmp_path):
    """-a of a batch that overflows its list while it also holds hashes that are found (they count in acc[] during the first attempt):
    .mosh and -H histogram equal the model's, value 0 is saturated, the flank moshes have depth 2 or 3 and not twice that; scan_retries
    rises by one per overflowing batch and stays 0 on random sequence of the same lengths"""
    import hash10x_amd
    k, w = 19, 31
    left, gapped, right = gap_seqs(fill)
    three = [gapped, right, left[:5000]]
    assert scan_cap([len(gapped)], k, w) == 74566 and len(gapped) - k + 1 == 139982           # the figures of the issue
    dm = os.path.join(str(tmp_path), "model"); os.makedirs(dm)
    write_fa(os.path.join(dm, "l.fa"), [left]); write_fa(os.path.join(dm, "g.fa"), three)
    cmd = [str(x) for x in ["-c", 20, k, w, 17, "-a", "l.fa", "-a", "g.fa", "-w", "s.mosh", "-H", "s.his"]]
    st, out, err = mm.run_commands(cmd, dm)
    assert st == 0, err
    model = mm.MoshModel.from_bytes(open(os.path.join(dm, "s.mosh"), "rb").read())
    listed = len(model.moshes(to_codes(gapped))[0])
    if fill:
        assert listed > scan_cap([len(s) for s in three], k, w) > scan_cap([len(gapped)], k, w) and listed >= GAP - k + 1
        assert model.depth[model.ix[0]] == 65535
        flank = {int(h) for s in (left, right) for h in model.moshes(to_codes(s))[0]} - {0}   # (a k-mer across a junction occurs once)
        assert len(flank) > 1000 and {model.depth[model.ix[h]] for h in flank} == {2, 3}
    else:
        assert listed < 6000 and 0 not in model.ix
    exp_his = "\n".join(mm.mask_lines(open(os.path.join(dm, "s.his"), "rb").read())).encode()
    for slab in (0, 162000, 50000):
        d = os.path.join(str(tmp_path), "slab%d" % slab); os.makedirs(d)
        for n in ("l.fa", "g.fa"):
            os.link(os.path.join(dm, n), os.path.join(d, n))
        r = run((["--slab", slab] if slab else []) + cmd, d)
        assert r.returncode == 0, r.stderr.decode()
        got = mm.mask_lines(r.stdout)
        if slab:
            got.remove("user")
        assert got == mm.mask_lines(out.encode())
        assert open(os.path.join(d, "s.mosh"), "rb").read() == open(os.path.join(dm, "s.mosh"), "rb").read(), "slab %d" % slab
        assert "\n".join(mm.mask_lines(open(os.path.join(d, "s.his"), "rb").read())).encode() == exp_his
        # the same batches through the class, where the counter can be read
        ms = hash10x_amd.MoshSet(B=20, k=k, w=w, seed=17)
        if slab:
            ms.set_option("mosh_slab", slab)
        ms.add(*mm.flatten([to_codes(left)]))
        assert ms.counters()["scan_retries"] == 0
        n = ms.add(*mm.flatten([to_codes(s) for s in three]))
        assert ms.counters()["scan_retries"] == (1 if fill else 0), "slab %d" % slab
        assert n == sum(len(model.moshes(to_codes(s))[0]) for s in three)
        ms.write(os.path.join(d, "py.mosh"))
        assert open(os.path.join(d, "py.mosh"), "rb").read() == open(os.path.join(dm, "s.mosh"), "rb").read(), "slab %d (class)" % slab
        h, c = ms.hist()
        assert h[:len(model.hist())].tolist() == model.hist().tolist() and int(h.sum()) == model.max
        ms.close()


@pytest.mark.parametrize("fill", ["N", "A", "T", None], ids=["N", "A", "T", "control"])
def test_scan_second_attempt_matches_reference_iterator(fill, tmp_path):
    """list mode: hashes, sequence numbers and positions in order, against the reference's own iterator (k 16, w 32, seed 1). Its test program reads N
    through another table than moshutils' reader does (N is code 0 = A there: the golden cases), so it is given the run as A where the scan is given N"""
    import hash10x_amd
    ref = os.path.join(orc.REF_DIR, "seqhash_test")
    if not os.path.exists(ref):
        pytest.fail("oracle/_ref/seqhash_test is missing: build() makes it where the reference is present")
    _, gapped, right = gap_seqs(fill)
    path = os.path.join(str(tmp_path), "g.fa")
    write_fa(path, [gapped.replace("N", "A"), right])
    r = subprocess.run([ref], input=open(path, "rb").read(), stdout=subprocess.PIPE, check=True)
    exp, s = [], -1
    for line in r.stdout.decode().splitlines():
        if line.startswith("read sequence"):
            s += 1
        elif line.startswith("\t"):
            h, p, _ = line.split()
            exp.append((int(h, 16), s, int(p)))
    overflow = bool(fill)
    assert (len(exp) > scan_cap([len(gapped), len(right)], 16, 32)) == overflow
    codes, start = mm.flatten([to_codes(gapped), to_codes(right)])
    for slab, retries in ((0, 1), (50000, 1)):                 # one batch of both; the gapped sequence alone
        ms = hash10x_amd.MoshSet(B=20, k=16, w=32, seed=1)
        if slab:
            ms.set_option("mosh_slab", slab)
        h, q, p = ms.scan(codes, start)
        # (MoshSet.scan calls h10x_mosh_scan a second time with room for all when the first call reports more moshes than its arrays hold: two scans of the batch)
        assert ms.counters()["scan_retries"] == (2 * retries if overflow else 0)
        assert list(zip(h.tolist(), q.tolist(), p.tolist())) == exp
        ms.close()


# ---- -x with a first read shorter than 23 bases (the reference aborts on an assert) ----------------------------------------
@pytest.mark.parametrize("slab", [0, 3000])
def test_short_10x_read_names_the_sequence(slab, tmp_path):
    """the number is the sequence's place in the FILE, carried over reader slabs and device batches (slab 3000: 30 reads each)"""
    import hash10x_amd
    d = str(tmp_path)
    rs = np.random.RandomState(23)
    lens = [100] * 401
    lens[299] = 5                                             # read 300 is a second read: any length will do
    ok = ["".join(np.array(list("ACGT"))[rs.randint(0, 4, n)]) for n in lens]
    bad = list(ok)
    bad[300] = bad[300][:22]                                  # read 301, a first read
    for name, reads in (("ok.fq", ok), ("short.fq", bad)):
        with open(os.path.join(d, name), "w") as f:
            f.write("".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)))
    pre = ["--slab", slab] if slab else []
    msg = "10x sequence 301 has 22 bases: the first read of a pair needs at least 23"
    r = run(pre + ["-c", 20, 19, 31, 17, "-x", "short.fq", "-w", "never.mosh"], d)
    assert r.returncode == 255 and r.stderr.decode().splitlines()[-1] == "FATAL ERROR: " + msg
    assert not os.path.exists(os.path.join(d, "never.mosh"))
    st, out, err = mm.run_commands(["-c", "20", "19", "31", "17", "-x", "short.fq"], d)
    assert st == 255 and err.splitlines()[-1] == "FATAL ERROR: " + msg
    seqs = [np.array(["ACGT".index(c) for c in r], np.uint8) for r in bad]
    ms = hash10x_amd.MoshSet(B=20, k=19, w=31, seed=17)
    if slab:
        ms.set_option("mosh_slab", slab)
    with pytest.raises(hash10x_amd.Hash10xError) as e:
        ms.add(*mm.flatten(seqs), is10x=True)
    assert str(e.value) == msg
    with pytest.raises(hash10x_amd.Hash10xError) as e:       # the same reads handed over in two calls: seq_base carries the count
        ms.add(*mm.flatten(seqs[250:]), is10x=True, seq_base=250)
    assert str(e.value) == msg
    with pytest.raises(hash10x_amd.Hash10xError) as e:
        ms.add_file(os.path.join(d, "short.fq"), is10x=True, slab=slab)
    assert str(e.value) == msg
    ms.close()
    r = run(pre + ["-c", 20, 19, 31, 17, "-x", "ok.fq", "-w", "ok.mosh"], d)          # the short SECOND read is fine
    st, out, err = mm.run_commands(["-c", "20", "19", "31", "17", "-x", "ok.fq", "-w", "model.mosh"], d)
    assert r.returncode == 0 == st
    got = mm.mask_lines(r.stdout)
    if pre:
        got.remove("user")
    assert got == mm.mask_lines(out.encode())
    assert open(os.path.join(d, "ok.mosh"), "rb").read() == open(os.path.join(d, "model.mosh"), "rb").read()


# ---- the table-full stop ------------------------------------------------------------------------------------------------
def test_table_full_stop(tmp_path):
    import hash10x_amd
    codes = np.random.RandomState(9).randint(0, 4, 9000000).astype(np.uint8)
    hs, _ = orc.Oracle(19, 31, 17, 20).mosh(codes)
    assert len(np.unique(hs)) >= 262143
    path = os.path.join(str(tmp_path), "big.fa")
    with open(path, "wb") as f:
        f.write(b">big\n" + np.frombuffer(b"ACGT", np.uint8)[codes].tobytes() + b"\n")
    r = run(["-c", 20, 19, 31, 17, "-a", "big.fa", "-w", "never.mosh"], str(tmp_path))
    assert r.returncode == 255
    assert r.stderr.decode().splitlines()[-1] == "FATAL ERROR: hashTableSize 262143 is too small for 262143"
    assert not os.path.exists(os.path.join(str(tmp_path), "never.mosh"))
    ms = hash10x_amd.MoshSet(B=20, k=19, w=31, seed=17)
    with pytest.raises(hash10x_amd.Hash10xError, match="^hashTableSize 262143 is too small for 262143$"):
        ms.add(codes, np.array([0, len(codes)], np.uint64))
    ms.close()


# ---- one larger run at B = 28 ---------------------------------------------------------------------------------------------
def test_large_set_b28():
    import hash10x_amd
    t0 = time.time()
    rs = np.random.RandomState(28)
    base = rs.randint(0, 4, 24000000).astype(np.uint8)
    seqs = [base[:9000000], base[9000000:], base[2000000:5000000], base[1000:1000 + 70000]] + [base[4000000:4000300]] * 70000
    o = orc.Oracle(19, 31, 17, 20)
    allh = []
    for s in seqs[:4]:
        allh.append(o.mosh(s)[0])
    rep = o.mosh(seqs[4])[0]
    allh.append(np.tile(rep, 70000))
    allh = np.concatenate(allh)
    u, first, cnt = np.unique(allh, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    ms = hash10x_amd.MoshSet(B=28, k=19, w=31, seed=17)
    ms.set_option("mosh_slab", 1 << 23)                       # several batches; the 9 and 15 Mbase sequences go alone
    n = ms.add(*mm.flatten(seqs))
    assert n == len(allh)
    ms.set_copy(2, 3, 1000)
    ix, v, dep, info = ms.export()
    ms.close()
    N = len(u)
    expd = np.minimum(cnt[order], 65535)
    assert len(rep) > 0 and expd.max() == 65535                 # the repeats saturate
    assert len(v) == N + 1 and np.array_equal(v[1:], u[order]) and v[0] == 0
    assert np.array_equal(dep[1:], expd.astype(np.uint16))
    assert np.array_equal(info[1:], np.where(expd < 2, 0, np.where(expd < 3, 1, np.where(expd < 1000, 2, 3))).astype(np.uint8))
    # the table by its defining property (one solution): exactly max non-zero entries, every index found by its probe walk,
    # and before its slot only lower indices
    assert np.count_nonzero(ix) == N and int(ix.max()) == N
    mask = np.uint64((1 << 28) - 1)
    me = np.arange(1, N + 1, dtype=np.uint32)
    slot = (v[1:] & mask).astype(np.int64)
    step = (((v[1:] >> np.uint64(28)) & mask) | np.uint64(1)).astype(np.int64)
    mask = np.int64(mask)
    todo = np.arange(N)
    for _ in range(10000):
        cur = ix[slot[todo]]
        found = cur == me[todo]
        assert np.all((cur[~found] != 0) & (cur[~found] < me[todo][~found]))
        todo = todo[~found]
        if not len(todo):
            break
        slot[todo] = (slot[todo] + step[todo]) & mask
    assert not len(todo)
    print("B = 28: %d occurrences, %d distinct, %.1f s" % (len(allh), N, time.time() - t0))
