"""The device-free half of moshutils-amd: the model of tests/mosh_model.py against the reference's golden fixtures (byte for
byte), the host sequence reader and MSHSTv1 reader through ctypes and through the sanitizer build on good and malformed
input, the seed helper, and the command-line cases that never reach a device."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import mosh_model as mm
import orc

MAN = mm.manifest()
EXE = os.path.join(orc.REPO, "bin", "moshutils-amd")
ASAN = os.path.join(orc.REPO, "build", "moshutils-amd-asan")


@pytest.fixture(scope="module")
def amd():
    import hash10x_amd
    hash10x_amd.load_native()
    return hash10x_amd


def cli(exe, args, cwd):
    if not os.path.exists(exe):
        pytest.fail("%s is missing: run build()" % exe)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err
    return r.returncode, r.stdout.decode(errors="replace"), err


@pytest.mark.parametrize("case", MAN["cases"], ids=[c["name"] for c in MAN["cases"]])
def test_model_reproduces_reference_golden(case, tmp_path):
    d = str(tmp_path)
    before = mm.stage_case(MAN, case, d)
    st, out, err = mm.run_commands(case["args"], d)
    mm.check_case(case, d, before, st, out.encode(), err.encode())


def test_merge_fixture_tells_or_from_replace():
    assert MAN["merge_or_differs"] > 0
    merge = [c for c in MAN["cases"] if c["name"] == "merge"][0]
    assert any(" copy2 0 " in ln for ln in merge["stdout"] if ln.startswith("MS average"))


def test_full_set_fixture():
    n = struct.unpack_from("<I", mm.read_maybe_gz(os.path.join(mm.GOLD, "build.g.mosh.gz")), 12)[0]      # max + 1 of g.mosh: a set that was read is full
    assert n > 1000
    for name in ("full_add", "full_merge"):
        c = [c for c in MAN["cases"] if c["name"] == name][0]
        assert c["status"] == 255 and c["stderr"][-1] == "FATAL ERROR: hashTableSize %d is too small for %d" % (n, n)
    sat = [c for c in MAN["cases"] if c["name"] == "saturation"][0]
    assert any("total count 65535" in ln for ln in sat["stdout"])
    assert mm.read_maybe_gz(os.path.join(mm.GOLD, "saturation.rep.his.gz")).decode().split("\n") == ["DP\t65535\t1"]


def test_factors_from_seed(amd):
    hip = amd.load_native()[0]
    for seed in (17, 18, 1, 5, 3):
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        hip.h10x_factors_from_seed(seed, ctypes.byref(a), ctypes.byref(b))
        assert (a.value, b.value) == mm.factors(seed)
        assert a.value == hip.h10x_factor1_from_seed(seed) == orc.lib().orc_factor1_from_seed(seed)
    assert mm.factors(17)[0] == 0x49308BB9003CB3AD            # SURVEY KAT-1; factor2 of seeds 17 / 18 is pinned by the golden file headers


@pytest.mark.parametrize("name", MAN["inputs"] + ["g.fa.gz"])
def test_reader_matches_model_on_fixture_inputs(name, amd, tmp_path):
    d = str(tmp_path)
    mm.stage_case(MAN, {"needs": []}, d)
    data = mm.read_maybe_gz(os.path.join(d, name))
    seqs, warn = mm.parse_seq_bytes(data, name)
    ec, es = mm.flatten(seqs)
    for slab in (0, 1000):
        codes, start, w = amd.read_sequences(os.path.join(d, name), slab)
        assert np.array_equal(start, es) and np.array_equal(codes, ec)
        assert ([w] if w else []) == warn
    rc, out, err = cli(ASAN, ["--check", name], d)
    assert rc == 0 and out.splitlines()[0] == "checked %d sequences total length %d" % (len(seqs), len(ec))
    assert err.splitlines()[1:] == warn


BAD_SEQ = [
    ("short_qual.fq", b"@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", "qual not same length as seq line 4"),
    ("no_plus.fq", b"@a\nACGT\nIIII\n@b\nAC\n+\nII\n", "missing + FASTQ line 3"),
    ("bad_base.fq", b"@a\nACGT\n+\nIIII\n@b\nACRT\n+\nIIII\n", "bad base 0x52 in FASTQ line 6"),
    ("crlf.fq", b"@a\r\nACGT\r\n+\r\nIIII\r\n", "bad base 0x0d in FASTQ line 2"),
    ("high.fq", b"@a\nAC\xe9T\n+\nIIII\n", "bad base 0xe9 in FASTQ line 2"),
    ("high.fa", b">a\nACGT\nAC\xe9T\n", "bad base 0xe9 in FASTA line 3"),
    ("no_at.fq", b"@a\nACGT\n+\nIIII\nb\nAC\n+\nII\n", "no initial @ for FASTQ record line 5"),
    ("binary.sq", b"B\x00\x00\x00\x00\x00\x00\x00rest", "sequence file binary.sq is in seqio's binary format, which is not supported"),
    ("empty.fa", b"", "sequence file empty.fa unreadable or empty\nfailed to open sequence file empty.fa"),
    ("unknown.txt", b"hello\n", "sequence file unknown.txt is unknown type\nfailed to open sequence file unknown.txt"),
]


@pytest.mark.parametrize("name,data,msg", BAD_SEQ, ids=[b[0] for b in BAD_SEQ])
def test_reader_refuses_malformed_sequence_files(name, data, msg, amd, tmp_path):
    d = str(tmp_path)
    with open(os.path.join(d, name), "wb") as f:
        f.write(data)
    with pytest.raises(amd.Hash10xError) as e:
        amd.read_sequences(os.path.join(d, name))
    assert str(e.value).replace(d + "/", "") == msg
    with pytest.raises(mm.ModelDie) as e2:                    # the model takes the same decisions
        mm.parse_seq_bytes(data, name)
    assert str(e2.value).replace("FATAL ERROR: ", "").split(" line")[0].split(" in FAST")[0] == msg.split(" line")[0].split(" in FAST")[0]
    for exe in (EXE, ASAN):
        rc, out, err = cli(exe, ["--check", name], d)
        lines = err.splitlines()
        assert rc == 255 and lines[0] == "COMMAND --check " + name
        assert lines[1:] == msg.split("\n")[:-1] + ["FATAL ERROR: " + msg.split("\n")[-1]]
    rc, out, err = cli(EXE, ["--check", "missing." + name], d)
    assert rc == 255 and err.splitlines()[-1] == "FATAL ERROR: failed to open sequence file missing." + name


def test_reader_incomplete_records(amd, tmp_path):
    d = str(tmp_path)
    for name, data, nseq, line in (("h.fa", b">a\nACGT\n>b\n", 1, 4), ("h2.fa", b">a\nACGT\n>b", 1, 3), ("q.fq", b"@a\nACGT\n+\nIIII", 0, 4),
                                   ("q2.fq", b"@a\nACGT\n+\nIIII\n@b\nAC\n", 1, 7)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
        codes, start, warn = amd.read_sequences(os.path.join(d, name))
        seqs, mwarn = mm.parse_seq_bytes(data, name)
        assert len(start) - 1 == nseq == len(seqs)
        assert [warn] == mwarn == ["incomplete sequence record line %d" % line]


def _good_mosh():
    return mm.read_maybe_gz(os.path.join(mm.GOLD, "iupac.iupac.mosh.gz"))


def test_mosh_file_reader_on_fixture(amd, tmp_path):
    p = os.path.join(str(tmp_path), "ok.mosh")
    data = _good_mosh()
    with open(p, "wb") as f:
        f.write(data)
    f = amd.read_mosh_file(p)
    m = mm.MoshModel.from_bytes(data)
    assert (f["B"], f["k"], f["w"], f["factor1"], f["factor2"], f["size"]) == (20, 19, 31) + mm.factors(17) + (m.max + 1,)
    assert f["value"][1:].tolist() == m.value[1:] and f["depth"].tolist() == m.depth and f["info"].tolist() == m.info
    assert np.array_equal(f["index"], m.table())


def _bad_mosh_files():
    g = _good_mosh()
    size = struct.unpack_from("<I", g, 12)[0]
    slot = int(np.flatnonzero(np.frombuffer(g, "<u4", 1 << 20, 96))[0])
    beyond = bytearray(g); struct.pack_into("<I", beyond, 96 + 4 * slot, size + 5)
    zeroed = bytearray(g); struct.pack_into("<I", zeroed, 96 + 4 * slot, 0)
    voff = 96 + (4 << 20)
    v1 = struct.unpack_from("<Q", g, voff + 8)[0]
    repeat = bytearray(g); struct.pack_into("<Q", repeat, voff + 16, v1)          # value[2] = value[1]
    return [("short_header.mosh", g[:5], "failed to read moshset header"),
            ("magic.mosh", b"MSHSTv2\0" + g[8:], "bad reference header"),
            ("bits.mosh", g[:10], "failed to read bits"),
            ("seqhash_magic.mosh", g[:16] + b"SQHSHv9\0" + g[24:], "seqhash read mismatch"),
            ("seqhash.mosh", g[:60], "failed to read seqhash"),
            ("B.mosh", g[:8] + struct.pack("<i", 19) + g[12:], "table bits 19 must be between 20 and 34"),
            ("size.mosh", g[:12] + struct.pack("<I", 1 << 18) + g[16:], "Moshset size 262144 is too big for 20 bits"),
            ("index.mosh", g[:96 + 1000], "failed read index"),
            ("value.mosh", g[:96 + (4 << 20) + 8 * size - 3], "failed to read value"),
            ("depth.mosh", g[:96 + (4 << 20) + 9 * size], "failed to read depth"),
            ("info.mosh", g[:-1], "failed to read info"),
            ("longer.mosh", g + b"x", "mosh file longer.mosh holds 1 bytes more than its header implies"),
            ("beyond.mosh", bytes(beyond), "mosh file beyond.mosh: table entry %d at slot %d is beyond max %d" % (size + 5, slot, size - 1)),
            ("zeroed.mosh", bytes(zeroed), "mosh file zeroed.mosh: %d table entries for %d hashes" % (size - 2, size - 1)),
            ("repeat.mosh", bytes(repeat), "mosh file repeat.mosh: entry 2 (hash %x) is not where its probe walk ends (found 1): repeated value or foreign table" % v1)]


@pytest.mark.parametrize("i", range(15))
def test_mosh_file_reader_refuses_malformed(i, amd, tmp_path):
    name, data, msg = _bad_mosh_files()[i]
    d = str(tmp_path)
    with open(os.path.join(d, name), "wb") as f:
        f.write(data)
    with pytest.raises(amd.Hash10xError) as e:
        amd.read_mosh_file(os.path.join(d, name))
    assert str(e.value).replace(d + "/", "") == msg
    for exe in (EXE, ASAN):                                   # -r stops at the file, before any device is opened
        rc, out, err = cli(exe, ["-r", name], d)
        assert rc == 255 and err.splitlines() == ["COMMAND -r " + name, "FATAL ERROR: " + msg]


def test_command_line_without_a_device(amd, tmp_path):
    d = str(tmp_path)
    for exe in (EXE, ASAN):
        rc, out, err = cli(exe, [], d)
        assert rc == 0 and err.startswith("Usage: moshutils-amd <commands>") and "--device <n>" in err and "--depths" in err
        assert mm.mask_lines(out.encode()) == ["total resources used: user"]
        for args, last in ((["-w", "x.mosh"], "unknown command -w - run without arguments for usage"),
                           (["-a", "x.fa"], "unknown command -a - run without arguments for usage"),
                           (["--moshcreate"], "unknown command --moshcreate - run without arguments for usage"),
                           (["-p", "2"], "unknown command -p - run without arguments for usage"),
                           (["x"], "option/command x does not start with '-': run without arguments for usage"),
                           (["-r", "nosuch.mosh"], "failed to open mosh file nosuch.mosh"),
                           (["-c", "19"], "bad moshbuild B 19"), (["-c", "35"], "bad moshbuild B 35"), (["-c", "x"], "bad moshbuild B x"),
                           (["-c", "20", "0"], "bad moshbuild k 0"), (["-c", "20", "19", "0"], "bad moshbuild w 0"),
                           (["--create", "20", "19", "31", "0"], "bad moshbuild w 0")):
            rc, out, err = cli(exe, args, d)
            assert rc == 255 and err.splitlines()[-1] == "FATAL ERROR: " + last, (args, err)
            st, mout, merr = mm.run_commands(args, d)
            assert st == 255 and merr.splitlines() == err.splitlines()
        rc, out, err = cli(exe, ["-v", "-o", "/nonexistent/dir/x", "-o", "-"], d)
        assert rc == 0 and "can't open output file /nonexistent/dir/x - resetting to stdout" in err
    for w in (0, -5):                                         # seqhashCreate's w check (seqhash.c:25); the command line cannot pass w < 1
        with pytest.raises(amd.Hash10xError, match=r"^seqhash w %d must be positive\n$" % w):      # ("-5" is the next command there, "0" is "bad moshbuild w")
            amd.MoshSet(B=20, k=19, w=w)
    with pytest.raises(amd.Hash10xError, match=r"^seqhash k 0 must be between 1 and 32\n$"):
        amd.MoshSet(B=20, k=0)
    with pytest.raises(amd.Hash10xError, match=r"^table bits 35 must be between 20 and 34$"):
        amd.MoshSet(B=35)
    for bad in ("0", "4294967296", "12x", "-1"):
        rc, out, err = cli(EXE, ["--slab", bad], d)
        assert rc == 255 and err.splitlines()[-1] == "FATAL ERROR: bad slab %s: 1 to 4294967295 bases" % bad
    rc, out, err = cli(EXE, ["--slab", "4294967295"], d)
    assert rc == 0
    rc, out, err = cli(EXE, ["-c", "20", "32"], d)            # seqhashCreate's die, newline included (seqhash.c:24), comes before the set
    assert rc == 255 and err.split("\n")[-3:] == ["FATAL ERROR: seqhash k 32 must be between 1 and 32", "", ""]
    if amd.device_count() == 0:                               # the device is opened by -c / -r, and there is no CPU fallback
        rc, out, err = cli(EXE, ["-c", "20"], d)
        assert rc == 255 and err.splitlines()[-1].startswith("FATAL ERROR: no HIP device available")
        good = os.path.join(d, "ok.mosh")
        with open(good, "wb") as f:
            f.write(_good_mosh())
        rc, out, err = cli(EXE, ["-r", "ok.mosh"], d)
        assert rc == 255 and err.splitlines()[-1].startswith("FATAL ERROR: no HIP device available")
        with pytest.raises(amd.Hash10xError, match="no HIP device available"):
            amd.MoshSet(B=20)
        with pytest.raises(amd.Hash10xError, match="no HIP device available"):
            amd.MoshSet.read(good)
