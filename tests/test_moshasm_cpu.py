"""The device-free half of moshasm-amd: the model of tests/asm_model.py against the reference's golden fixtures (byte for byte —
this is what pins the stable tie order of the overlap sort and the RSMSHv2 layout), the fixture conditions, the host RSMSHv2
reader and writer through ctypes and through the sanitizer build on good and malformed files, the command-line cases that never
reach a device, and the new symbols."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import asm_model as am
import mosh_model as mm
import orc

MAN = am.manifest()
EXE = os.path.join(orc.REPO, "bin", "moshasm-amd")
ASAN = os.path.join(orc.REPO, "build", "moshasm-amd-asan")


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
    before = am.stage_case(MAN, case, d)
    st, out, err = am.run_commands(case["args"], d)
    am.check_case(case, d, before, st, out.encode(), err.encode())


def test_fixture_conditions():
    """what make_asm_golden.py refused to go without, read back from the manifest"""
    c = MAN["conditions"]
    assert len(c["bad_line"]) == 7 and all(c["bad_line"])       # bad, repeat, order10, order1, no_match, low_hit, low_copy1 after -b
    assert len(c["mb"]) == 3 and all(c["mb"])                    # each pass of -b finds reads
    assert c["minus_only"] > 0 and c["mixed"] > 0 and c["contained"] > 0 and c["tie_decided"] > 0 and c["dx_wrapped_reads"] > 0
    by = {x["name"]: x for x in MAN["cases"]}
    bad = [ln for ln in by["bad"]["stdout"] if ln.startswith("RS bad")][0]
    assert bad == "RS bad %d : %d repeat, %d order10, %d order1, %d no_match, %d low_hit, %d low_copy1" % tuple(c["bad_line"])
    assert [int(ln.split()[1]) for ln in by["bad"]["stdout"] if ln.startswith("MB")] == c["mb"]
    rh = [ln for x in MAN["cases"] if x["name"].startswith("o1_") for ln in x["stdout"] if ln.startswith("RH")]
    assert any("nPlus 0\t" in ln and "nMinus 0\t" not in ln for ln in rh)
    assert any("nPlus 0\t" not in ln and "nMinus 0\t" not in ln and "BAD" in ln for ln in rh)
    # the tie: the read planted inside two containers with the same hits goes to the one met first
    sp = MAN["special"]
    rc = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(am.gold("badc.rc.mosh")), am.gold("badc.rc.readset"))
    assert rc.reads[sp["contained_tie"]].contained == sp["container1"]
    # the wrapped dx: the read is longer than its dx add up to
    rs = am.ReadsetModel.from_bytes(mm.MoshModel.from_bytes(am.gold("build.rs.mosh")), am.gold("build.rs.readset"))
    r = rs.reads[sp["dx_wrap"]]
    assert r.len > 66000 and sum(r.dx) < 66000 and r.nHit > 20
    assert rs.reads[sp["empty"]].len == 0 and rs.reads[sp["shorter_than_k"]].nHit == 0 and rs.reads[0].nHit == 0


def _stage(d):
    for n in ("rs.mosh", "rs.readset"):
        with open(os.path.join(d, n), "wb") as f:
            f.write(am.gold("badc.rc." + n.split(".")[1]))
    return os.path.join(d, "rs.readset")


def test_readset_file_reader_and_writer_on_fixture(amd, tmp_path):
    d = str(tmp_path)
    p = _stage(d)
    data = open(p, "rb").read()
    ms = mm.MoshModel.from_bytes(open(os.path.join(d, "rs.mosh"), "rb").read())
    model = am.ReadsetModel.from_bytes(ms, data)
    f = amd.read_readset_file(p, ms.max)
    assert (f["totHit"], f["dim"], len(f["reads"])) == (model.totHit, model.dim, len(model.reads))
    assert f["reads"]["nHit"].tolist() == [r.nHit for r in model.reads] and f["reads"]["bad"].tolist() == [r.bad for r in model.reads]
    assert f["reads"]["contained"].tolist() == [r.contained for r in model.reads] and f["reads"]["nCopy"].tolist() == [r.nCopy for r in model.reads]
    assert f["hit"].tolist() == [h for r in model.reads for h in r.hit] and f["dx"].tolist() == [x for r in model.reads for x in r.dx]
    hs = np.concatenate([[0], np.cumsum(f["reads"]["nHit"])]).astype(np.uint64)
    amd.write_readset_file(os.path.join(d, "again.readset"), f["totHit"], f["dim"], f["reads"], hs, f["hit"], f["dx"])
    assert open(os.path.join(d, "again.readset"), "rb").read() == data == model.to_bytes()


def _bad_readset_files(g, set_max):
    dim, size, mx = struct.unpack_from("<iii", g, 32)
    rec = 48
    hits0 = 48 + 72 * dim
    first = next(i for i in range(mx) if struct.unpack_from("<i", g, rec + 72 * i + 4)[0])      # first read with hits
    n = struct.unpack_from("<i", g, rec + 72 * first + 4)[0]
    beyond = bytearray(g); struct.pack_into("<I", beyond, hits0 + 8, set_max + 1)
    zero = bytearray(g); struct.pack_into("<I", zero, hits0, 0x80000000)
    many = bytearray(g); struct.pack_into("<i", many, rec + 72 * first + 4, 65535)
    neg = bytearray(g); struct.pack_into("<i", neg, rec + 72 * first + 4, -1)
    tot = bytearray(g); struct.pack_into("<Q", tot, 8, struct.unpack_from("<Q", g, 8)[0] + 1)
    return [("short_header", g[:5], "failed to read readset header"),
            ("magic", b"RSMSHv1\0" + g[8:], "bad readset header RSMSHv1 != RSMSHv2"),
            ("tothit", g[:12], "failed to read totHit"),
            ("array_head", g[:40], "failed to read the reads array"),
            ("size", g[:36] + struct.pack("<i", 64) + g[40:], "readset record size 64 != 72"),
            ("max_over_dim", g[:40] + struct.pack("<i", dim + 1) + g[44:], "readset max %d outside 1 .. dim %d" % (dim + 1, dim)),
            ("max_zero", g[:40] + struct.pack("<i", 0) + g[44:], "readset max 0 outside 1 .. dim %d" % dim),
            ("records", g[:hits0 - 100], "failed to read the reads array"),
            ("huge_dim", g[:32] + struct.pack("<i", 0x7FFFFFFF) + g[36:], "failed to read the reads array"),
            ("hits", g[:hits0 + 4 * n - 2], "failed read hits"),
            ("dx", g[:hits0 + 4 * n + 2 * n - 1], "failed read dx"),
            ("last_dx", g[:-1], "failed read dx"),
            ("beyond", bytes(beyond), "read %d holds mosh index %d outside 1 .. %d" % (first, set_max + 1, set_max)),
            ("index_zero", bytes(zero), "read %d holds mosh index 0 outside 1 .. %d" % (first, set_max)),
            ("too_many", bytes(many), "read %d has 65535 hits: more than 65534 are not supported" % first),
            ("negative", bytes(neg), "read %d has -1 hits: more than 65534 are not supported" % first),
            ("tothit_sum", bytes(tot), "readset totHit %d but the reads hold %d hits" % (struct.unpack_from("<Q", g, 8)[0] + 1, struct.unpack_from("<Q", g, 8)[0]))]


@pytest.mark.parametrize("i", range(17))
def test_readset_file_reader_refuses_malformed(i, amd, tmp_path):
    d = str(tmp_path)
    good = open(_stage(d), "rb").read()
    ms = mm.MoshModel.from_bytes(open(os.path.join(d, "rs.mosh"), "rb").read())
    name, data, msg = _bad_readset_files(good, ms.max)[i]
    with open(os.path.join(d, "rs.readset"), "wb") as f:
        f.write(data)
    with pytest.raises(amd.Hash10xError) as e:
        amd.read_readset_file(os.path.join(d, "rs.readset"), ms.max)
    assert str(e.value) == msg
    if name != "huge_dim":                                      # (the model reads the file whole)
        with pytest.raises(mm.ModelDie) as e2:
            am.ReadsetModel.from_bytes(ms, data)
        assert str(e2.value) == "FATAL ERROR: " + msg
    for exe in (EXE, ASAN):                                   # -r parses both files before any device is opened
        rc, out, err = cli(exe, ["-r", "rs"], d)
        assert rc == 255 and err.splitlines() == ["COMMAND -r rs", "FATAL ERROR: " + msg]


def test_command_line_without_a_device(amd, tmp_path):
    d = str(tmp_path)
    _stage(d)
    for exe in (EXE, ASAN):
        rc, out, err = cli(exe, [], d)
        assert rc == 0 and err.startswith("Usage: moshasm-amd <commands>") and "--device <n>" in err and "--assemble1" in err
        assert mm.mask_lines(out.encode()) == ["total resources used: user"]
        for name in ("unknown", "no_dash", "no_mosh", "no_stem", "f_before_m", "bad_output", "short_args"):     # the reference's own runs
            case = [c for c in MAN["cases"] if c["name"] == name][0]
            rc, out, err = cli(exe, case["args"], d)
            assert (rc, mm.mask_lines(out.encode()), mm.mask_lines(err.encode())) == (case["status"], case["stdout"], case["stderr"]), name
        os.rename(os.path.join(d, "rs.readset"), os.path.join(d, "away"))
        rc, out, err = cli(exe, ["-r", "rs"], d)
        assert rc == 255 and err.splitlines()[-1] == "FATAL ERROR: can't open file rs.readset"
        os.rename(os.path.join(d, "away"), os.path.join(d, "rs.readset"))
        for args, last in ((["-S"], "-S needs a readset: give -f or -r first"), (["--write", "x"], "--write needs a readset: give -f or -r first"),
                           (["-o1", "1"], "-o1 needs a readset: give -f or -r first"), (["-o2", "1"], "-o2 needs a readset: give -f or -r first"),
                           (["-o3", "1", "2"], "-o3 needs a readset: give -f or -r first"), (["-b"], "-b needs a readset: give -f or -r first"),
                           (["-c"], "-c needs a readset: give -f or -r first"), (["-a1", "1"], "-a1 needs a readset: give -f or -r first"),
                           (["-o3", "1"], "unkown command -o3 - run without arguments for usage"),
                           (["--slab", "0"], "bad slab 0: 1 to 4294967295 bases")):
            rc, out, err = cli(exe, args, d)
            assert rc == 255 and err.splitlines()[-1] == "FATAL ERROR: " + last, (args, err)
            if args[0] != "--slab":
                st, mout, merr = am.run_commands(args, d)
                assert st == 255 and merr.splitlines() == err.splitlines()
    if amd.device_count() == 0:                                 # the device is opened by -m / -r, and there is no CPU fallback
        rc, out, err = cli(EXE, ["-r", "rs"], d)
        assert rc == 255 and err.splitlines()[-1].startswith("FATAL ERROR: no HIP device available")
        with pytest.raises(amd.Hash10xError, match="no HIP device available"):
            amd.ReadSet.read(os.path.join(d, "rs"))


def test_new_symbols_are_exported(amd):
    hip, host = amd.load_native()
    for n in ("create", "add", "load", "export", "info", "overlap_cap", "overlaps", "mark_bad", "mark_contained", "stats_sums", "destroy", "error"):
        assert hasattr(hip, "h10x_readset_" + n), n
    for n in ("h10x_readsetfile_read", "h10x_readsetfile_write", "h10x_readsetfile_free", "h10x_readset_write_file", "h10x_readset_add_file",
              "h10x_readset_print_stats", "h10x_readset_print_overlaps", "h10x_readset_print_pair", "h10x_readset_print_assembly"):
        assert hasattr(host, n), n
    assert hip.h10x_abi_version() == 3                          # symbols were added, nothing changed
    assert amd.READ_DTYPE.itemsize == 72 and callable(amd.ReadSet.mark_contained)
    assert os.path.exists(EXE) and os.path.exists(ASAN)
