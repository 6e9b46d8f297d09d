"""The barcode census and whitelist correction of .fqb records without a GPU: the numpy model of tests/fqb_model.py against the
reference's fq2b (fresh input and the recorded files of tests/golden/fixfqb), the whitelist text reader of libh10x_host.so, and
the usage text."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fqb_model as fm
import orc

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
needs_fq2b = pytest.mark.skipif(not os.path.exists(fm.FQ2B_REF), reason="oracle/_ref/fq2b not present")


@pytest.fixture(scope="module")
def host():
    import hash10x_amd
    try:
        return hash10x_amd.load_native()[1]
    except hash10x_amd.Hash10xError:
        import __graft_entry__
        __graft_entry__.build()
        return hash10x_amd.load_native()[1]


@pytest.fixture(scope="module")
def fresh(tmp_path_factory):
    return fm.fresh_case(str(tmp_path_factory.mktemp("fixfqb")))


@needs_fq2b
@pytest.mark.parametrize("T", fm.FRESH_T)
def test_model_equals_reference_on_fresh_input(fresh, T):
    """4000 pairs (barcodes with N, good barcodes one substitution apart): the model's fix of the raw file with the ascending
    goodcodes of threshold T gives the bytes and the statistics lines of the reference's `fq2b -10x`"""
    recs = np.frombuffer(fresh["raw"], dtype=np.uint32).reshape(-1, 30)
    assert recs.shape[0] == 4000
    codes, counts, good = fm.census(recs, T)
    assert np.all(np.diff(codes.astype(np.int64)) > 0) and int(counts.sum()) == 4000 and np.array_equal(good, fresh[T]["codes"])
    if T == 1:
        assert good.size == codes.size
    out, st = fm.fix(recs, good)
    assert out.tobytes() == fresh[T]["bytes"]
    exp = ("read %d barcodes from file %s\n" % (good.size, fresh[T]["good"])).encode() + fm.stats_lines(out.shape[0], st)
    assert exp == fresh[T]["stderr"]
    assert st["corrected"] > 0 and (T == 1 or st["dropped"] > 0)


def test_model_equals_recorded_reference():
    raw = np.fromfile(os.path.join(fm.GOLDEN, "raw.fqb"), dtype=np.uint32).reshape(-1, 30)
    words = open(os.path.join(fm.GOLDEN, "goodcodes.txt")).read().split()
    good = fm.census(raw, 3)[2]
    assert fm.text(good) == open(os.path.join(fm.GOLDEN, "goodcodes.txt")).read() and np.array_equal(fm.pack(words), good)
    out, st = fm.fix(raw, good)
    assert out.tobytes() == open(os.path.join(fm.GOLDEN, "fixed.fqb"), "rb").read()
    exp = b"read %d barcodes from file goodcodes.txt\n" % good.size + fm.stats_lines(out.shape[0], st)
    assert exp == open(os.path.join(fm.GOLDEN, "fixed.stderr.txt"), "rb").read()


@needs_fq2b
def test_model_honours_whitelist_line_order(tmp_path):
    """a whitelist in no order, with shadowing neighbours and a repeated line: the model equals the reference"""
    wl = fm.shadow_whitelist(np.random.default_rng(5))
    fm.write_fastq_for_whitelist(str(tmp_path), wl, 900, 6)
    (tmp_path / "wl.txt").write_text("\n".join(wl) + "\n")
    raw, _ = fm.run_fq2b_ref(str(tmp_path), "raw.fqb")
    exp, err = fm.run_fq2b_ref(str(tmp_path), "ref.fqb", "wl.txt")
    out, st = fm.fix(np.frombuffer(raw, dtype=np.uint32), fm.pack(wl))
    assert out.tobytes() == exp and 0 < len(exp) < len(raw)
    assert b"read %d barcodes from file wl.txt\n" % len(wl) + fm.stats_lines(out.shape[0], st) == err


def _read(host, path):
    codes, n, err = ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.create_string_buffer(512)
    rc = host.h10x_host_whitelist_read(os.fsencode(str(path)), ctypes.byref(codes), ctypes.byref(n), err, 512)
    if rc:
        return None, err.value
    out = np.ctypeslib.as_array(ctypes.cast(codes, ctypes.POINTER(ctypes.c_uint32)), shape=(max(n.value, 1),))[:n.value].copy() if n.value else np.zeros(0, np.uint32)
    host.h10x_host_whitelist_free(codes)
    return out, b""


def test_whitelist_reader(host, tmp_path):
    words = ["ACGTACGTACGTACGT", "TTTTTTTTTTTTTTTT", "acgtNcgtacgtacgx", "AAAAAAAAAAAAAAAA", "ACGTACGTACGTACGT", "TTTTTTTTTTTTTTTT"]
    (tmp_path / "wl.txt").write_text("\n".join(words) + "\n")
    codes, _ = _read(host, tmp_path / "wl.txt")
    assert np.array_equal(codes, fm.pack(words))                                        # line order, lower case and N accepted (N and x pack as A)
    assert codes[2] == fm.pack(["ACGTACGTACGTACGA"])[0] and codes[3] == 0 and codes[1] == 0xFFFFFFFF
    q = np.array([codes[0], codes[1], codes[2], 0, 12345], dtype=np.uint32)
    lines = np.zeros(q.size, dtype=np.uint32)
    assert host.h10x_host_whitelist_lines(codes.ctypes.data, codes.size, q.ctypes.data, q.size, lines.ctypes.data) == 0
    assert list(lines) == [5, 6, 3, 4, 0]                                               # a repeated line keeps the latest number
    mc, ml = fm.latest_lines(codes)
    assert dict(zip(mc.tolist(), ml.tolist())) == {int(c): int(l) for c, l in zip(q[:4], lines[:4])}
    # the writer gives back the canonical text
    err = ctypes.create_string_buffer(512)
    assert host.h10x_host_whitelist_write(os.fsencode(str(tmp_path / "out.txt")), codes.ctypes.data, codes.size, err, 512) == 0
    assert (tmp_path / "out.txt").read_text() == fm.text(codes)
    # a 15-letter word: the message of fq2b-amd / the reference, with the line number
    (tmp_path / "bad.txt").write_text("ACGTACGTACGTACGT\nACGTACGTACGTACG\n")
    codes, msg = _read(host, tmp_path / "bad.txt")
    assert codes is None and msg == b"bad barcode line 2 in %s: ACGTACGTACGTACG" % os.fsencode(str(tmp_path / "bad.txt"))
    codes, msg = _read(host, tmp_path / "nosuch.txt")
    assert codes is None and msg == b"failed to open 10x whitelist file %s\n" % os.fsencode(str(tmp_path / "nosuch.txt"))
    (tmp_path / "empty.txt").write_text("")
    codes, msg = _read(host, tmp_path / "empty.txt")
    assert codes is not None and codes.size == 0


def test_usage_lists_the_commands(host):
    r = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0
    for line in (b"   --codeCensus <thresh> <fqb from fq2b> <goodcodes output>", b"   --fixFQB <goodcodes> <fqb from fq2b> <fixed fqb output>",
                 b"   --fixFQBThresh <thresh> <fqb from fq2b> <fixed fqb output>"):
        assert line in r.stderr
