"""The bookkeeping around the big kernels of a step (readFQB -> hashDepthRange -> cluster): counters drawn from the context's zeroed arena or zeroed by the
kernel that produces them, the reductions folded into the small kernels that already walk the arrays, the fused depth filter, and a --hashDepthRange that
leaves its three figures on the device until a command asks for them. Every case compares the canonical .hash bytes (and within[] where named) with the
CPU oracle on small generated sets. Needs a real MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

LO, HI, CT = 2, 30, 2


def _gen(tmp, name, pairs, barcodes, genome=20000, seed=7, err=0.003, mol=4.0, mol_len=6000):
    return orc.gen_fqb(os.path.join(str(tmp), name + ".fqb"), pairs, barcodes, genome, err, seed, mol, 150, mol_len).reshape(-1)


def _finish(x, tmp, name, ranges=((LO, HI),), cluster=True, ct=CT):
    for lo, hi in ranges:
        x.depth_range(lo, hi)
    if cluster:
        x.cluster(1, 0, ct)
    p = os.path.join(str(tmp), name)
    x.write_hash(p)
    with open(p, "rb") as f:
        b = f.read()
    os.remove(p)
    return b


def _oracle(recs, tmp, k=21, w=31, B=20, **kw):
    o = orc.Oracle(k, w, 17, B)
    o.read_fqb(recs)
    b = _finish(o, tmp, "orc.hash", **kw)
    o.close()
    return b


def _hip(B=20, k=21, w=31, **opts):
    import hash10x_amd
    h = hash10x_amd.Hash10x(k=k, w=w, r=17, B=B)
    for n, v in opts.items():
        h.set_option(n, v)
    return h


def _same(got, exp):
    assert got == exp, orc.describe_diff(got, exp)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """the generated sets the cases share, with the oracle's bytes of the plain step, made once"""
    tmp = tmp_path_factory.mktemp("bookkeeping")
    big = _gen(tmp, "a", 2400, 40, seed=11)             # 40 barcodes x 60 pairs
    small = _gen(tmp, "b", 15, 3, seed=12)              # 3 barcodes x 5 pairs
    mixed = _gen(tmp, "m", 600, 40, seed=13)            # 15 pairs a barcode on average: blocks on both sides of a 256-slot table
    r = big.reshape(-1, 30)                             # the barcodes of `big` with more than 25 read pairs: none fits a 256-slot table
    starts = np.flatnonzero(np.r_[True, r[1:, 0] != r[:-1, 0]])
    ends = np.r_[starts[1:], len(r)]
    large = r[np.concatenate([np.arange(a, b) for a, b in zip(starts, ends) if b - a > 25])].reshape(-1)
    return {"tmp": tmp, "big": big, "small": small, "mixed": mixed, "large": large,
            "big_exp": _oracle(big, tmp), "small_exp": _oracle(small, tmp), "mixed_exp": _oracle(mixed, tmp), "large_exp": _oracle(large, tmp)}


# ---------------------------------------------------------------------------------------------- stale state
def test_three_steps_on_one_context(sets):
    h = _hip()
    for name in ("big", "small", "big"):
        h.read_fqb(sets[name])
        _same(_finish(h, sets["tmp"], "hip.hash"), sets[name + "_exp"])
    h.close()


def test_steps_around_a_failing_command(sets):
    """a command that dies half-way (more distinct hashes than -B 20 allows) leaves nothing behind that the next steps of the context could see"""
    import hash10x_amd
    toobig = _gen(sets["tmp"], "toobig", 200000, 100, genome=3000000, seed=5, err=0.02)
    h = _hip()
    h.read_fqb(sets["big"])
    _same(_finish(h, sets["tmp"], "hip.hash"), sets["big_exp"])
    with pytest.raises(hash10x_amd.Hash10xError, match="hashTableSize is too small"):
        h.read_fqb(toobig)
    with pytest.raises(hash10x_amd.Hash10xError):
        h.depth_range(LO, HI)                           # no state
    for name in ("small", "big"):
        h.read_fqb(sets[name])
        _same(_finish(h, sets["tmp"], "hip.hash"), sets[name + "_exp"])
    h.close()


# ---------------------------------------------------------------------------------------------- edges of the counters and the folded reductions
def test_empty_input(sets):
    empty = np.zeros(0, dtype=np.uint32)
    h = _hip()
    h.read_fqb(empty)
    _same(_finish(h, sets["tmp"], "hip.hash"), _oracle(empty, sets["tmp"]))
    h.read_fqb(sets["small"])                           # and a real set behind it on the same context
    _same(_finish(h, sets["tmp"], "hip.hash"), sets["small_exp"])
    h.close()


def test_one_barcode(sets):
    recs = _gen(sets["tmp"], "one", 30, 1, seed=21)
    h = _hip()
    h.read_fqb(recs)
    assert h.sizes()["nBlocks"] == 2
    _same(_finish(h, sets["tmp"], "hip.hash"), _oracle(recs, sets["tmp"]))
    h.close()


def _tiny():
    return np.fromfile(os.path.join(orc.GOLDEN, "tiny.fqb"), dtype=np.uint32)


@pytest.mark.parametrize("slots", [0, 256], ids=["lds", "fallback"])
def test_block_without_any_mosh(sets, slots):
    """tiny.fqb: barcode 2 is one read pair without a mosh — its block is the {hash 0, read 0} entry (on the LDS path and on the global one)"""
    recs = _tiny()
    h = _hip(stage_a_max_slots=slots)
    h.read_fqb(recs)
    b = h.export_blocks()
    assert b["nHash"][2] == 1
    _same(_finish(h, sets["tmp"], "hip.hash", ranges=((1, 14),), ct=1), _oracle(recs, sets["tmp"], ranges=((1, 14),), ct=1))
    h.close()


@pytest.mark.parametrize("slots", [0, 256], ids=["lds", "fallback"])
def test_block_of_poly_a_pairs_only(sets, slots):
    """a barcode of three A-only read pairs right behind tiny.fqb's barcode without a mosh: its block has one distinct hash, VALUE 0, which is also what the
    stand-in entry of the block without a mosh holds — the two blocks share one hash index >= 1 (the oracle says so; the bytes must agree)"""
    recs = _tiny().reshape(-1, 30)
    codes = np.unique(recs[:, 0])
    assert int(codes[1]) + 1 < int(codes[2])                    # room for a new barcode right behind barcode 2
    new = np.stack([orc.make_record(int(codes[1]) + 1, np.zeros(135, np.uint32), np.zeros(151, np.uint32))] * 3)
    at = int(np.searchsorted(recs[:, 0], codes[1], side="right"))
    recs = np.concatenate([recs[:at], new, recs[at:]]).reshape(-1)
    h = _hip(stage_a_max_slots=slots)
    h.read_fqb(recs)
    b = h.export_blocks()
    assert b["nHash"][2] == 1 and b["nHash"][3] == 1
    o = orc.Oracle(21, 31, 17, 20)
    o.read_fqb(recs)
    ix = [int(o.clushash(c).copy()["hash"][0]) for c in (2, 3)]
    assert ix[0] == ix[1] >= 1 and int(o.hash_value()[ix[0]]) == 0 and int(o.hash_depth()[0][ix[0]]) >= 2
    o.close()
    _same(_finish(h, sets["tmp"], "hip.hash", ranges=((1, 14),), ct=1), _oracle(recs, sets["tmp"], ranges=((1, 14),), ct=1))
    h.close()


def test_some_blocks_on_the_fallback_path(sets):
    """a 256-slot table holds 25 read pairs: the larger blocks take the global path (a fallback table, repaired counts), the others stay"""
    h = _hip(stage_a_max_slots=256)
    h.read_fqb(sets["mixed"])
    fb, nb = h.counters()["fallback_blocks"], h.sizes()["nBlocks"]
    assert 0 < fb < nb - 2, (fb, nb)
    o = orc.Oracle(21, 31, 17, 20)
    o.read_fqb(sets["mixed"])
    ob, _, mx = o.blocks()
    assert np.array_equal(h.export_blocks()["nHash"][1:nb], ob["nHash"][1:mx])
    o.close()
    _same(_finish(h, sets["tmp"], "hip.hash"), sets["mixed_exp"])
    h.read_fqb(sets["large"])                           # the next step of the context: every hashed block on the fallback path
    assert h.counters()["fallback_blocks"] == h.sizes()["nBlocks"] - 2
    _same(_finish(h, sets["tmp"], "hip.hash"), sets["large_exp"])
    h.close()


# ---------------------------------------------------------------------------------------------- depth filter
def _within(depth, n, ranges):
    d = depth[:n].astype(np.int64)
    w = np.zeros(n, dtype=np.uint8)
    for lo, hi in ranges:
        w |= ((d >= lo) & (d < hi)).astype(np.uint8)
    return w


@pytest.mark.parametrize("ranges", [((2, 5), (8, 30)), ((2, 30), (2, 30)), ((8, 30), (2, 5), (8, 30)), ((5000, 6000),), ((5000, 6000), (2, 30))],
                         ids=["a_then_b", "same_twice", "a_b_a", "no_hash_in_it", "empty_then_real"])
def test_depth_ranges_accumulate(sets, ranges):
    h = _hip()
    h.read_fqb(sets["big"])
    got = _finish(h, sets["tmp"], "hip.hash", ranges=ranges)
    o = orc.Oracle(21, 31, 17, 20)
    o.read_fqb(sets["big"])
    depth, _, _ = o.hash_depth()
    n = o.hash_number
    exp_within = _within(np.array(depth), n, ranges)
    o.close()
    w = h.export_within()
    assert np.array_equal(w[1:], exp_within[1:n])
    _same(got, _oracle(sets["big"], sets["tmp"], ranges=ranges))
    h.close()


def test_device_wide_sort_path_of_the_good_lists(sets):
    """one barcode with more entries than a workgroup sorts (8192), beside small ones: the good lists take the key kernel, the 32-bit offsets and the
    segmented sort"""
    a = _gen(sets["tmp"], "s1", 300, 10, seed=31)
    one = _gen(sets["tmp"], "s2", 2500, 1, seed=32, genome=2000000, mol=30.0, mol_len=20000)
    c = _gen(sets["tmp"], "s3", 300, 10, seed=33)
    recs = np.concatenate([a, one, c])
    h = _hip()
    h.read_fqb(recs)
    assert h.export_blocks()["nHash"].max() > 8192
    _same(_finish(h, sets["tmp"], "hip.hash", ranges=((1, 30),)), _oracle(recs, sets["tmp"], ranges=((1, 30),)))
    h.close()


# ---------------------------------------------------------------------------------------------- index build: runs of equal hashes
def _index_only(recs, tmp, k=21, w=31, **opts):
    h = _hip(k=k, w=w, **opts)
    h.read_fqb(recs)
    got = _finish(h, tmp, "hip.hash", ranges=(), cluster=False)
    h.close()
    _same(got, _oracle(recs, tmp, k=k, w=w, ranges=(), cluster=False))


@pytest.fixture(scope="module")
def sweep(sets):
    """40 sets from a few entries to some 20 000 with the oracle's bytes of the index, made once for both forms of the entries"""
    out = []
    for i in range(40):
        pairs = 2 + (i * i * 3000) // (39 * 39)
        recs = _gen(sets["tmp"], "sw", pairs, 2 + i // 2, seed=100 + i, genome=200000, mol=8.0, mol_len=20000)
        out.append((recs, _oracle(recs, sets["tmp"], ranges=(), cluster=False)))
    return out


@pytest.mark.parametrize("opts", [{"index_rank_fused": 1}, {"index_rank_fused": 2}, {"index_no_pack": 1}], ids=["packed_fused", "packed_two_kernels", "unpacked"])
def test_sweep_of_entry_counts(sets, sweep, opts):
    """every tile edge of the scan over the sorted entries is crossed, on one context (each set also meets what the one before left)"""
    h = _hip(**opts)
    for recs, exp in sweep:
        h.read_fqb(recs)
        _same(_finish(h, sets["tmp"], "hip.hash", ranges=(), cluster=False), exp)
    h.close()


def test_key_and_block_number_do_not_fit_one_word(sets):
    recs = _gen(sets["tmp"], "k31", 600, 20, seed=41)
    _index_only(recs, sets["tmp"], k=31, w=5)


@pytest.mark.parametrize("fused", [1, 2], ids=["fused", "two_kernels"])
def test_single_run_and_all_distinct(sets, fused):
    tiny = _tiny().reshape(-1, 30)
    nomosh = tiny[3].copy()
    single = np.stack([nomosh] * 7)
    single[:, 0] = 0x10000000 + np.arange(7, dtype=np.uint32) * 0x01010101      # seven barcodes, each the {hash 0, read 0} entry: one run
    _index_only(single.reshape(-1), sets["tmp"], index_rank_fused=fused)
    distinct = _gen(sets["tmp"], "d", 40, 2, seed=51)   # one hashed barcode (the file's last is not): every hash once, the last entry a run of its own
    _index_only(distinct, sets["tmp"], index_rank_fused=fused)


@pytest.fixture(scope="module")
def at_the_bound(sets):
    """Two sets for -B 20, which admits 2^18 - 3 distinct hashes (hashNumber ends at U + 1 and must not exceed 2^18 - 2: hash10x.c:149): one with exactly that many,
    one with one more. Built from a set of tiny barcodes: as many leading barcodes as stay at or under the target, then ONE later barcode whose hashes make up the
    difference, then the file's last barcode (never hashed). The counts that steer the search are taken on the GPU; what the two sets must do is the oracle's word."""
    r = _gen(sets["tmp"], "edge", 60000, 30000, genome=3000000, seed=5, err=0.02).reshape(-1, 30)
    starts = np.flatnonzero(np.r_[True, r[1:, 0] != r[:-1, 0]])
    ends = np.r_[starts[1:], len(r)]
    last = r[starts[-1]:]
    target = (1 << 18) - 3
    import hash10x_amd
    h = _hip(B=21)                                          # (a table that admits them all: the search wants counts on both sides of the target)

    def count(*parts):
        recs = np.concatenate(parts + (last,)).reshape(-1)
        try:
            h.read_fqb(recs)
        except hash10x_amd.Hash10xError as e:               # beyond the bound: how far is not needed then
            assert "hashTableSize is too small" in str(e)
            return target + (1 << 20), recs
        return h.sizes()["hashNumber"] - 1, recs

    lo, hi = 1, len(starts) - 1                             # the largest K whose first K barcodes hold at most `target` hashes
    assert count(r[:ends[hi - 1]])[0] > target + 64
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(r[:ends[mid - 1]])[0] <= target:
            lo = mid
        else:
            hi = mid - 1
    K = lo
    base, _ = count(r[:ends[K - 1]])
    found = {}
    if base == target:
        found[0] = count(r[:ends[K - 1]])[1]
    for j in range(K + 1, min(K + 400, len(starts) - 1)):   # (barcode K itself overshoots)
        if 0 in found and 1 in found:
            break
        n, recs = count(r[:ends[K - 1]], r[starts[j]:ends[j]])
        if n - target in (0, 1) and n - target not in found:
            found[n - target] = recs
    h.close()
    assert 0 in found and 1 in found, (base, target, sorted(found))
    return found


@pytest.mark.parametrize("fused", [1, 2], ids=["fused", "two_kernels"])
def test_distinct_hashes_at_and_beyond_the_table_bound(sets, at_the_bound, fused):
    import hash10x_amd
    h = _hip(index_rank_fused=fused)
    h.read_fqb(at_the_bound[0])
    assert h.sizes()["hashNumber"] == (1 << 18) - 2
    got = _finish(h, sets["tmp"], "hip.hash", ranges=(), cluster=False)
    with pytest.raises(hash10x_amd.Hash10xError, match="hashTableSize is too small"):
        h.read_fqb(at_the_bound[1])                         # one hash more: the bound clamps what is written, the check fails the command
    h.read_fqb(at_the_bound[0])                             # and the context is as good as new
    _same(_finish(h, sets["tmp"], "hip.hash", ranges=(), cluster=False), got)
    h.close()
    _same(got, _oracle(at_the_bound[0], sets["tmp"], ranges=(), cluster=False))
    with pytest.raises(orc.OracleError, match="hashTableSize is too small"):
        _oracle(at_the_bound[1], sets["tmp"], ranges=(), cluster=False)


# ---------------------------------------------------------------------------------------------- the figures that stay on the device
def test_cluster_without_a_range_is_refused(sets):
    import hash10x_amd
    h = _hip()
    h.read_fqb(sets["small"])
    with pytest.raises(hash10x_amd.Hash10xError, match="!! you must set hashDepthRange before cluster"):
        h.cluster(1, 0, CT)
    h.close()


def test_commands_between_range_and_cluster(sets):
    exp = sets["big_exp"]
    h = _hip()
    h.read_fqb(sets["big"])
    h.depth_range(LO, HI)
    rows = h.share_graph(2)                             # reads the good lists; the figures are still on the device
    h.cluster(1, 0, CT)
    p = os.path.join(str(sets["tmp"]), "hip.hash")
    h.write_hash(p)
    _same(open(p, "rb").read(), exp)
    h.cluster(1, 0, CT)                                 # a second cluster command: the figures are cached by now
    h.write_hash(p)
    second = open(p, "rb").read()
    h.close()
    g = _hip()
    g.read_fqb(sets["big"])
    g.depth_range(LO, HI)
    g.cluster(1, 0, CT)
    g.cluster(1, 0, CT)
    g.write_hash(p)
    _same(second, open(p, "rb").read())
    rows2 = g.share_graph(2)
    g.close()
    os.remove(p)
    for a, b in zip(rows, rows2):                       # (offsets, block, count)
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_new_range_replaces_the_figures(sets):
    """a wide range, clustered; then a range that holds a few shallow hashes only: the second cluster runs on the second range's figures"""
    h = _hip()
    h.read_fqb(sets["big"])
    _finish(h, sets["tmp"], "hip.hash", ranges=((2, 40),))
    h.read_fqb(sets["big"])
    _same(_finish(h, sets["tmp"], "hip.hash", ranges=((2, 4),)), _oracle(sets["big"], sets["tmp"], ranges=((2, 4),)))
    h.close()


def test_sharded_single_rank(sets):
    import hash10x_amd
    comms = hash10x_amd.Comm.local(1)
    try:
        h = _hip()
        h.shard_read_fqb(comms[0], sets["big"])
        _same(_finish(h, sets["tmp"], "hip.hash"), sets["big_exp"])
        h.close()
    finally:
        for c in comms:
            c.destroy()
