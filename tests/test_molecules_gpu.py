"""--moleculeMap and --splitFQB on the GPU (csrc/stage_k.hip) against the numpy model of tests/mol_model.py over .hash files the
reference wrote: the goldens, fresh runs of oracle/_ref/hash10x, and hand-built states at the shapes where the numbering can go wrong."""
import os
import subprocess

import numpy as np
import pytest

import mol_model
import orc

pytestmark = pytest.mark.gpu
EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
needs_ref = pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built (needs the reference's sources)")
FORMS = [pytest.param(0, id="lds"), pytest.param(1, id="global")]


def golden_bytes(name):
    return orc.read_maybe_gz(os.path.join(orc.GOLDEN, name))


def golden_records(name):
    return np.frombuffer(golden_bytes(name), dtype=np.uint32).reshape(-1, 30)


def fake_records(model, seed=3):
    """records nobody hashed: a distinct non-zero barcode word per block, the record's own number in word 1, noise behind it"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 1 << 32, size=(max(model.R, 1), 30), dtype=np.uint64).astype(np.uint32)[:model.R]
    block = np.repeat(np.arange(model.n_codes), np.diff(model.base))
    r[:, 0] = (block * 2654435761 + 12345) % (1 << 32) | 1
    r[:, 1] = np.arange(model.R)
    return r


def check_map_and_split(h, model, records, device=False):
    import hash10x_amd
    mol, slot, info = h.molecule_map()
    assert info == model.info
    bad = np.flatnonzero((mol != model.mol) | (slot != model.slot))
    assert bad.size == 0, "record %d: mol %d slot %d, model %d %d (%d differ)" % (bad[0], mol[bad[0]], slot[bad[0]], model.mol[bad[0]], model.slot[bad[0]], bad.size)
    if records is None:
        return None
    if device:
        d = hash10x_amd.DeviceRecords(records[:model.R])
        out_d, start = h.split_fqb(d)
        out = out_d.download()
        d.free(); out_d.free()
    else:
        out, start = h.split_fqb(records[:model.R])
    assert np.array_equal(start, model.start)
    assert np.array_equal(out, model.split(records))
    return out


# ------------------------------------------------------------------------------------------ 1, 2: the goldens
def test_golden_through_read_fqb(tmp_path):
    import hash10x_amd
    recs = golden_records("small.fqb.gz")
    model = mol_model.load("small.c_3_14_2.hash.gz")
    h = hash10x_amd.Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(3, 14)
    h.cluster(1, 0, 2)
    out = check_map_and_split(h, model, recs)
    h.cluster_split()
    h.write_hash(str(tmp_path / "split.hash"))
    h.close()
    got = (tmp_path / "split.hash").read_bytes()
    gold = golden_bytes("small.split.hash.gz")
    assert got == gold, orc.describe_diff(got, gold)
    sp = orc.HashFile(got)
    model.check_against_split(sp)
    mol_model.split_refs(model, sp, out, recs)               # ClusterHash (hash, read r) of block m is record start[m] + r


@pytest.mark.parametrize("name,fqb", [("small.c_3_14_2", "small.fqb.gz"), ("small.accum", "small.fqb.gz"), ("tiny.c", "tiny.fqb"), ("abort255.out", None)])
def test_golden_through_read_hash(workdir, name, fqb):
    import hash10x_amd
    model = mol_model.load(name + ".hash.gz")
    recs = golden_records(fqb) if fqb else fake_records(model)
    assert len(recs) >= model.R
    h = hash10x_amd.Hash10x(B=20)
    h.read_hash(workdir.need(name + ".hash.gz"))
    out = check_map_and_split(h, model, recs)
    if model.M == 0:
        assert np.array_equal(out, recs[:model.R])           # identity
    h.cluster_split()
    h.write_hash(workdir.file("split.hash"))
    h.close()
    sp = orc.HashFile(open(workdir.file("split.hash"), "rb").read())
    model.check_against_split(sp)
    mol_model.split_refs(model, sp, out, recs)
    if name == "small.c_3_14_2":
        assert open(workdir.file("split.hash"), "rb").read() == golden_bytes("small.split.hash.gz")


# ------------------------------------------------------------------------------------------ 3: hand-built states
def hash_bytes(blocks, B=20):
    """a .hash v2 image (hash10x.c:244-267) from [(nRead, nSubCluster, clusterParent, [(read, subCluster), ...]), ...] for blocks 1 ..:
    the record at position p of a block holds hash index p + 1, so hashDepth[h] = the blocks with at least h records.
    (Not orc.hash_image: that one takes the hash indices of each block; this one sets each record's read and label and the block's header fields.)"""
    n_blocks = len(blocks) + 1
    longest = max([len(b[3]) for b in blocks] + [0])
    hash_number = longest + 1
    depth = np.zeros(hash_number, dtype="<u4")
    blk = np.zeros(n_blocks, dtype=orc.BLOCK)
    parts = []
    for i, (n_read, n_sub, parent, ents) in enumerate(blocks, start=1):
        blk[i] = (n_read, len(ents), n_sub, parent, 0, 0.0)
        ch = np.zeros(len(ents), dtype=orc.CLUSHASH)
        if ents:
            e = np.asarray(ents, dtype=np.int64).reshape(-1, 2)
            ch["hash"] = np.arange(1, len(ents) + 1); ch["read"] = e[:, 0]; ch["subCluster"] = e[:, 1]
            depth[1:len(ents) + 1] += 1
        parts.append(ch.tobytes())
    hdr = np.zeros(1, dtype="<i4,<i4,<u8,<i4,<i4,<i4,<i4")
    out = [b"10XH", (2).to_bytes(4, "little"), (8).to_bytes(2, "little"), (32).to_bytes(2, "little"), B.to_bytes(4, "little"),
           bytes(4 << B), hash_number.to_bytes(4, "little"), (np.arange(hash_number, dtype="<u8") * 31).tobytes()]
    hdr[0] = (8918274, 0, 0, hash_number, 4, hash_number, 0); out += [hdr.tobytes(), depth.tobytes()]
    hdr[0] = (8918274, 0, 0, n_blocks, 32, n_blocks, 0); out += [hdr.tobytes(), blk.tobytes()]
    return b"".join(out + parts)


def edge_blocks():
    rng = np.random.default_rng(11)
    blocks = []
    # 200 records, all label 1, each from a read of its own, reads descending: the rank carries over 64-lane steps, slot order is not read order
    blocks.append((200, 1, 0, [(199 - p, 1) for p in range(200)]))
    # labels 1 and 255 in one block of 300 reads, in shuffled order, every read twice
    order = rng.permutation(300).tolist()
    blocks.append((300, 255, 0, [(r, 1 if r % 3 else 255) for r in order] + [(r, 1 if r % 3 else 255) for r in order[::-1]]))
    # 65 reads of one label whose first clustered records lie in positions 40 .. 104: one 64-position step and the next; repeats behind
    blocks.append((90, 2, 0, [(70 + (p % 20), 0) for p in range(40)] + [(64 - k, 2) for k in range(65)] + [(k, 2) for k in range(65)] + [(80, 1), (3, 2)]))
    # a read whose first record is unclustered and a later one clustered (read 5); a label above nSubCluster (read 6: unclustered); a read beyond the block
    blocks.append((8, 3, 0, [(5, 0), (1, 3), (6, 4), (5, 3), (0, 1), (6, 200), (2, 0), (1, 3), (7, 1), (5, 3), (9, 1)]))
    blocks.append((37, 0, 0, [(p % 37, 0) for p in range(50)]))                    # no clusters
    blocks.append((5, 0, 0, []))                                                   # records, no hashes
    # the threshold between the LDS table and the scratch slice: 2048 and 2049 reads, the last read clustered
    for n in (2048, 2049):
        ents = [(int(r), 1 + int(r) % 7) for r in rng.integers(0, n, size=3000)] + [(n - 1, 7), (0, 7)]
        blocks.append((n, 7, 0, ents))
    blocks.append((3, 1, 0, [(2, 1), (0, 1), (2, 1)]))
    return blocks


@pytest.fixture(scope="module")
def edges():
    data = hash_bytes(edge_blocks())
    model = mol_model.MolModel(orc.HashFile(data))
    return data, model, fake_records(model)


def load_bytes(h, tmp_path, data):
    p = tmp_path / "state.hash"
    p.write_bytes(data)
    h.read_hash(str(p))


@pytest.mark.parametrize("form", FORMS)
def test_hand_built_blocks(tmp_path, edges, form):
    import hash10x_amd
    data, model, recs = edges
    # the model itself on the shapes it is trusted for here, by hand: block 1's slots are the positions of its reads, read 5 of block 4 is
    # clustered with label 3 behind read 1, reads 6 and 2 of block 4 stay
    assert np.array_equal(model.slot[:200], np.arange(199, -1, -1)) and (model.mol[:200] == model.n_codes).all()
    b4 = int(model.base[4])
    ext4 = model.n_codes - 1 + int(model.sub_before[4])
    assert model.mol[b4 + 5] == ext4 + 3 and model.slot[b4 + 5] == 1 and model.mol[b4 + 1] == ext4 + 3 and model.slot[b4 + 1] == 0
    assert model.mol[b4 + 6] == 4 and model.mol[b4 + 2] == 4 and model.mol[b4 + 0] == ext4 + 1 and model.mol[b4 + 7] == ext4 + 1 and model.slot[b4 + 7] == 1
    h = hash10x_amd.Hash10x(B=20)
    h.set_option("molmap_global", form)
    load_bytes(h, tmp_path, data)
    check_map_and_split(h, model, recs, device=bool(form))
    h.close()


@pytest.mark.parametrize("form", FORMS)
def test_block_of_65536_reads(tmp_path, form):
    import hash10x_amd
    data = hash_bytes([(65536, 2, 0, [(65535, 2), (0, 1), (65535, 2), (40000, 2), (1, 0)]), (3, 0, 0, [])])
    model = mol_model.MolModel(orc.HashFile(data))
    assert model.n_clustered == 3 and model.mol[65535] == 2 + 2 and model.slot[65535] == 0 and model.slot[40000] == 1
    h = hash10x_amd.Hash10x(B=20)
    h.set_option("molmap_global", form)
    load_bytes(h, tmp_path, data)
    check_map_and_split(h, model, None)
    h.close()


def test_refusals_of_states(tmp_path):
    import hash10x_amd
    h = hash10x_amd.Hash10x(B=20)
    with pytest.raises(hash10x_amd.Hash10xError, match="no hash state loaded"):
        h.molecule_map()
    load_bytes(h, tmp_path, hash_bytes([(4, 0, 0, []), (65537, 1, 0, [(65535, 1)])]))
    with pytest.raises(hash10x_amd.Hash10xError, match="block 2 is clustered and holds more than 65536 read pairs"):
        h.molecule_map()
    with pytest.raises(hash10x_amd.Hash10xError, match="more than 65536 read pairs"):
        h.split_fqb(np.zeros((65541, 30), dtype=np.uint32))
    data = hash_bytes([(65537, 0, 0, [(1, 0)]), (2, 1, 0, [(1, 1)])])                 # unclustered: fine at any size
    load_bytes(h, tmp_path, data)
    check_map_and_split(h, mol_model.MolModel(orc.HashFile(data)), None)
    load_bytes(h, tmp_path, hash_bytes([(4, 1, 0, [(1, 1)]), (2, 0, 1, [(1, 0)])]))
    with pytest.raises(hash10x_amd.Hash10xError, match="block 2 was made by --clusterSplit"):
        h.molecule_map()
    h.close()


# ------------------------------------------------------------------------------------------ 4: the reference on fresh data
@pytest.fixture(scope="module", params=["mid.c", "dense.c"])
def fresh(request, tmp_path_factory, golden_manifest):
    case = [c for c in golden_manifest["digest_cases"] if c["name"] == request.param][0]
    d = str(tmp_path_factory.mktemp("mol_" + request.param.replace(".", "_")))
    recs = orc.gen_fqb(os.path.join(d, "x.fqb"), **case["gen"])
    args = orc.leading_options(case["args"])
    r = orc.run_ref(["-B", case["B"]] + args + ["--readFQB", "x.fqb"] + case["args"][len(args):] + ["--writeHash", "a.hash", "--clusterSplit", "--writeHash", "b.hash"], d)
    assert r.returncode == 0, r.stderr.decode()
    a = open(os.path.join(d, "a.hash"), "rb").read()
    assert orc.sha256(orc.canonical_hash_bytes(a)) == case["sha256"]                   # the recorded run of this case
    return {"dir": d, "case": case, "recs": recs, "model": mol_model.MolModel(orc.HashFile(a)), "split": orc.HashFile(open(os.path.join(d, "b.hash"), "rb").read())}


@needs_ref
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_fresh_against_reference(fresh, device):
    import hash10x_amd
    model, sp = fresh["model"], fresh["split"]
    assert model.R == len(fresh["recs"]) and model.M == fresh["case"]["sum_nSubCluster"]
    model.check_against_split(sp)
    h = hash10x_amd.Hash10x(B=fresh["case"]["B"])
    h.read_hash(os.path.join(fresh["dir"], "a.hash"))
    out = check_map_and_split(h, model, fresh["recs"], device=device)
    h.close()
    mol_model.split_refs(model, sp, out, fresh["recs"])


# ------------------------------------------------------------------------------------------ 5: refusals and checks
def test_refusals_of_records_and_contexts(workdir):
    import hash10x_amd
    recs = golden_records("small.fqb.gz")
    model = mol_model.load("small.c_3_14_2.hash.gz")
    h = hash10x_amd.Hash10x(B=20)
    h.read_hash(workdir.need("small.c_3_14_2.hash.gz"))
    swapped = recs.copy()
    a, b = int(model.base[3]), int(model.base[7])
    swapped[[a, b]] = swapped[[b, a]]                                                 # a record of block 3 and one of block 7 change places
    with pytest.raises(hash10x_amd.Hash10xError, match="is not the file this state was read from: block 3 holds more than one barcode"):
        h.split_fqb(swapped)
    with pytest.raises(hash10x_amd.Hash10xError, match="3999 records given, the state was read from 4000"):
        h.split_fqb(recs[:-1])
    with pytest.raises(hash10x_amd.Hash10xError, match="4001 records given"):
        h.split_fqb(np.concatenate([recs, recs[:1]]))
    h.cluster_split()
    with pytest.raises(hash10x_amd.Hash10xError, match="was made by --clusterSplit"):
        h.molecule_map()
    with pytest.raises(hash10x_amd.Hash10xError, match="was made by --clusterSplit"):
        h.split_fqb(recs)
    h.close()


def test_sharded_context_is_refused():
    import threading
    import hash10x_amd
    recs = golden_records("small.fqb.gz")
    cut = hash10x_amd.partition(recs, 2)
    comms = hash10x_amd.Comm.local(2)
    flat = np.ascontiguousarray(recs).reshape(-1)
    said = [[], []]

    def work(r):
        try:
            h = hash10x_amd.Hash10x(B=20)
            h.shard_read_fqb(comms[r], flat[30 * cut[r]: 30 * cut[r + 1]])
            h.depth_range(3, 14)
            h.cluster(1, 0, 2)
            for call in (h.molecule_map, lambda: h.split_fqb(recs)):
                try:
                    call()
                    said[r].append("not refused")
                except hash10x_amd.Hash10xError as e:
                    said[r].append(str(e))
            h.close()
        except Exception as e:              # noqa: BLE001
            said[r].append("failed: %r" % (e,))
    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    for c in comms:
        c.destroy()
    for s in said:
        assert len(s) == 2 and all(m.startswith("moleculeMap does not run on a sharded context") for m in s), s


# ------------------------------------------------------------------------------------------ 6: the command line
def run(args, cwd, stdin=None, limit=120):
    return subprocess.run([EXE] + [str(a) for a in args], cwd=str(cwd), input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=limit)


HEAD = ["-B", "20", "-ct", "2", "--readFQB", "small.fqb", "--hashDepthRange", "3", "14", "--cluster", "1", "0"]


@pytest.fixture(scope="module")
def small():
    model = mol_model.load("small.c_3_14_2.hash.gz")
    return model, golden_records("small.fqb.gz")


def check_cli_files(d, model, recs, mol="m.mol", fqb="s.fqb"):
    assert open(os.path.join(d, mol), "rb").read() == model.mol_bytes()
    assert open(os.path.join(d, fqb), "rb").read() == model.split(recs).tobytes()
    assert open(os.path.join(d, fqb + ".idx"), "rb").read() == model.idx_bytes()


def test_cli(workdir, small):
    import hash10x_amd
    model, recs = small
    workdir.need("small.fqb.gz")
    p = run(HEAD + ["--moleculeMap", "m.mol", "--splitFQB", "small.fqb", "s.fqb", "--clusterSplit", "--writeHash", "split.hash"], workdir.path)
    assert p.returncode == 0, p.stderr.decode()
    check_cli_files(workdir.path, model, recs)
    got = orc.canonical_hash_bytes(open(workdir.file("split.hash"), "rb").read())
    assert got == orc.canonical_hash_bytes(golden_bytes("small.split.hash.gz"))
    assert b"  mapped 4000 read pairs: 1391 in 88 molecules, 2609 unclustered, 40 barcodes\n" in p.stdout
    mol, slot, info = hash10x_amd.read_molecule_map(workdir.file("m.mol"))
    assert np.array_equal(mol, model.mol) and info == model.info
    assert np.array_equal(hash10x_amd.read_split_index(workdir.file("s.fqb.idx"))[0], model.start)


def test_cli_interactive(workdir, small):
    model, recs = small
    workdir.need("small.fqb.gz")
    script = b"readFQB small.fqb\nhashDepthRange 3 14\ncluster 1 0\nmoleculeMap i.mol\nsplitFQB small.fqb i.fqb\nquit\n"
    p = run(["-B", "20", "-ct", "2", "--interactive"], workdir.path, stdin=script)
    assert p.returncode == 0, p.stderr.decode()
    check_cli_files(workdir.path, model, recs, "i.mol", "i.fqb")
    assert b"  mapped 4000 read pairs: 1391 in 88 molecules" in p.stdout


def test_cli_refusals(workdir, small):
    model, recs = small
    workdir.need("small.fqb.gz")
    p = run(["--gpus", "2"] + HEAD + ["--moleculeMap", "g.mol"], workdir.path)
    assert p.returncode == 255 and b"FATAL ERROR: --moleculeMap does not run on a sharded session (--gpus 2)" in p.stderr
    p = run(["--gpus", "2"] + HEAD + ["--splitFQB", "small.fqb", "g.fqb"], workdir.path)
    assert p.returncode == 255 and b"FATAL ERROR: --splitFQB does not run on a sharded session (--gpus 2)" in p.stderr
    p = run(["-B", "20", "--moleculeMap", "n.mol"], workdir.path)
    assert p.returncode == 255 and b"FATAL ERROR: moleculeMap: no hash state loaded" in p.stderr
    p = run(HEAD + ["--clusterSplit", "--moleculeMap", "a.mol"], workdir.path)
    assert p.returncode == 255 and b"FATAL ERROR: moleculeMap: block 41 was made by --clusterSplit" in p.stderr
    for f in ("g.mol", "g.fqb", "n.mol", "a.mol"):
        assert not os.path.exists(workdir.file(f))


def test_cli_short_and_long_files(workdir, small):
    model, recs = small
    workdir.need("small.fqb.gz")
    recs[:-10].tofile(workdir.file("short.fqb"))
    np.concatenate([recs, recs[:10]]).tofile(workdir.file("long.fqb"))
    p = run(HEAD + ["--splitFQB", "short.fqb", "x.fqb"], workdir.path)
    assert p.returncode == 255 and b"FATAL ERROR: short.fqb holds 3990 records, the state was read from 4000" in p.stderr
    assert not os.path.exists(workdir.file("x.fqb"))
    p = run(HEAD + ["--moleculeMap", "m.mol", "--splitFQB", "long.fqb", "s.fqb"], workdir.path)
    assert p.returncode == 0, p.stderr.decode()
    assert b"  10 records beyond the 4000 the state was read from are left out\n" in p.stdout
    check_cli_files(workdir.path, model, recs)
