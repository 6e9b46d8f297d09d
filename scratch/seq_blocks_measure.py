"""the rows of sequences at T = 5 on the molecule state of the yeast-like workload (after --cluster 1 0 --clusterSplit and the range
again). The sequences are the generator's two haplotypes cut into 20 kb pieces. Two ways in one process, in alternation: (a) the host route,
Hash10x.mosh_set over the range, MoshSet.scan plus lookup of every piece back to the host, and a join in numpy against the exported clushash (the barcode
lists on the host, exported once and not timed); (b) Hash10x.seq_blocks(pieces, 5). Call times by the host clock around calls that end in a synchronise,
six rounds, the first dropped. SB_UNDER_PROF=1 (for a run under rocprofv3 --kernel-trace --stats): three rounds of (b) only. The records come from
build/gen_fqb with the workload's parameters and seed 1 (it writes the haplotypes beside them) and are checked against bench.generate's."""
import json, os, subprocess, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench, hash10x_amd

T, PIECE = 5, 20000
PROF = bool(os.environ.get("SB_UNDER_PROF"))
wl = bench.WORKLOADS["yeast-like-2.5M"]
tmp = tempfile.mkdtemp(prefix="sb_measure_")
fqb, fa = os.path.join(tmp, "x.fqb"), os.path.join(tmp, "x")
subprocess.run([os.path.join(REPO, "build", "gen_fqb"), "-o", fqb, "-P", str(wl["pairs"]), "-C", str(wl["barcodes"]), "-G", str(wl["genome"]), "-e", str(wl["err"]),
                "-s", "1", "-m", str(wl["mol"]), "-S", str(wl["snp"]), "-L", str(wl["mol_len"]), "-fa", fa], check=True, stderr=subprocess.DEVNULL)
recs = np.fromfile(fqb, dtype=np.uint32)
same_records = bool(np.array_equal(recs, bench.generate(wl, seed=1)))
pairs = recs.size // 30


def haplotype(path):
    text = b"".join(ln.strip() for ln in open(path, "rb") if not ln.startswith(b">"))
    return hash10x_amd.Hash10x._flatten_seqs([text])[0]


pieces = []
for name in (fa + ".A.fa", fa + ".B.fa"):
    codes = haplotype(name)
    pieces += [codes[a:a + PIECE] for a in range(0, len(codes), PIECE)]
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs)
h.depth_range(wl["lo"], wl["hi"]); h.cluster(1, 0, wl["ct"]); h.cluster_split(); h.depth_range(wl["lo"], wl["hi"])
hash10x_amd.synchronize(0)
for f in (fqb, fa + ".A.fa", fa + ".B.fa"):
    os.remove(f)
os.rmdir(tmp)
nb, U1 = h.sizes()["nBlocks"], h.sizes()["hashNumber"]
codes_all, starts = hash10x_amd.Hash10x._flatten_seqs(pieces)

res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (gen_fqb seed 1 with its haplotypes), after --cluster 1 0 --clusterSplit, range again",
       "records_equal_bench_generate": same_records, "pairs": pairs, "nBlocks": nb, "hashNumber": U1, "T": T, "pieces": len(pieces), "bases": int(len(codes_all)),
       "host_route_ms": [], "seq_blocks_ms": []}

if not PROF:
    # the barcode lists on the host, once (not timed: the host route holds them): the records sorted by hash, block ascending inside
    n_hash = h.export_blocks()["nHash"].astype(np.int64)
    hashes = h.export_clushash()["hash"].astype(np.int64)
    blk_of = np.repeat(np.arange(nb, dtype=np.int64), n_hash)
    order = np.lexsort((blk_of, hashes))
    hs, bs = hashes[order], blk_of[order]
    start = np.searchsorted(hs, np.arange(U1 + 1))
    within = h.export_within().astype(bool); within[0] = False
    kept = np.flatnonzero(within)                              # set index k (from 1) is state index kept[k - 1]


def host_route():
    """(offsets, block, count) the host's way"""
    ms = h.mosh_set(wl["lo"], wl["lo"] + 1, wl["hi"])
    hv, sq, _ = ms.scan(codes_all, starts)
    ix, _ = ms.lookup(hv)
    ms.close()
    hit = ix > 0
    q = np.unique(sq[hit].astype(np.int64) * U1 + kept[ix[hit].astype(np.int64) - 1])      # Q(s): distinct (sequence, state index)
    qs, qx = q // U1, q % U1
    n = start[qx + 1] - start[qx]
    at = np.repeat(start[qx] - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
    key, cnt = np.unique(np.repeat(qs, n) * nb + bs[at], return_counts=True)
    keep = cnt >= T
    rows_of = np.bincount(key[keep] // nb, minlength=len(pieces))
    return np.concatenate([[0], np.cumsum(rows_of)]).astype(np.uint64), (key[keep] % nb).astype(np.uint32), cnt[keep].astype(np.uint32)


for rep in range(3 if PROF else 6):
    if not PROF:
        t0 = time.perf_counter()
        a = host_route()
        res["host_route_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    t0 = time.perf_counter()
    b = h.seq_blocks(pieces, T)
    res["seq_blocks_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        res["info"] = dict(h.seq_blocks_info)
        fig = b[3]
        res["figures"] = {k: int(fig[k].sum()) for k in ("moshes", "found", "query", "entries")}
        if not PROF:
            res["equal"] = bool(all(np.array_equal(x, y) for x, y in zip(a, b[:3])))
            # the algorithmic bytes of the look-up and the gather: 12 B read and 8 B written per occurrence plus one probe of 4 + 8 + 1 B at least;
            # 4 B per list entry read and K B per key written (K from the run's key width)
            K = 8 if res["info"]["wideBatches"] else 4
            res["lookup_kernel_bytes"] = {"read": 12 * res["figures"]["moshes"], "probes_at_least": 13 * res["figures"]["moshes"], "written": 8 * res["figures"]["moshes"]}
            res["gather_kernel_bytes"] = {"lists": 4 * res["info"]["listEntries"], "keys": K * res["info"]["listEntries"], "units": 28 * res["info"]["listHashes"]}
if not PROF:
    for k in ("host_route_ms", "seq_blocks_ms"):
        v = res[k][1:]
        res[k + "_median_min_max"] = [round(float(np.median(v)), 3), min(v), max(v)]
print(json.dumps(res))
