"""the per-hash linkage groups at T = 5 on the yeast-like workload after --cluster 1 0 --clusterSplit and the range again (the
molecules), with the crib of the generator's two haplotypes. Two ways in one process, in alternation: (a) the parent's way, Hash10x.share_graph(5) over
all blocks copied out to host arrays and a numpy union per hash there, over a random sample of SAMPLE in-range hashes (RandomState(18)); (b)
Hash10x.hash_copies(5) over the whole table. Call times by the host clock around calls that end in a synchronise. HC_UNDER_PROF=1 (for a run under
rocprofv3 --kernel-trace --stats): three rounds of (b) only. The records come from build/gen_fqb with the workload's parameters and seed 1 (it writes the
haplotypes beside them) and are checked against bench.generate's."""
import json, os, subprocess, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench, hash10x_amd

T, SAMPLE = 5, 2000
PROF = bool(os.environ.get("HC_UNDER_PROF"))
wl = bench.WORKLOADS["yeast-like-2.5M"]
tmp = tempfile.mkdtemp(prefix="hc_measure_")
fqb, fa = os.path.join(tmp, "x.fqb"), os.path.join(tmp, "x")
subprocess.run([os.path.join(REPO, "build", "gen_fqb"), "-o", fqb, "-P", str(wl["pairs"]), "-C", str(wl["barcodes"]), "-G", str(wl["genome"]), "-e", str(wl["err"]),
                "-s", "1", "-m", str(wl["mol"]), "-S", str(wl["snp"]), "-L", str(wl["mol_len"]), "-fa", fa], check=True, stderr=subprocess.DEVNULL)
recs = np.fromfile(fqb, dtype=np.uint32)
same_records = bool(np.array_equal(recs, bench.generate(wl, seed=1)))
pairs = recs.size // 30
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs); h.crib_build(fa + ".A.fa", fa + ".B.fa")
h.depth_range(wl["lo"], wl["hi"]); h.cluster(1, 0, wl["ct"]); h.cluster_split(); h.depth_range(wl["lo"], wl["hi"])
hash10x_amd.synchronize(0)
for f in (fqb, fa + ".A.fa", fa + ".B.fa"):
    os.remove(f)
os.rmdir(tmp)
nb = h.sizes()["nBlocks"]

res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (gen_fqb seed 1 with its haplotypes), after --cluster 1 0 --clusterSplit, range again",
       "records_equal_bench_generate": same_records, "pairs": pairs, "nBlocks": nb, "T": T, "sample": SAMPLE, "share_graph_copy_out_ms": [], "sample_union_ms": [],
       "hash_copies_ms": []}

if not PROF:
    # the barcode lists on the host, once (not timed: the parent's way would need them as well): the records sorted by hash, block ascending inside
    n_hash = h.export_blocks()["nHash"].astype(np.int64)
    hashes = h.export_clushash()["hash"].astype(np.int64)
    blk_of = np.repeat(np.arange(nb, dtype=np.int64), n_hash)
    order = np.lexsort((blk_of, hashes))
    hs, bs = hashes[order], blk_of[order]
    start = np.searchsorted(hs, np.arange(h.sizes()["hashNumber"] + 1))
    within = h.export_within().astype(bool); within[0] = False
    xs = np.flatnonzero(within)
    sample = np.sort(np.random.RandomState(18).choice(xs, size=min(SAMPLE, len(xs)), replace=False))


def host_groups(x, off, blk):
    """the definition for one hash from the copied-out graph: the distinct blocks, the members of each one's row among them, a union-find"""
    dd = np.unique(bs[start[x]:start[x + 1]])
    m = len(dd)
    parent = list(range(m))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, a in enumerate(dd):
        row = blk[off[a - 1]:off[a]]
        for j in np.searchsorted(dd, row[np.isin(row, dd)]):
            ra, rb = find(i), find(int(j))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    sizes = np.bincount([find(i) for i in range(m)])
    top = np.sort(sizes[sizes > 0])[::-1]
    return m, len(top), int(top[0]), int(top[1]) if len(top) > 1 else 0


for rep in range(3 if PROF else 6):
    if not PROF:
        t0 = time.perf_counter()
        off, blk, cnt = h.share_graph(T)
        t1 = time.perf_counter()
        off = off.astype(np.int64)
        a = np.array([host_groups(int(x), off, blk) for x in sample], dtype=np.uint16)
        t2 = time.perf_counter()
        res["share_graph_copy_out_ms"].append(round(1e3 * (t1 - t0), 3)); res["sample_union_ms"].append(round(1e3 * (t2 - t1), 3))
    t0 = time.perf_counter()
    b = h.hash_copies(T)
    res["hash_copies_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        res["info"] = dict(h.hash_copies_info)
        tally = h.hash_copies_tally()
        res["tally_by_crib_type"] = {name: dict(zip(("n", "one", "split"), (int(v) for v in tally[k]))) for k, name in enumerate(("err", "htA", "htB", "hom", "mul"))}
        if not PROF:
            res["rows_copied_out"] = int(len(blk))
            res["equal_on_sample"] = bool(np.array_equal(a, b[sample]))
            res["sample_list_entries"] = int(sum(start[x + 1] - start[x] for x in sample))
            res["sample_row_entries"] = int(sum(int(off[c] - off[c - 1]) for x in sample for c in np.unique(bs[start[x]:start[x + 1]])))
            # the algorithmic bytes of hc_groups_kernel over the whole table: 4 B per list entry, 4 B per row entry of every member, 8 B written per hash
            rowlen = np.zeros(nb, dtype=np.int64); rowlen[1:] = np.diff(off)
            first = np.ones(len(hs), dtype=bool); first[1:] = (hs[1:] != hs[:-1]) | (bs[1:] != bs[:-1])
            sel = first & within[hs]
            res["groups_kernel_bytes"] = {"list": int(4 * within[hs].sum()), "rows": int(4 * rowlen[bs[sel]].sum()), "out": int(8 * len(xs))}
if not PROF:
    per_hash = float(np.median(res["sample_union_ms"][1:])) / len(sample)
    res["host_union_ms_per_hash"] = round(per_hash, 5)
    res["host_union_extrapolated_to_table_s"] = round(per_hash * len(xs) / 1e3, 1)       # an extrapolation from the sample, not a measurement
print(json.dumps(res))
