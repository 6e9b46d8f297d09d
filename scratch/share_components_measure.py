"""the linkage groups at T = 5 on the yeast-like workload after --cluster 1 0 --clusterSplit and the range again (the molecules), two
ways to the same five arrays in one process, in alternation: (a) the parent's way, Hash10x.share_graph(5) over all blocks copied out to host arrays and a
vectorised numpy min-label union there, (b) Hash10x.share_components(5), at the default 8192 blocks a range and with all blocks in one range. Call times by
the host clock around calls that end in a synchronise. SC_UNDER_PROF=1 (for a run under rocprofv3 --kernel-trace --stats): three rounds of (b) only."""
import json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench, hash10x_amd

T = 5
PROF = bool(os.environ.get("SC_UNDER_PROF"))
wl = bench.WORKLOADS["yeast-like-2.5M"]
recs = bench.generate(wl, seed=1)
pairs = recs.size // 30
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs); h.depth_range(wl["lo"], wl["hi"]); h.cluster(1, 0, wl["ct"]); h.cluster_split(); h.depth_range(wl["lo"], wl["hi"])
hash10x_amd.synchronize(0)
nb = h.sizes()["nBlocks"]
n_hash = h.export_blocks()["nHash"].astype(np.int64)


def host_union(off, blk):
    """min-label union over the rows: hook the larger root's label to the smaller (np.minimum.at), compress by pointer jumping, until no row is open"""
    src = np.repeat(np.arange(1, nb, dtype=np.int64), np.diff(off.astype(np.int64)))
    dst = blk.astype(np.int64)
    lab = np.arange(nb, dtype=np.int64)
    rounds = 0
    while True:
        ls, ld = lab[src], lab[dst]
        hi, lo = np.maximum(ls, ld), np.minimum(ls, ld)
        m = hi != lo
        if not m.any():
            break
        rounds += 1
        np.minimum.at(lab, hi[m], lo[m])
        while True:
            nl = lab[lab]
            if np.array_equal(nl, lab):
                break
            lab = nl
    roots = np.unique(lab[1:])
    comp = np.zeros(nb, dtype=np.uint32)
    comp[1:] = np.searchsorted(roots, lab[1:]) + 1
    blocks = np.bincount(comp[1:], minlength=len(roots) + 1).astype(np.uint32)
    records = np.zeros(len(roots) + 1, dtype=np.uint64)
    np.add.at(records, comp[1:], n_hash[1:].astype(np.uint64))
    return (comp, lab.astype(np.uint32), np.concatenate([[0], roots]).astype(np.uint32), blocks, records), rounds


res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (bench.py, gen_fqb seed 1), after --cluster 1 0 --clusterSplit, range again", "pairs": pairs,
       "nBlocks": nb, "T": T, "share_graph_copy_out_ms": [], "host_union_ms": [], "parent_way_ms": [], "share_components_ms": [], "share_components_one_range_ms": []}
for rep in range(3 if PROF else 6):
    if not PROF:
        t0 = time.perf_counter()
        off, blk, cnt = h.share_graph(T)
        t1 = time.perf_counter()
        a, rounds = host_union(off, blk)
        t2 = time.perf_counter()
        res["share_graph_copy_out_ms"].append(round(1e3 * (t1 - t0), 3)); res["host_union_ms"].append(round(1e3 * (t2 - t1), 3))
        res["parent_way_ms"].append(round(1e3 * (t2 - t0), 3))
    h.set_option("share_graph_blocks", 0)
    t0 = time.perf_counter()
    b = h.share_components(T)
    res["share_components_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        res["info"] = dict(h.share_components_info)
        res["ranges"] = -(-nb // 8192)
    h.set_option("share_graph_blocks", 1 << 30)
    t0 = time.perf_counter()
    b1 = h.share_components(T)
    res["share_components_one_range_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        res["info_one_range"] = dict(h.share_components_info)
        res["one_range_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(b, b1)))
        if not PROF:
            res["host_union_rounds"] = rounds
            res["rows_copied_out"] = int(len(blk))
            res["equal"] = bool(all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)))
print(json.dumps(res))
