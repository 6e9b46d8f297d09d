"""the share graph at T = 5 on the yeast-like workload, two ways to the same answer in alternation: (a) the barcode census
of every block (h10x_code_share: a sizing call, then the rows) and a numpy filter, (b) h10x_share_graph_run + _get. Call times by the host clock
around calls that end in a synchronise. Then (b) on the state after --cluster 1 0 --clusterSplit and a new range: the molecule graph.
SG_UNDER_PROF=1 (for a run under rocprofv3 --kernel-trace --stats): three rounds of (b) only."""
import json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench, hash10x_amd

T = 5
PROF = bool(os.environ.get("SG_UNDER_PROF"))
wl = bench.WORKLOADS["yeast-like-2.5M"]
recs = bench.generate(wl, seed=1)
pairs = recs.size // 30
hip, host = hash10x_amd.load_native()
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs); h.depth_range(wl["lo"], wl["hi"])
hash10x_amd.synchronize(0)
ctx = h._ctx()
nb = h.sizes()["nBlocks"]


def census_and_filter():
    q = np.arange(1, nb, dtype=np.uint32)
    off = np.zeros(q.size + 1, dtype=np.uint64)
    assert hip.h10x_code_share(ctx, q.ctypes.data, q.size, off.ctypes.data, None, None, None, None, 0) == 0
    m = int(off[-1])
    blk, cnt = np.zeros(max(m, 1), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
    assert hip.h10x_code_share(ctx, q.ctypes.data, q.size, off.ctypes.data, blk.ctypes.data, cnt.ctypes.data, None, None, m) == 0
    keep = cnt[:m] >= T
    before = np.concatenate([[0], np.cumsum(keep, dtype=np.uint64)])
    return before[off.astype(np.int64)], blk[:m][keep], cnt[:m][keep], m


res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (bench.py, gen_fqb seed 1)", "pairs": pairs, "nBlocks": nb, "T": T,
       "census_filter_ms": [], "share_graph_ms": []}
for rep in range(3 if PROF else 6):
    if not PROF:
        t0 = time.perf_counter()
        a = census_and_filter()
        res["census_filter_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    h.neighbour_stats(reset=True)
    t0 = time.perf_counter()
    b = h.share_graph(T)
    res["share_graph_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        res["info"] = dict(h.share_graph_info)
        if not PROF:
            res["rows_T1"] = a[3]
            res["equal"] = bool(all(np.array_equal(x, y) for x, y in zip(a[:3], b)))
if not PROF:
    h.cluster(1, 0, wl["ct"]); h.cluster_split(); h.depth_range(wl["lo"], wl["hi"])
    res["molecule_nBlocks"] = h.sizes()["nBlocks"]
    res["molecule_share_graph_ms"] = []
    for rep in range(3):
        t0 = time.perf_counter()
        h.share_graph(T)
        res["molecule_share_graph_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    res["molecule_info"] = dict(h.share_graph_info)
print(json.dumps(res))
