"""the in-range hashes of the state as a classed mosh set, on the yeast-like workload after --cluster 1 0 --clusterSplit and the
range again (the molecules), with a --hashCopies result at T = 5 kept (the run itself is common to both ways and is made once, before the timing). Two ways
in one process, in alternation, six rounds with the first dropped: (a) the host route that was possible before: hashIndex / hashValue / hashDepth / within
exported, the kept --hashCopies table copied out, the classes in numpy, MoshSet.from_arrays of the WHOLE table with the depth of every hash out of range set
to 0, prune(1, 0); (b) Hash10x.mosh_set. The two sets' exports must be equal byte for byte. Call times by the host clock around calls that end in a
synchronise. WM_UNDER_PROF=1 (for a run under rocprofv3 --kernel-trace --stats): three rounds of (b) only."""
import ctypes, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench, hash10x_amd

T, THR = 5, (30, 55, 100)
PROF = bool(os.environ.get("WM_UNDER_PROF"))
wl = bench.WORKLOADS["yeast-like-2.5M"]
recs = bench.generate(wl, seed=1)
pairs = recs.size // 30
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs)
h.depth_range(wl["lo"], wl["hi"]); h.cluster(1, 0, wl["ct"]); h.cluster_split(); h.depth_range(wl["lo"], wl["hi"])
h.hash_copies(T)
hash10x_amd.synchronize(0)
z = h.sizes()
B, n = z["B"], z["hashNumber"]
f1, f2 = ctypes.c_uint64(0), ctypes.c_uint64(0)
h._hip.h10x_factors_from_seed(17, ctypes.byref(f1), ctypes.byref(f2))

res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (bench.generate seed 1), after --cluster 1 0 --clusterSplit, range again, --hashCopies 5 kept",
       "pairs": pairs, "nBlocks": z["nBlocks"], "hashNumber": n, "B": B, "T": T, "thresholds": THR, "host_route_ms": [], "mosh_set_ms": []}


def host_route():
    ix = np.zeros(1 << B, np.uint32); v = np.zeros(n, np.uint64); dep = np.zeros(n, np.uint32)
    h._chk_ctx(h._hip.h10x_export(h._ctx(), ix.ctypes.data, v.ctypes.data, dep.ctypes.data, None, None))
    within = h.export_within().astype(bool); within[0] = False
    table = np.zeros((n, 4), np.uint16)
    h._chk_ctx(h._hip.h10x_hash_copies_get(h._ctx(), table.ctypes.data, 0, n))
    d16 = np.minimum(dep, 65535).astype(np.int64)
    cls = np.where(d16 < THR[0], 0, np.where(d16 < THR[1], 1, np.where(d16 < THR[2], 2, 3))).astype(np.uint8)
    cls[(table[:, 3] < 2) & (table[:, 2] < 2)] = 0
    cls[table[:, 3] >= 2] = 3
    d16[~within] = 0; cls[~within] = 0; v[0] = 0               # in-range depths are >= lo >= 1: prune(1, 0) keeps exactly the range
    ms = hash10x_amd.MoshSet.from_arrays(B, 21, 31, f1.value, f2.value, ix, v, d16.astype(np.uint16), cls)
    ms.prune(1, 0)
    return ms


for rep in range(3 if PROF else 6):
    a = None
    if not PROF:
        t0 = time.perf_counter()
        a = host_route()
        res["host_route_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    t0 = time.perf_counter()
    b = h.mosh_set(*THR)
    res["mosh_set_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        info = dict(h.mosh_set_info)
        res["info"] = {k: v for k, v in info.items() if k != "crib"}
        kept = info["kept"]
        # algorithmic bytes, counted here: classify 1 + 4 + 8 B read and 4 + 1 B written per hash, the scan's 4 + 4 B per hash, compact 11 B written per kept hash
        # (4 B of flag read per hash, 4 + 1 + 8 + 4 B per kept hash), the table's memset and one probe (4 B read, 4 B written, 8 B of value[]) per kept hash when nothing collides
        res["bytes"] = {"classify_read": 13 * n, "classify_written": 5 * n, "scan": 8 * n, "compact_read": 4 * n + 17 * kept, "compact_written": 11 * kept,
                        "table_memset": 4 << info["bits"], "place_min": 16 * kept}
        if not PROF:
            ea, eb = a.export(), b.export()
            res["equal_exports"] = bool(all(np.array_equal(x, y) for x, y in zip(ea, eb)) and a.info().max == b.info().max == kept)
    if a is not None:
        a.close()
    b.close()
print(json.dumps(res))
