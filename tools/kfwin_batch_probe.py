"""Batched vs per-keyframe orbm_keyframe_search timing at the
shape of LocalMapping::SearchInNeighbors: keyframes of 2000 features at
640 x 480, 60 target keyframes x 1500 queries (the current keyframe's map
points, one shared descriptor per map point) plus one keyframe x 40000 queries
(every target's map points), th = 3.  Times the C ABI itself (the ctypes
structs are built once): p50 of the one batched call, p50 of the same 61
problems as one call each, and p50 of the CPU restatement
(tests/cpp/kfwindow_ref.c, one core, grids built beforehand as the reference's
KeyFrame has them; the grid build is reported apart).  The two device forms
alternate in one loop so that both see the same clocks.  Also reports what a
query visits: cell entries per query, and entries per (query, column) run,
which is what k_kfwin_search's KFW_G lanes read at a time.  Prints one JSON
line."""
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, "..", "orb-slam-system_amd"))
import torch  # noqa: E402

import orbx  # noqa: E402
import kfwindow_util as K  # noqa: E402

NKF, NFEAT, NQ, NQ_LAST = int(os.environ.get("NKF", 60)), 2000, 1500, int(os.environ.get("NQ_LAST", 40000))
CALLS, REF_CALLS = int(os.environ.get("CALLS", 100)), int(os.environ.get("REF_CALLS", 5))
TH = np.float32(3.0)
rng = np.random.RandomState(5)
sf = K.scale_factors()
# features per pyramid level as ORBextractor spreads them: ~ 1 / 1.2 per level
plevel = (1.0 / 1.2) ** np.arange(K.NLEVELS)
plevel /= plevel.sum()


def few_bits(n, mean_bits=4.0):
    """n x 32 masks with about mean_bits bits set"""
    return np.packbits(rng.uniform(size=(n, 256)) < mean_bits / 256.0, axis=1)


def frame(desc):
    n = len(desc)
    keys = K.make_keys(rng.uniform(0, K.W, n).astype(np.float32), rng.uniform(0, K.H, n).astype(np.float32),
                       rng.choice(K.NLEVELS, n, p=plevel).astype(np.int32))
    return K.frame_dict(keys, desc)


def queries(kf, feat, rows):
    """query i: feature feat[i]'s place plus noise at its octave or the one
    above (70 %) or a random place (30 %); descriptor pool row rows[i]"""
    n = len(feat)
    k = kf["keys"][feat]
    level = np.minimum(k["octave"] + (rng.uniform(size=n) < 0.4), K.NLEVELS - 1).astype(np.int32)
    s = 0.8 * sf[level]
    x = k["x"] + rng.normal(0, 1, n) * s
    y = k["y"] + rng.normal(0, 1, n) * s
    away = rng.uniform(size=n) < 0.3
    x[away], y[away] = rng.uniform(0, K.W, away.sum()), rng.uniform(0, K.H, away.sum())
    q = np.zeros(n, K.KF_QUERY_DTYPE)
    q["x"], q["y"], q["radius"], q["level"], q["desc"] = x, y, TH * sf[level], level, rows
    return q


# the current keyframe's map points: one descriptor each, seen in every target
pool_cur = rng.randint(0, 256, (NQ, 32)).astype(np.uint8)
kfs, qs = [], []
for p in range(NKF):
    desc = rng.randint(0, 256, (NFEAT, 32)).astype(np.uint8)
    seen = rng.permutation(NFEAT)[:NQ]  # feature seen[j] observes map point j
    desc[seen] = pool_cur ^ few_bits(NQ)
    kf = frame(desc)
    kfs.append(kf)
    qs.append(queries(kf, seen, np.arange(NQ, dtype=np.int32)))
# the current keyframe itself, searched by every target's map points
desc = rng.randint(0, 256, (NFEAT, 32)).astype(np.uint8)
kf = frame(desc)
feat = rng.randint(0, NFEAT, NQ_LAST)
pool_last = desc[feat] ^ few_bits(NQ_LAST)
kfs.append(kf)
qs.append(queries(kf, feat, NQ + np.arange(NQ_LAST, dtype=np.int32)))
pool = np.ascontiguousarray(np.concatenate([pool_cur, pool_last]))
NP = len(kfs)

keep = []
arr = (orbx.KfFrame * NP)(*[orbx.kf_struct(k, keep) for k in kfs])
qoff = np.zeros(NP + 1, np.int32)
qoff[1:] = np.cumsum([len(q) for q in qs])
qall = np.ascontiguousarray(np.concatenate(qs))
nq = int(qoff[-1])
bi, bd = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
si, sd = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
# one call per problem: each with the pool slice its queries use
q_single = [q.copy() for q in qs]
q_single[-1]["desc"] -= NQ
pools = [pool_cur] * NKF + [np.ascontiguousarray(pool_last)]
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
fn = orbx.lib().orbm_keyframe_search


def batched():
    rc = fn(NP, ctypes.cast(arr, ctypes.c_void_p), vp(qall), vp(qoff), vp(pool), len(pool), 0, vp(bi), vp(bd))
    assert rc == 0, rc


def singles():
    for p in range(NP):
        o = np.array([0, len(q_single[p])], np.int32)
        rc = fn(1, ctypes.byref(arr[p]), vp(q_single[p]), vp(o), vp(pools[p]), len(pools[p]), 0,
                vp(si[qoff[p]:]), vp(sd[qoff[p]:]))
        assert rc == 0, rc


for _ in range(5):
    batched()
    singles()
tb, ts = [], []
for _ in range(CALLS):
    t0 = time.perf_counter()
    batched()
    t1 = time.perf_counter()
    singles()
    t2 = time.perf_counter()
    tb.append(t1 - t0)
    ts.append(t2 - t1)

# the restatement on one core: grids beforehand (the KeyFrame has its grid)
ref = K.ref_lib()
rkeep = []
structs = [K._struct(k, rkeep) for k in kfs]
ri, rd = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
tg, tr = [], []
for it in range(REF_CALLS):
    t0 = time.perf_counter()
    grids = [ref.kfw_grid_create(ctypes.byref(s)) for s in structs]
    t1 = time.perf_counter()
    for p in range(NP):
        ref.kfw_search_grid(grids[p], vp(qs[p]), len(qs[p]), vp(pool), vp(ri[qoff[p]:]), vp(rd[qoff[p]:]), None)
    t2 = time.perf_counter()
    for g in grids:
        ref.kfw_grid_free(g)
    tg.append(t1 - t0)
    tr.append(t2 - t1)

# what a query visits (restatement's counts), and the (query, column) runs
st = np.zeros((nq, 5), np.int32)
runs = []
f32 = np.float32
for p in range(NP):
    o = slice(qoff[p], qoff[p + 1])
    ref.kfw_search(ctypes.byref(structs[p]), vp(qs[p]), len(qs[p]), vp(pool), vp(ri[o]), vp(rd[o]), vp(st[o]))
    k, q = kfs[p]["keys"], qs[p]
    wi, hi = f32(kfs[p]["grid_w_inv"]), f32(kfs[p]["grid_h_inv"])
    cnt = np.zeros((K.COLS, K.ROWS + 1), np.int64)
    px = np.floor((k["x"] * wi).astype(np.float64) + 0.5).astype(int)  # round(), x >= 0
    py = np.floor((k["y"] * hi).astype(np.float64) + 0.5).astype(int)
    ok = (px >= 0) & (px < K.COLS) & (py >= 0) & (py < K.ROWS)
    np.add.at(cnt, (px[ok], py[ok] + 1), 1)
    pre = np.cumsum(cnt, axis=1)
    x0 = np.maximum(0, np.floor((q["x"] - q["radius"]) * wi).astype(int))
    x1 = np.minimum(K.COLS - 1, np.ceil((q["x"] + q["radius"]) * wi).astype(int))
    y0 = np.maximum(0, np.floor((q["y"] - q["radius"]) * hi).astype(int))
    y1 = np.minimum(K.ROWS - 1, np.ceil((q["y"] + q["radius"]) * hi).astype(int))
    for c in range(int((x1 - x0).max()) + 1):
        ix = x0 + c
        m = (ix <= x1) & (y1 >= y0)
        runs.append(pre[ix[m], y1[m] + 1] - pre[ix[m], y0[m]])
runs = np.concatenate(runs)
visited, boxed, gated = st[:, 0], st[:, 1], st[:, 2]
assert runs.sum() == visited.sum(), (runs.sum(), visited.sum())
label = lambda lo, hi: "%d" % lo if hi == lo + 1 else "%d+" % lo if hi >= 1 << 30 else "%d-%d" % (lo, hi - 1)
hist = lambda a, edges: {label(lo, hi): int(((a >= lo) & (a < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])}
cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][:1]
pct = lambda a, q: round(float(np.percentile(a, q)) * 1e3, 4)
print(json.dumps({
    "box": {"device": torch.cuda.get_device_name(0),
            "arch": torch.cuda.get_device_properties(0).gcnArchName, "hip": torch.version.hip,
            "cpu": cpu[0] if cpu else None},
    "variant": os.environ.get("ORBX_VARIANT") or None,
    "problems": NP, "features": NFEAT, "queries": nq, "pool_rows": len(pool), "calls": CALLS,
    "batched_ms_p50": pct(tb, 50), "batched_ms_p10": pct(tb, 10), "batched_ms_p90": pct(tb, 90),
    "singles_ms_p50": pct(ts, 50), "singles_ms_p10": pct(ts, 10), "singles_ms_p90": pct(ts, 90),
    "cpu_restatement_ms_p50": pct(tr, 50), "cpu_grid_build_ms_p50": pct(tg, 50),
    "cpu_restatement_calls": REF_CALLS,
    "visited_per_query": {"mean": round(float(visited.mean()), 3), "p50": int(np.percentile(visited, 50)),
                          "p90": int(np.percentile(visited, 90)), "p99": int(np.percentile(visited, 99)),
                          "max": int(visited.max())},
    "boxed_per_query_mean": round(float(boxed.mean()), 3),
    "gated_per_query_mean": round(float(gated.mean()), 3),
    "columns_per_query_mean": round(len(runs) / float(nq), 3),
    "run_length": {"mean": round(float(runs.mean()), 3), "p90": int(np.percentile(runs, 90)),
                   "p99": int(np.percentile(runs, 99)), "max": int(runs.max()),
                   "hist": hist(runs, [0, 1, 2, 3, 4, 5, 9, 17, 33, 1 << 30])},
    "matched_le_50": int((rd <= 50).sum()),
    "same_results": bool(np.array_equal(bi, ri) and np.array_equal(bd, rd) and np.array_equal(si, bi)
                         and np.array_equal(sd, bd))}))
