"""Batched vs per-neighbour SearchForTriangulation timing: one
KeyFrame of 2000 features against 20 neighbours of 2000 features, a 100-node
FeatureVector, about half the features with MapPoints (the neighbour loop of
LocalMapping::CreateNewMapPoints).  Times the C ABI itself (the ctypes
structs are built once): p50 of the one batched call, p50 of the 20 single
calls, and p50 of the CPU restatement (tests/cpp/triangulation_ref.c, one
core) over the same 20 neighbours.  The two device forms alternate in one
loop so that both see the same clocks.  Prints one JSON line."""
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
import triangulation_util as T  # noqa: E402

NK, NNODES, PER = int(os.environ.get("NK", 20)), 100, 20
CALLS, REF_CALLS = int(os.environ.get("CALLS", 200)), int(os.environ.get("REF_CALLS", 20))
nodes = {7 * j + 3: PER for j in range(NNODES)}
kf1, kf2s, Fs = T.make_case(5, nodes, [nodes] * NK, mp1=0.5, mp2=0.5)
n1 = len(kf1["keys"])

keep = []
b1 = orbx.tri_struct(kf1, keep)
arr = (orbx.TriFrame * NK)(*[orbx.tri_struct(k, keep) for k in kf2s])
F = np.ascontiguousarray(np.asarray(Fs, np.float32).reshape(NK, 9))
m = np.zeros((NK, n1), np.int32)
nm = np.zeros(NK, np.int32)
ms = np.zeros((NK, n1), np.int32)
nms = np.zeros(NK, np.int32)
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
fn = orbx.lib().orbm_search_for_triangulation


def batched():
    rc = fn(ctypes.byref(b1), NK, ctypes.cast(arr, ctypes.c_void_p), vp(F), 0, 1, 0, vp(m), vp(nm))
    assert rc == 0, rc


def singles():
    for p in range(NK):
        rc = fn(ctypes.byref(b1), 1, ctypes.byref(arr[p]), vp(F[p]), 0, 1, 0, vp(ms[p]), vp(nms[p:]))
        assert rc == 0, rc


for _ in range(10):
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
tr = []
for _ in range(REF_CALLS):
    t0 = time.perf_counter()
    rm, rnm, _ = T.ref_batch(kf1, kf2s, Fs)
    tr.append(time.perf_counter() - t0)
cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][:1]
pct = lambda a, q: round(float(np.percentile(a, q)) * 1e3, 4)
print(json.dumps({
    "box": {"device": torch.cuda.get_device_name(0),
            "arch": torch.cuda.get_device_properties(0).gcnArchName, "hip": torch.version.hip,
            "cpu": cpu[0] if cpu else None},
    "neighbours": NK, "features": n1, "nodes": NNODES, "calls": CALLS,
    "batched_ms_p50": pct(tb, 50), "batched_ms_p10": pct(tb, 10), "batched_ms_p90": pct(tb, 90),
    "singles_ms_p50": pct(ts, 50), "singles_ms_p10": pct(ts, 10), "singles_ms_p90": pct(ts, 90),
    "cpu_restatement_ms_p50": pct(tr, 50), "cpu_restatement_calls": REF_CALLS,
    "matches": int(nm.sum()),
    "same_matches": bool(np.array_equal(m, rm) and np.array_equal(nm, rnm) and np.array_equal(ms, m)
                         and np.array_equal(nms, nm))}))
