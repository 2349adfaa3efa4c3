#!/usr/bin/env python3
"""Latency of one synchronous orbm_search_for_initialization call on a pair of
2 x N-feature 640x480 frames (window 100, nnratio 0.9, orientation check on),
next to the CPU restatement (tests/cpp/initsearch_ref.c, gcc -O2, one thread)
on the same input, and the share of rows whose walk step scanned its window a
second time.  Prints one JSON line (DESIGN.md §15 quotes it).

  python tools/init_latency.py [--n 2000] [--iters 200] [--warmup 20] [--pairs 1]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "orb-slam-system_amd")):
    sys.path.insert(0, p)

import initsearch_util as U  # noqa: E402
import orbx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.RandomState(a.seed)
    pairs = []
    for _ in range(a.pairs):
        f1 = U.make_f1(rng, a.n)
        pairs.append(U.first_pair(f1, U.make_f2(rng, f1, a.n)))
    want = [U.ref_search(p) for p in pairs]
    got = orbx.search_for_initialization(pairs, stats=True)
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[1]) and np.array_equal(g[1].view(np.uint32), w[2].view(np.uint32)) \
            and g[2] == w[3], "the call and the restatement differ"

    # the raw entry point on prepared structs: the binding's copies are not timed
    keep = []
    arr = (orbx.InitPair * a.pairs)()
    for i, p in enumerate(pairs):
        arr[i] = orbx.init_pair_struct(p, keep)[0]
    nm = np.zeros(a.pairs, np.int32)
    fn = orbx.lib().orbm_search_for_initialization
    args = (a.pairs, ctypes.cast(arr, ctypes.c_void_p), 100, 0.9, 1, 0, nm.ctypes.data_as(ctypes.c_void_p))
    # every call starts from the first call's state
    m0 = [np.full(a.n, -1, np.int32) for _ in pairs]
    p0 = [p["prev_matched"].copy() for p in pairs]
    ts = []
    for it in range(a.warmup + a.iters):
        for i in range(a.pairs):
            keep[6 * i + 4][:] = p0[i]  # init_pair_struct keeps [keys1, desc1, keys2, desc2, prev, m12]
            keep[6 * i + 5][:] = m0[i]
        t = time.perf_counter()
        rc = fn(*args)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        if it >= a.warmup:
            ts.append(dt)
    tr = []
    for _ in range(5):
        t = time.perf_counter()
        for p in pairs:
            U.ref_search(p)
        tr.append(time.perf_counter() - t)
    rows = sum(int((p["f1"]["keys"]["octave"] <= 0).sum()) for p in pairs)
    print(json.dumps(dict(n=a.n, pairs=a.pairs, iters=a.iters, call_p50_us=round(1e6 * float(np.median(ts)), 1),
                          call_p10_us=round(1e6 * float(np.percentile(ts, 10)), 1),
                          call_p90_us=round(1e6 * float(np.percentile(ts, 90)), 1),
                          restatement_min_us=round(1e6 * min(tr), 1), rows_searched=rows,
                          rescans=int(sum(g[3] for g in got)),
                          rescan_share=round(sum(g[3] for g in got) / max(rows, 1), 5),
                          nmatches=[int(g[2]) for g in got])))


if __name__ == "__main__":
    main()
