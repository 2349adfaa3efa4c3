#!/usr/bin/env python3
"""Latency of the keyframe database's queries, single against batched
(DESIGN §16 "Measured").  Setup as §16's: a 100,000-word synthetic vocabulary,
keyframes of 1400-1600 random words, 1500-word queries that share a word with
every keyframe, 1,000 and 10,000 keyframes.  Timed with the host clock around
synchronous calls of the C ABI over preallocated buffers, 5 warm-up calls and
then --calls timed ones, per Q = 1, 16, 256 queries:

  (a) single   a loop of Q orbv_db_query calls
  (b) batch    one orbv_db_query_batch of Q queries, ungated and gated
  (c) device   one orbv_db_query_batch_device plus one stream synchronise

and reported per query: p50 (p10-p90) in microseconds.  The three are checked
against each other on the first call.  One JSON line per row, then the table.

  python tools/bowdb_query_bench.py [--keyframes 1000 10000] [--queries 1 16 256] [--calls 50]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bowdb_query_bench.py --profile

--profile makes a few calls of each form at Q = 256 and nothing else: kernel
times come from that separate run, never from the timed one.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb-slam-system_amd"))

NWORDS = 100000
ANCHORS = 64  # every query holds them all, every keyframe one of them


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def make_bow(rng, n, must):
    w = np.unique(np.concatenate([rng.integers(0, NWORDS, n + n // 50), must]))
    keep = np.setdiff1d(w, must)
    keep = keep[rng.permutation(len(keep))[:n - len(must)]]
    w = np.sort(np.concatenate([keep, must])).astype(np.uint32)
    v = rng.uniform(0.1, 1.0, len(w))
    return w, v / v.sum()


def percentiles(us):
    return [float(np.percentile(us, q)) for q in (50, 10, 90)]


def timed(call, calls, warmup=5):
    for _ in range(warmup):
        call()
    t = np.zeros(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        call()
        t[i] = time.perf_counter() - t0
    return t * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.calls < 50 and not a.profile:
        ap.error("at least 50 timed calls")

    import torch
    import orbx
    from orbx import synth
    if orbx.device_count() < 1:
        raise SystemExit("no GPU visible: nothing is measured without one")
    L = orbx.lib()
    voc = orbx.Vocabulary.from_records(synth.vocabulary(k=10, L=5, stop_frac=0.0))
    assert voc.info()["nwords"] == NWORDS
    rng = np.random.default_rng(16)
    anchors = np.sort(rng.choice(NWORDS, ANCHORS, replace=False)).astype(np.uint32)
    qmax = max(a.queries) if not a.profile else 256
    qs = [make_bow(rng, 1500, anchors) for _ in range(qmax)]
    rows = []
    for nkf in (a.keyframes if not a.profile else [max(a.keyframes)]):
        db = orbx.KeyFrameDatabase(voc, reserve_words=nkf * 1600)
        for i in range(nkf):
            db.add(i, make_bow(rng, int(rng.integers(1400, 1601)), anchors[int(rng.integers(ANCHORS))][None]))
        h = db._h
        for Q in ([256] if a.profile else a.queries):
            off = np.zeros(Q + 1, np.uint32)
            off[1:] = np.cumsum([len(w) for w, _ in qs[:Q]])
            qw = np.concatenate([w for w, _ in qs[:Q]])
            qv = np.concatenate([v for _, v in qs[:Q]])
            cap = Q * nkf
            out = np.zeros(Q + 1, np.uint32)
            ids, nc, sc = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
            ids1, nc1, sc1 = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
            n = ctypes.c_int()
            ptrs = [(p(qw[off[q]:]), p(qv[off[q]:]), int(off[q + 1] - off[q]), p(ids1[q * nkf:]), p(nc1[q * nkf:]),
                     p(sc1[q * nkf:])) for q in range(Q)]
            counts = np.zeros(Q, np.int64)

            def single():
                for q, (w_, v_, n_, i_, c_, s_) in enumerate(ptrs):
                    assert L.orbv_db_query(h, w_, v_, n_, nkf, i_, c_, s_, ctypes.byref(n)) == 0
                    counts[q] = n.value

            def batch(flags):
                assert L.orbv_db_query_batch(h, Q, p(off), p(qw), p(qv), flags, cap, p(out), p(ids), p(nc), p(sc)) == 0

            stride = int(max(off[1:] - off[:-1]))
            dw = np.zeros((Q, stride), np.int32)
            dv = np.zeros((Q, stride), np.float64)
            for q in range(Q):
                dw[q, :off[q + 1] - off[q]] = qw[off[q]:off[q + 1]].astype(np.int32)
                dv[q, :off[q + 1] - off[q]] = qv[off[q]:off[q + 1]]
            tw, tv = torch.from_numpy(dw).cuda(), torch.from_numpy(dv).cuda()
            tn = torch.from_numpy((off[1:] - off[:-1]).astype(np.int32)).cuda()
            o = db.query_batch_device(tw, tv, tn, nkf)
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()

            def device():
                db.query_batch_device_into(tw, tv, tn, o, stream=stream)
                stream.synchronize()

            # the three forms agree before anything is timed
            single()
            batch(0)
            device()
            assert (out[1:] - out[:-1]).tolist() == counts.tolist() == o["nsharing"].cpu().numpy().tolist()
            assert counts.min() == nkf  # every keyframe shares a word with every query
            dk, ds = o["kf_id"].cpu().numpy(), o["score"].cpu().numpy()
            for q in range(Q):
                s = slice(int(out[q]), int(out[q + 1]))
                assert np.array_equal(ids[s], ids1[q * nkf:q * nkf + nkf]) and np.array_equal(ids[s], dk[q].astype(np.uint64))
                assert np.array_equal(sc[s].view(np.uint64), sc1[q * nkf:q * nkf + nkf].view(np.uint64))
                assert np.array_equal(sc[s].view(np.uint64), ds[q].view(np.uint64))
            if a.profile:
                for _ in range(4):
                    single(), batch(0), batch(1), device()
                continue
            forms = (("single", single), ("batch", lambda: batch(0)), ("batch gated", lambda: batch(1)),
                     ("device", device))
            for name, call in forms:
                p50, p10, p90 = percentiles(timed(call, a.calls) / Q)
                kept = int(out[Q]) if name.startswith("batch") else cap
                row = dict(keyframes=nkf, queries=Q, form=name, calls=a.calls, p50_us_per_query=round(p50, 2),
                           p10_us_per_query=round(p10, 2), p90_us_per_query=round(p90, 2), entries=kept)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del db
    if rows:
        print("\n| keyframes | Q | form | per query p50 (p10-p90) µs | entries returned |\n|---|---|---|---|---|")
        for r in rows:
            print("| %d | %d | %s | %.1f (%.1f-%.1f) | %d |" % (r["keyframes"], r["queries"], r["form"],
                                                                 r["p50_us_per_query"], r["p10_us_per_query"],
                                                                 r["p90_us_per_query"], r["entries"]))


if __name__ == "__main__":
    main()
