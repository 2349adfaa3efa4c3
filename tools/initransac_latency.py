"""Timing of the batched Initializer RANSAC, one process: the C
call orbm_initializer_ransac (host pointers in, results out, so the upload, the
host-side Normalize, four launches and the download are all inside) for 1, 64
and 256 pairs of 300 and 1000 matches at nit = 200, and the CPU restatement
(tests/cpp/initransac_ref.c, one thread) on the same pairs -- the comparison
point; nothing here is measured against OpenCV, which this tree cannot build.
Host clock around the synchronous call; p50 over --iters calls after --warmup,
each case repeated --repeats times (the spread is reported).  Every timed
result is compared with the restatement bit for bit in the same run.  Prints
one JSON line per case and writes them to --out.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "orb-slam-system_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import initransac_util as U  # noqa: E402

DISTINCT = 16  # scenes built per size; a batch cycles through them
NIT = 200


def p50(v):
    return float(np.percentile(np.asarray(v), 50))


def scenes(nmatch):
    return [U.scene("planar" if i % 2 else "general", nmatch, 700 + i, NIT, extra1=nmatch // 3, extra2=nmatch // 4)[0]
            for i in range(DISTINCT)]


def time_ref(pairs, iters):
    out = []
    for pair in pairs:
        U.ref_initialize(pair, NIT)
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            U.ref_initialize(pair, NIT)
            ts.append((time.perf_counter() - t0) * 1e6)
        out.append(p50(ts))
    return float(np.mean(out))


class RawCall:
    """the arguments of one orbm_initializer_ransac call, built once"""

    def __init__(self, orbx, pairs):
        self.orbx, self.n = orbx, len(pairs)
        self.arr = (orbx.RansacPair * self.n)()
        self.keep, off = [], [0]
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for i, pr in enumerate(pairs):
            a = [np.ascontiguousarray(pr["keys1"]), np.ascontiguousarray(pr["keys2"]),
                 np.ascontiguousarray(pr["match12"], np.int32), np.ascontiguousarray(pr["sets"], np.int32)]
            self.keep.append(a)
            self.arr[i] = orbx.RansacPair(len(a[0]), len(a[1]), P(a[0]), P(a[1]), P(a[2]), P(a[3]))
            off.append(off[-1] + int((a[2] >= 0).sum()))
        self.off = np.array(off, np.int32)
        self.res = np.zeros(self.n, orbx.RANSAC_RESULT_DTYPE)
        self.inl_h = np.zeros(off[-1], np.uint8)
        self.inl_f = np.zeros(off[-1], np.uint8)
        self.args = (self.n, ctypes.cast(self.arr, ctypes.c_void_p), NIT, ctypes.c_float(U.SIGMA), 0, P(self.res),
                     P(self.inl_h), P(self.inl_f), P(self.off))

    def __call__(self):
        rc = self.orbx.lib().orbm_initializer_ransac(*self.args)
        if rc:
            raise SystemExit("orbm_initializer_ransac: %d" % rc)

    def result(self, p):
        r, o = self.res[p], self.off
        return dict(H21=r["H21"], F21=r["F21"], SH=r["SH"], SF=r["SF"], RH=r["RH"], it_H=r["it_H"], it_F=r["it_F"],
                    nmatch=r["nmatch"], inliers_H=self.inl_h[o[p]:o[p + 1]], inliers_F=self.inl_f[o[p]:o[p + 1]])


def time_call(call, iters, warmup):
    ts = []
    for i in range(warmup + iters):
        t0 = time.perf_counter()
        call()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e6)
    return p50(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initransac_latency.json"))
    args = ap.parse_args()
    import orbx
    if orbx.device_count() < 1:
        raise SystemExit("initransac_latency: no GPU visible")
    rows = []
    for nmatch in (300, 1000):
        sc = scenes(nmatch)
        refs = [U.ref_initialize(p, NIT) for p in sc]
        cpu_us = time_ref(sc, 5)  # mean over the distinct scenes of the p50 of one pair
        for npair in (1, 64, 256):
            call = RawCall(orbx, [sc[i % DISTINCT] for i in range(npair)])
            ts = []
            for _ in range(args.repeats):
                call.res[:] = 0
                call.inl_h[:] = 7
                call.inl_f[:] = 7
                ts.append(time_call(call, args.iters, args.warmup))
                bad = [(p, U.same_result(call.result(p), refs[p % DISTINCT])) for p in range(npair)]
                bad = [b for b in bad if b[1]]
                assert not bad, ("timed result differs from the restatement", nmatch, npair, bad[:4])
            row = dict(case="host_form", nmatch=nmatch, npair=npair, nit=NIT, p50_us=p50(ts), repeats_us=ts,
                       per_pair_us=p50(ts) / npair, restatement_cpu_us_per_pair=cpu_us,
                       restatement_cpu_us_batch_one_thread=cpu_us * npair, checked_bit_for_bit=True)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/initransac_latency.py", iters=args.iters, warmup=args.warmup, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
