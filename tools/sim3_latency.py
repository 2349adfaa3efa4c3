"""Timing of the batched Sim3Solver RANSAC, one process: the C
call orbm_sim3_solve (host pointers in, results out, so the upload, the one
launch and the download are all inside) for 1, 8, 64 and 256 problems of 50 and
300 correspondences at nit = 300, and the CPU restatement (tests/cpp/sim3_ref.c,
gcc -O2, one thread) on the same problems -- the comparison point; nothing here
is measured against OpenCV, which this tree cannot build.  min_inliers is out of
reach in every problem, so that neither side stops early: both evaluate all 300
hypotheses.  Host clock around the synchronous call; p50 over --iters calls
after --warmup, each case repeated --repeats times (the spread is reported).
Every timed result is compared with the restatement bit for bit in the same
run.  Prints one JSON line per case and writes them to --out.  Needs a GPU."""
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

import sim3_util as U  # noqa: E402

DISTINCT = 16  # scenes built per size; a batch cycles through them
NIT = 300


def p50(v):
    return float(np.percentile(np.asarray(v), 50))


def scenes(ncorr):
    return [U.scene(ncorr, 700 + i, s=(1.0, 0.7, 1.4)[i % 3], nit=NIT, fix_scale=i % 3 == 0, min_inliers=ncorr)[0]
            for i in range(DISTINCT)]


def time_ref(problems, iters):
    out = []
    for pr in problems:
        U.ref_solve(pr)
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            U.ref_solve(pr)
            ts.append((time.perf_counter() - t0) * 1e6)
        out.append(p50(ts))
    return float(np.mean(out))


class RawCall:
    """the arguments of one orbm_sim3_solve call, built once"""

    def __init__(self, orbx, problems):
        self.orbx, self.n = orbx, len(problems)
        self.arr = (orbx.Sim3Problem * self.n)()
        self.keep, off = [], [0]
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for i, pr in enumerate(problems):
            self.arr[i] = orbx.sim3_problem(pr, self.keep)
            off.append(off[-1] + self.arr[i].ncorr)
        self.off = np.array(off, np.int32)
        self.res = np.zeros(self.n, orbx.SIM3_RESULT_DTYPE)
        self.inl = np.zeros(off[-1], np.uint8)
        self.args = (self.n, ctypes.cast(self.arr, ctypes.c_void_p), 0, P(self.res), P(self.inl), P(self.off))

    def __call__(self):
        rc = self.orbx.lib().orbm_sim3_solve(*self.args)
        if rc:
            raise SystemExit("orbm_sim3_solve: %d" % rc)

    def result(self, p):
        r, o = self.res[p], self.off
        d = {k: r[k] for k in self.orbx.SIM3_RESULT_DTYPE.names}
        d["inliers"] = self.inl[o[p]:o[p + 1]]
        return d


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_latency.json"))
    args = ap.parse_args()
    import orbx
    if orbx.device_count() < 1:
        raise SystemExit("sim3_latency: no GPU visible")
    rows = []
    for ncorr in (50, 300):
        sc = scenes(ncorr)
        refs = [U.ref_solve(p) for p in sc]
        assert all(r["it_hit"] == -1 and r["counters"]["evaluated"] == NIT for r in refs)
        cpu_us = time_ref(sc, 5)  # mean over the distinct scenes of the p50 of one problem
        for nprob in (1, 8, 64, 256):
            call = RawCall(orbx, [sc[i % DISTINCT] for i in range(nprob)])
            ts = []
            for _ in range(args.repeats):
                call.res[:] = 0
                call.inl[:] = 7
                ts.append(time_call(call, args.iters, args.warmup))
                bad = [(p, U.same_result(call.result(p), refs[p % DISTINCT])) for p in range(nprob)]
                bad = [b for b in bad if b[1]]
                assert not bad, ("timed result differs from the restatement", ncorr, nprob, bad[:4])
            row = dict(case="host_form", ncorr=ncorr, nprob=nprob, nit=NIT, p50_us=p50(ts), repeats_us=ts,
                       per_problem_us=p50(ts) / nprob, restatement_cpu_us_per_problem=cpu_us,
                       restatement_cpu_us_batch_one_thread=cpu_us * nprob, checked_bit_for_bit=True)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/sim3_latency.py", iters=args.iters, warmup=args.warmup, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
