"""Timing of the batched Initializer reconstruction, one
process: the C call orbm_initializer_reconstruct (host pointers in, results out,
so the host-side compaction, the upload, four launches and the download are all
inside) for 1 and 256 pairs of 1000 matches (800 flagged inliers) through H and
through F, the chain orbm_initializer_ransac + orbm_initializer_reconstruct on
the same pairs at nit = 200, and the CPU restatements (tests/cpp/initrecon_ref.c
and initransac_ref.c, one thread) on the same inputs -- the comparison point;
nothing here is measured against OpenCV, which this tree cannot build.  Host
clock around the synchronous calls; p50 over --iters calls after --warmup, each
case repeated --repeats times (the spread is reported).  Every timed result is
compared with the restatement bit for bit in the same run.  Prints one JSON line
per case and writes them to --out.  --profile only repeats the two 256-pair
calls a few times, for a kernel trace.  Needs a GPU."""
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

import initransac_util as RU  # noqa: E402
import initrecon_util as U  # noqa: E402

DISTINCT = 16  # scenes built per model; a batch cycles through them
NIT = 200
NINL, NOUT = 800, 200


def p50(v):
    return float(np.percentile(np.asarray(v), 50))


def scenes(kind):
    out = []
    for i in range(DISTINCT):
        pair, _ = U.scene(kind, NINL, 900 + i, nout=NOUT, extra1=300, extra2=250, noise=0.3)
        out.append(dict(pair, sets=RU.rng_sets(NINL + NOUT, NIT, 900 + i)))
    return out


def time_fn(fn, iters, warmup):
    ts = []
    for i in range(warmup + iters):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e6)
    return p50(ts)


P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


class RansacCall:
    """the arguments of one orbm_initializer_ransac call, built once"""

    def __init__(self, orbx, pairs):
        self.orbx, self.n = orbx, len(pairs)
        self.arr = (orbx.RansacPair * self.n)()
        self.keep, off = [], [0]
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


class ReconCall:
    """the arguments of one orbm_initializer_reconstruct call, built once; with
    `ransac` the records and flags are read where that RansacCall writes them"""

    def __init__(self, orbx, pairs, model=None, ransac=None):
        self.orbx, self.n = orbx, len(pairs)
        self.arr = (orbx.ReconPair * self.n)()
        self.keep, off = [], [0]
        for i, pr in enumerate(pairs):
            a = [np.ascontiguousarray(pr["keys1"]), np.ascontiguousarray(pr["keys2"]),
                 np.ascontiguousarray(pr["match12"], np.int32)]
            if ransac is None:
                a += [np.ascontiguousarray(pr["ransac"], orbx.RANSAC_RESULT_DTYPE).reshape(1),
                      np.ascontiguousarray(pr["inliers_H"], np.uint8), np.ascontiguousarray(pr["inliers_F"], np.uint8)]
            else:
                o = ransac.off
                a += [ransac.res[i:i + 1], ransac.inl_h[o[i]:o[i + 1]], ransac.inl_f[o[i]:o[i + 1]]]
            self.keep.append(a)
            K = np.asarray(pr["K"], np.float32).reshape(9)
            self.arr[i] = orbx.ReconPair(len(a[0]), len(a[1]), P(a[0]), P(a[1]), P(a[2]), (ctypes.c_float * 9)(*K.tolist()),
                                         int(pr["model"] if model is None else model), P(a[3]), P(a[4]), P(a[5]))
            off.append(off[-1] + len(a[0]))
        self.off = np.array(off, np.int32)
        self.res = np.zeros(self.n, orbx.RECON_RESULT_DTYPE)
        self.p3d = np.zeros((off[-1], 3), np.float32)
        self.tri = np.zeros(off[-1], np.uint8)
        self.args = (self.n, ctypes.cast(self.arr, ctypes.c_void_p), ctypes.c_float(U.SIGMA),
                     ctypes.c_float(U.MIN_PARALLAX), U.MIN_TRIANGULATED, 0, P(self.res), P(self.p3d), P(self.tri),
                     P(self.off))

    def __call__(self):
        rc = self.orbx.lib().orbm_initializer_reconstruct(*self.args)
        if rc:
            raise SystemExit("orbm_initializer_reconstruct: %d" % rc)

    def result(self, p):
        r, o = self.res[p], self.off
        d = {k: r[k] for k in self.orbx.RECON_RESULT_DTYPE.names}
        d.update(P3D=self.p3d[o[p]:o[p + 1]], triangulated=self.tri[o[p]:o[p + 1]])
        return d


def check(call, refs, what):
    bad = [(p, U.same_recon(call.result(p), refs[p % DISTINCT])) for p in range(call.n)]
    bad = [b for b in bad if b[1]]
    assert not bad, ("timed result differs from the restatement", what, bad[:4])


def chain_pair(pair, rs):
    """the pair as the chain's reconstruction sees it: AUTO over what the RANSAC left"""
    return dict(pair, model=U.AUTO, ransac=rs["rec"], inliers_H=rs["inliers_H"], inliers_F=rs["inliers_F"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initrecon_latency.json"))
    args = ap.parse_args()
    import orbx
    if orbx.device_count() < 1:
        raise SystemExit("initrecon_latency: no GPU visible")
    rows = []
    for kind, model, name in (("planar", U.H, "H"), ("general", U.F, "F")):
        sc = scenes(kind)
        if args.profile:
            call = ReconCall(orbx, [sc[i % DISTINCT] for i in range(256)], model)
            for _ in range(20):
                call()
            continue
        refs = [U.ref_reconstruct(p) for p in sc]
        assert all(r["ok"] == 1 for r in refs), [r["ok"] for r in refs]
        cpu_us = float(np.mean([time_fn(lambda p=p: U.ref_reconstruct(p), 5, 1) for p in sc]))
        # the chain's restatement: the models, then the reconstruction of what they leave
        ir = [RU.ref_initialize(p, NIT) for p in sc]
        cpu_ransac_us = float(np.mean([time_fn(lambda p=p: RU.ref_initialize(p, NIT), 3, 0) for p in sc[:4]]))
        chain_in = []
        for p, r in zip(sc, ir):
            rec = np.zeros((), orbx.RANSAC_RESULT_DTYPE)
            for k in orbx.RANSAC_RESULT_DTYPE.names:
                rec[k] = r[k]
            chain_in.append(chain_pair(p, dict(rec=rec, inliers_H=r["inliers_H"], inliers_F=r["inliers_F"])))
        chain_refs = [U.ref_reconstruct(p) for p in chain_in]
        cpu_chain_recon_us = float(np.mean([time_fn(lambda p=p: U.ref_reconstruct(p), 5, 1) for p in chain_in]))
        for npair in (1, 256):
            pairs = [sc[i % DISTINCT] for i in range(npair)]
            call = ReconCall(orbx, pairs, model)
            ts = []
            for _ in range(args.repeats):
                call.res[:] = 0
                call.p3d[:] = 7
                call.tri[:] = 7
                ts.append(time_fn(call, args.iters, args.warmup))
                check(call, refs, (name, npair))
            row = dict(case="reconstruct_" + name, nmatch=NINL + NOUT, n_inliers=NINL, npair=npair, p50_us=p50(ts),
                       repeats_us=ts, per_pair_us=p50(ts) / npair, restatement_cpu_us_per_pair=cpu_us,
                       restatement_cpu_us_batch_one_thread=cpu_us * npair, checked_bit_for_bit=True)
            rows.append(row)
            print(json.dumps(row), flush=True)
            rcall = RansacCall(orbx, pairs)
            ccall = ReconCall(orbx, pairs, U.AUTO, ransac=rcall)

            def chain():
                rcall()
                ccall()

            ts = []
            for _ in range(args.repeats):
                ts.append(time_fn(chain, max(args.iters // 4, 5), max(args.warmup // 4, 2)))
                check(ccall, chain_refs, ("chain " + name, npair))
            used = sorted(set(int(ccall.res[p]["model_used"]) for p in range(npair)))
            row = dict(case="ransac_plus_reconstruct_" + kind, nmatch=NINL + NOUT, npair=npair, nit=NIT, p50_us=p50(ts),
                       repeats_us=ts, per_pair_us=p50(ts) / npair, models_used=used,
                       ok=int(sum(int(ccall.res[p]["ok"]) for p in range(npair))),
                       restatement_cpu_us_per_pair=cpu_ransac_us + cpu_chain_recon_us,
                       restatement_cpu_us_batch_one_thread=(cpu_ransac_us + cpu_chain_recon_us) * npair,
                       checked_bit_for_bit=True)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.profile:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/initrecon_latency.py", iters=args.iters, warmup=args.warmup, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
