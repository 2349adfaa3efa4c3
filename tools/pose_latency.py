"""Timing of the batched pose-only optimisation, one process:
the host form (orbm_pose_optimization) for one problem, the plan form
(orbm_pose_plan_optimize) per call for batches of problems, and the CPU
restatement (tests/cpp/poseopt_ref.c, one thread) on the same problems -- the
comparison point, because g2o itself cannot be built without Eigen.  Host
clock around work that ends in a device synchronise for the host form, device
events for the plan form; p50 over --iters calls after --warmup, each case
repeated --repeats times (the spread is reported).  Prints one JSON line per
case and writes them to --out.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "orb-slam-system_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import poseopt_util as U  # noqa: E402

DISTINCT = 16  # scenes built; a batch cycles through them (outputs are per problem)


def p50(v):
    return float(np.percentile(np.asarray(v), 50))


def problems(n, count):
    return [U.scene(n, 900 + i, **U.OUTLIER_SCENE)[:2] for i in range(min(count, DISTINCT))]


def work(refs):
    """what the timed problems do, from the restatement's counters: Levenberg
    trials (each one solve, one pose update and one chi2 pass over the edges)"""
    trials = [r["counters"]["accepted"] + r["counters"]["rejected"] for r in refs]
    return dict(trials_mean=float(np.mean(trials)), trials_max=int(max(trials)))


def time_ref(probs, iters):
    out = []
    for cam, obs in probs:
        U.ref_optimize(cam, obs)
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            U.ref_optimize(cam, obs)
            ts.append((time.perf_counter() - t0) * 1e6)
        out.append(p50(ts))
    return float(np.mean(out))


def time_host_form(orbx, torch, prob, iters, warmup):
    ts = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        orbx.pose_optimization([prob])
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e6)
    return p50(ts)


def device_problem(torch, cam, obs):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()
    n = len(obs["keys"])
    return dict(camera=cam, keys=t(np.ascontiguousarray(obs["keys"]).view(np.uint8).reshape(n, 28)),
                pos=t(obs["pos"]), uright=t(obs["uright"]),
                Tcw_out=torch.zeros(16, device="cuda"), outlier=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                ninliers=torch.zeros(1, dtype=torch.int32, device="cuda"),
                status=torch.zeros(1, dtype=torch.int32, device="cuda"))


def time_plan(orbx, torch, probs, nprob, iters, warmup):
    pbs = [device_problem(torch, *probs[i % len(probs)]) for i in range(nprob)]
    plan = orbx.PosePlan(nprob, max(len(p[1]["keys"]) for p in probs))
    ts = []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan.optimize(pbs)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b) * 1e3)
    return p50(ts), pbs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import orbx
    if orbx.device_count() < 1:
        raise SystemExit("pose_latency: no GPU visible")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for n in (200, 1000):
        probs = problems(n, DISTINCT)
        refs = [U.ref_optimize(c, o) for c, o in probs]
        (got,) = orbx.pose_optimization([probs[0]])
        assert U.same_bits(got[0], refs[0]["Tcw"]) and np.array_equal(got[1], refs[0]["outlier"])
        host = [time_host_form(orbx, torch, probs[0], args.iters, args.warmup) for _ in range(args.repeats)]
        emit(dict(case="host_form", n=n, nprob=1, p50_us=p50(host), repeats_us=host,
                  restatement_cpu_us=time_ref(probs[:1], 20), **work(refs[:1])))
    n = 1000
    probs = problems(n, DISTINCT)
    refs = [U.ref_optimize(c, o) for c, o in probs]
    cpu_us = time_ref(probs, 10)  # mean over the distinct scenes of the p50 of one problem
    for nprob in (1, 64, 256):
        res = [time_plan(orbx, torch, probs, nprob, args.iters, args.warmup) for _ in range(args.repeats)]
        ts = [r[0] for r in res]
        pbs = res[-1][1]
        for i in (0, nprob - 1):
            r = refs[i % len(refs)]
            assert U.same_bits(pbs[i]["Tcw_out"].cpu().numpy().reshape(4, 4), r["Tcw"])
            assert int(pbs[i]["ninliers"].cpu()[0]) == r["ninliers"]
        used = [refs[i % len(refs)] for i in range(nprob)]
        emit(dict(case="plan_form", n=n, nprob=nprob, p50_us=p50(ts), repeats_us=ts, per_problem_us=p50(ts) / nprob,
                  restatement_cpu_us_per_problem=cpu_us, restatement_cpu_us_batch=cpu_us * nprob, **work(used)))
    # does the time follow n (throughput) or the trial count (latency)?  one problem each
    for n in (64, 256, 1024, 4096, 8192):
        probs = problems(n, 4)
        refs = [U.ref_optimize(c, o) for c, o in probs]
        for (c, o), r in zip(probs, refs):
            t, _ = time_plan(orbx, torch, [(c, o)], 1, max(args.iters // 4, 10), args.warmup)
            trials = r["counters"]["accepted"] + r["counters"]["rejected"]
            emit(dict(case="scaling", n=n, nprob=1, p50_us=t, trials=trials, us_per_trial=t / max(trials, 1)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/pose_latency.py", iters=args.iters, warmup=args.warmup, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
