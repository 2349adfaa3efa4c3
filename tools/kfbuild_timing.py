"""Timing of the keyframe projection: orbm_kf_plan_project_search
on device tensors against the route it replaces -- the query rows built on the
host (the C restatement of tests/cpp/kfbuild_ref.c), the live ones handed to
the synchronous orbm_keyframe_search -- at a LocalMapping::SearchInNeighbors
shape (20 keyframes x 2000 shared map points, 2000 features each) and at one
SearchBySim3 pair.  Host clock around work that ends with the results usable
(a device synchronise for the plan's call; orbm_keyframe_search is
synchronous), and device events around the plan's call alone; p50 over --iters
calls after --warmup.  Prints one JSON line per case.  Needs a GPU."""
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

import kfbuild_util as U  # noqa: E402
import kfwindow_util as KW  # noqa: E402


def keyframe(form, cam, P, qdesc, nfeat, seed):
    """nfeat features around the projections of the restatement's live rows"""
    r = U.ref_project(form, cam, P, U.TH[form])
    rng = np.random.default_rng(seed)
    live = np.nonzero(r["branch"] == 0)[0]
    src = rng.choice(live, nfeat)
    q = r["q"][src]
    flip = rng.integers(0, 256, (nfeat, 32)).astype(np.uint8) & rng.integers(0, 256, (nfeat, 32)).astype(np.uint8) \
        & rng.integers(0, 256, (nfeat, 32)).astype(np.uint8)  # about an eighth of the bits
    keys = KW.make_keys((q["x"] + rng.uniform(-4, 4, nfeat)).astype(np.float32),
                        (q["y"] + rng.uniform(-4, 4, nfeat)).astype(np.float32),
                        np.clip(q["level"] - rng.integers(0, 2, nfeat), 0, 7).astype(np.int32))
    return KW.frame_dict(keys, qdesc[src] ^ flip)


def p50(v):
    return float(np.percentile(np.asarray(v), 50))


def host_timed(torch, fn, iters, warmup):
    out = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return p50(out)


def event_timed(torch, fn, iters, warmup):
    out = []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b) * 1e3)
    return p50(out)


def run(orbx, torch, name, form, nkf, npts, nfeat, iters, warmup):
    t = lambda a: torch.from_numpy(np.array(a, copy=True)).cuda()
    _, P = U.random_scene(form, npts, 600 + form)  # one point set, shared by every keyframe
    rng = np.random.default_rng(9)
    qdesc = rng.integers(0, 256, (npts, 32)).astype(np.uint8)
    cams = [U.random_camera(form, 600 + form)] + [U.random_camera(form, 700 + i) for i in range(1, nkf)]
    # the later cameras see the shared points from elsewhere: fewer live rows, as in SearchInNeighbors
    kfs = [keyframe(form, cams[0], P, qdesc, nfeat, 50 + i) for i in range(nkf)]
    pts, pool = {k: t(v) for k, v in P.items()}, t(qdesc)
    probs = []
    for cam, kf in zip(cams, kfs):
        probs.append(dict(camera=orbx.kf_camera(cam), points=pts, npts=npts, qdesc=pool,
                          frame=dict(keys=t(kf["keys"].view(np.uint8).reshape(nfeat, 28)), desc=t(kf["desc"]),
                                     min_x=kf["min_x"], min_y=kf["min_y"], grid_w_inv=kf["grid_w_inv"],
                                     grid_h_inv=kf["grid_h_inv"]),
                          n_live=torch.zeros(1, dtype=torch.int32, device="cuda"),
                          best_idx=torch.zeros(npts, dtype=torch.int32, device="cuda"),
                          best_dist=torch.zeros(npts, dtype=torch.int32, device="cuda")))
    plan = orbx.KeyframePlan(nkf, nfeat, npts)
    last = {}

    def host_route():  # the parent commit's: project on the host, search the live rows
        rows, keep = [], []
        for cam in cams:
            r = U.ref_project(form, cam, P, U.TH[form])
            k = np.nonzero(r["level"] >= 0)[0]
            rows.append(r["q"][k])
            keep.append(k)
        last["res"], last["keep"] = orbx.keyframe_search(kfs, rows, qdesc), keep

    res = dict(case=name, form=form, nkf=nkf, npts=npts, nfeat=nfeat, iters=iters)
    res["project_search_us_p50"] = host_timed(torch, lambda: plan.project_search(form, probs, th=U.TH[form]), iters,
                                              warmup)
    res["project_search_device_us_p50"] = event_timed(torch, lambda: plan.project_search(form, probs, th=U.TH[form]),
                                                     iters, warmup)
    res["host_route_us_p50"] = host_timed(torch, host_route, iters, warmup)
    torch.cuda.synchronize()
    agree = True
    for pb, (bi, bd), k in zip(probs, last["res"], last["keep"]):
        gi, gd = pb["best_idx"].cpu().numpy(), pb["best_dist"].cpu().numpy()
        inert = np.ones(npts, bool)
        inert[k] = False
        agree &= bool(np.array_equal(gi[k], bi) and np.array_equal(gd[k], bd) and (gi[inert] == -1).all())
    res["routes_agree"] = agree
    res["live_share"] = float(np.mean([len(k) / npts for k in last["keep"]]))
    res["matched_share_kf0"] = float((last["res"][0][1] <= 50).mean())
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    import orbx
    if orbx.device_count() < 1:
        raise SystemExit("no GPU visible")
    run(orbx, torch, "search_in_neighbors", U.FUSE, 20, 2000, 2000, a.iters, a.warmup)
    run(orbx, torch, "search_by_sim3_pair", U.SIM3, 1, 2000, 2000, a.iters, a.warmup)


if __name__ == "__main__":
    main()
