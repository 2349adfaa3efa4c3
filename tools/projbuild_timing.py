"""Timing of the device-side projection: orbm_proj_plan_track
against the route it replaces -- the queries built on the host (the C
restatement of tests/cpp/projbuild_ref.c), uploaded, then orbm_proj_plan_search
-- plus the projection call alone and the search with and without the inert
rows.  Host clock around work that ends in a device synchronise for the two
routes, device events for the parts; p50 over --iters calls after --warmup.
Prints one JSON line per case.  Needs a GPU."""
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

import projbuild_util as U  # noqa: E402
import projection_util as PU  # noqa: E402

READS = {1: ("pos", "normal", "min_dist_inv", "max_dist_inv", "max_dist", "skip"),
         2: ("pos", "octave", "angle", "skip"), 3: ("pos", "max_dist", "angle", "skip")}
SEARCH = {1: dict(nnratio=0.8, th_dist=100, check_ori=False), 2: dict(nnratio=0.6, th_dist=100, check_ori=True)}
DISTINCT = 8  # scenes built; a batch cycles through them (outputs are per problem)


def scene(mode, npts, nfeat, seed):
    cam, P = U.random_scene(mode, npts, seed)
    r = U.ref_project(mode, cam, P, **U.MODE_ARGS[mode])
    rng = np.random.default_rng(seed + 1)
    live = np.nonzero(r["branch"] == 0)[0]
    qdesc = rng.integers(0, 256, (npts, 32)).astype(np.uint8)
    src = rng.choice(live, nfeat)
    q = r["q"][src]
    flip = rng.integers(0, 256, (nfeat, 32)).astype(np.uint8) & rng.integers(0, 256, (nfeat, 32)).astype(np.uint8) \
        & rng.integers(0, 256, (nfeat, 32)).astype(np.uint8)  # about an eighth of the bits
    fr = PU.make_frame(q["x"] + rng.uniform(-3, 3, nfeat), q["y"] + rng.uniform(-3, 3, nfeat), qdesc[src] ^ flip,
                       octave=np.clip(r["level"][src] + rng.integers(-1, 2, nfeat), 0, 7),
                       angle=np.mod(q["angle"] + rng.normal(0, 8, nfeat), 360),
                       uright=np.where(rng.uniform(size=nfeat) < 0.5, q["xr"], -1.0) if mode == 1 else None,
                       occupied=(rng.uniform(size=nfeat) < 0.1).astype(np.uint8), geom="plain")
    return cam, P, qdesc, fr, r, live


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


def run(orbx, torch, mode, npts, nfeat, nprob, iters, warmup):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()
    scenes = [scene(mode, npts, nfeat, 500 + 10 * mode + i) for i in range(min(nprob, DISTINCT))]
    kw = U.MODE_ARGS[mode]
    track, build, search_all, search_live, refs = [], [], [], [], []
    for i in range(nprob):
        cam, P, qdesc, fr, r, live = scenes[i % len(scenes)]
        frame = dict(keys=t(fr["keys"].view(np.uint8).reshape(nfeat, 28)), desc=t(fr["desc"]), uright=t(fr["uright"]),
                     occupied=t(fr["occupied"]), min_x=fr["min_x"], min_y=fr["min_y"], grid_w_inv=fr["grid_w_inv"],
                     grid_h_inv=fr["grid_h_inv"])
        out = lambda: dict(match=torch.full((nfeat,), -1, dtype=torch.int32, device="cuda"),
                           nmatches=torch.zeros(1, dtype=torch.int32, device="cuda"))
        pts = {k: t(P[k]) for k in READS[mode]}
        qrows = torch.zeros((npts, 28), dtype=torch.uint8, device="cuda")
        common = dict(camera=orbx.proj_camera(cam), points=pts, n_in_view=torch.zeros(1, dtype=torch.int32, device="cuda"),
                      n_nonfinite=torch.zeros(1, dtype=torch.int32, device="cuda"))
        track.append(dict(common, frame=frame, qdesc=t(qdesc), **out()))
        build.append(dict(common, q=qrows, level=torch.zeros(npts, dtype=torch.int32, device="cuda")))
        sa = dict(frame, q=qrows, qdesc=t(qdesc), **out())
        search_all.append(sa)
        search_live.append(dict(frame, q=t(np.ascontiguousarray(r["q"][live]).view(np.uint8).reshape(-1, 28)),
                                qdesc=t(qdesc[live]), **out()))
        refs.append((cam, {k: P[k] for k in READS[mode]}))
    plan = orbx.ProjPlan(nprob, nfeat, npts)
    pinned = torch.zeros((nprob, npts, 28), dtype=torch.uint8).pin_memory()
    dev_rows = torch.zeros((nprob, npts, 28), dtype=torch.uint8, device="cuda")
    host_probs = [dict(sa, q=dev_rows[i]) for i, sa in enumerate(search_all)]

    def host_route():  # the parent commit's: project on the host, one upload, search
        for i, (cam, P) in enumerate(refs):
            r = U.ref_project(mode, cam, P, **kw)
            pinned[i].numpy()[...] = r["q"].view(np.uint8).reshape(npts, 28)
        dev_rows.copy_(pinned, non_blocking=True)
        plan.search(mode, host_probs, **SEARCH[mode])

    res = dict(mode=mode, npts=npts, nfeat=nfeat, nprob=nprob, iters=iters,
               live_share=float(np.mean([len(s[5]) / npts for s in scenes])))
    res["track_us_p50"] = host_timed(torch, lambda: plan.track(mode, track, **kw, **SEARCH[mode]), iters, warmup)
    res["host_route_us_p50"] = host_timed(torch, host_route, max(iters // 4, 10), 3)
    res["project_call_device_us_p50"] = event_timed(torch, lambda: plan.project(mode, build, **kw), iters, warmup)
    plan.project(mode, build, **kw)  # the rows search_all reads
    res["search_with_inert_device_us_p50"] = event_timed(torch, lambda: plan.search(mode, search_all, **SEARCH[mode]),
                                                        iters, warmup)
    res["search_live_only_device_us_p50"] = event_timed(torch, lambda: plan.search(mode, search_live, **SEARCH[mode]),
                                                       iters, warmup)
    torch.cuda.synchronize()
    # the three routes agree (matches name map points; the live-only search names kept rows)
    a, b = track[0]["match"].cpu().numpy(), host_probs[0]["match"].cpu().numpy()
    live = scenes[0][5]
    c = search_live[0]["match"].cpu().numpy()
    res["routes_agree"] = bool(np.array_equal(a, b) and np.array_equal(a, np.where(c >= 0, live[np.maximum(c, 0)], -1)))
    res["nmatches"] = int(track[0]["nmatches"].cpu()[0])
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
    for mode, npts, nprob in ((1, 3000, 1), (1, 3000, 64), (2, 2000, 64)):
        run(orbx, torch, mode, npts, 2000, nprob, a.iters, a.warmup)


if __name__ == "__main__":
    main()
