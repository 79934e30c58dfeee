#!/usr/bin/env python3
"""Measures an adaptive render beside the fixed-spp render of the same build.

    python3 tools/adaptive_bench.py [--config C3] [--size 1920x1080] [--max-spp 256] [--min-spp 16] [--step-spp 16]
                                    [--thresholds T1,T2] [--reps 3] [--out FILE]

Wall time (host clock around the call and a device synchronisation, the median of `reps` after one warm-up) of
octpt_render_device at max-spp and of octpt_render_adaptive_device at each threshold, with the driver's rounds and
tile samples; and the per-round overhead, one octpt_tile_error_device launch plus the read-back of one float per tile,
timed the same way over 100 repetitions.  Without --thresholds the two are the median of the tiles' finite errors
after min-spp samples, and half of it."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step-spp", type=int, default=16)
    ap.add_argument("--thresholds", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing measured")
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import LUMINANCE_FLOOR, HipRenderer, tile_count

    W, H = map(int, args.size.split("x"))
    n, T = W * H, tile_count(W, H)
    sc, cam, rs = S.make_config(args.config)
    r = HipRenderer(device=0)
    r.set_scene(sc)
    r.max_depth, r.seed = rs.max_depth, rs.seed
    r.set_camera(cam)
    acc = torch.zeros((n, 4), device="cuda")
    mom = torch.zeros((n, 2), device="cuda")
    err = torch.zeros(T, device="cuda")
    res = {"config": args.config, "width": W, "height": H, "tiles": T, "max_spp": args.max_spp,
           "min_spp": args.min_spp, "step_spp": args.step_spp, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    def wall(fn, reps):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}, out

    def fixed():
        acc.zero_()
        acc[:, 3] = 1.0
        r.render_device(r.params(W, H, 0, args.max_spp), acc.data_ptr(), None)

    res["fixed"], _ = wall(fixed, args.reps)

    # the tiles' errors after the first round, and the per-round overhead
    acc.zero_()
    mom.zero_()
    r.render_tiles_device(r.params(W, H, 0, args.min_spp), None, acc.data_ptr(), mom.data_ptr())
    spp = torch.full((T,), args.min_spp, dtype=torch.int32, device="cuda")
    pe = _lib.TileErrorParams(W, H, LUMINANCE_FLOOR)

    def round_overhead():
        r.tile_error_device(pe, mom.data_ptr(), spp.data_ptr(), err.data_ptr())
        return err.cpu().numpy()

    res["round_overhead"], e0 = wall(round_overhead, 100)
    finite = e0[np.isfinite(e0)]
    res["first_round_error"] = {"finite_tiles": int(finite.size), "min": float(finite.min()),
                                "median": float(np.median(finite)), "max": float(finite.max())}
    if args.thresholds:
        thresholds = [float(t) for t in args.thresholds.split(",")]
    else:
        thresholds = [float(np.median(finite)), float(np.median(finite)) / 2]

    res["adaptive"] = []
    for th in thresholds:
        a = _lib.AdaptiveParams(args.min_spp, args.step_spp, th, LUMINANCE_FLOOR)
        t, (tile_spp, result) = wall(lambda: r.render_adaptive_device(r.params(W, H, 0, args.max_spp), a, acc.data_ptr(),
                                                                      mom.data_ptr()), args.reps)
        res["adaptive"].append(dict(t, threshold=th, fixed_tile_samples=args.max_spp * T,
                                    sample_fraction=result["tile_samples"] / (args.max_spp * T),
                                    time_fraction=t["median_ms"] / res["fixed"]["median_ms"],
                                    tiles_at_cap=int((tile_spp == args.max_spp).sum()), **result))
    r.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
