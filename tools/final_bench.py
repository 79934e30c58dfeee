#!/usr/bin/env python3
"""Measures the finished-frame chain beside the plain adaptive render of the same build.

    python3 tools/final_bench.py [--config C3] [--size 1920x1080] [--max-spp 64] [--min-spp 16] [--step-spp 16]
                                 [--weight 0.5] [--reps 3] [--out FILE]

Wall time (host clock around the call and a device synchronisation, the median of `reps` after one warm-up) of
octpt_render_adaptive_device, of octpt_render_adaptive_ex_device at `weight` and of octpt_render_final_device (weight,
3 filter iterations, demodulated), with each driver's rounds and tile samples; and of one octpt_tile_error_spread_device
and one octpt_sample_variance_device launch, timed the same way over 100 repetitions.  The threshold is the median of
the tiles' finite errors after min-spp samples."""
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
    ap.add_argument("--max-spp", type=int, default=64)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step-spp", type=int, default=16)
    ap.add_argument("--weight", type=float, default=0.5)
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
    out = torch.zeros((n, 4), device="cuda")
    var = torch.zeros(n, device="cuda")
    err = torch.zeros(T, device="cuda")
    spread = torch.zeros(T, device="cuda")
    guides = {"albedo": torch.zeros((n, 4), device="cuda"), "depth": torch.zeros(n, device="cuda")}
    res = {"config": args.config, "width": W, "height": H, "tiles": T, "max_spp": args.max_spp,
           "min_spp": args.min_spp, "step_spp": args.step_spp, "weight": args.weight, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    def wall(fn, reps):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ret = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}, ret

    # the tiles' errors after the first round, and the two new kernels on that frame
    p = r.params(W, H, 0, args.max_spp)
    r.render_tiles_device(r.params(W, H, 0, args.min_spp), None, acc.data_ptr(), mom.data_ptr())
    spp = torch.full((T,), args.min_spp, dtype=torch.int32, device="cuda")
    r.tile_error_device(_lib.TileErrorParams(W, H, LUMINANCE_FLOOR), mom.data_ptr(), spp.data_ptr(), err.data_ptr())
    r.render_aov_device(p, {k: v.data_ptr() for k, v in guides.items()})
    torch.cuda.synchronize()
    e0 = err.cpu().numpy()
    threshold = float(np.median(e0[np.isfinite(e0)]))
    res["threshold"] = threshold
    res["tile_error_spread"], _ = wall(
        lambda: r.tile_error_spread_device(W, H, args.weight, err.data_ptr(), spread.data_ptr()), 100)
    pv = _lib.SampleVarianceParams(W, H, _lib.DENOISE_DEMODULATE)
    res["sample_variance"], _ = wall(
        lambda: r.sample_variance_device(pv, mom.data_ptr(), spp.data_ptr(), {k: v.data_ptr() for k, v in guides.items()},
                                         var.data_ptr()), 100)

    plain = _lib.AdaptiveParams(args.min_spp, args.step_spp, threshold, LUMINANCE_FLOOR)
    t, (_, result) = wall(lambda: r.render_adaptive_device(p, plain, acc.data_ptr(), mom.data_ptr()), args.reps)
    res["render_adaptive"] = dict(t, **result)
    ex = _lib.AdaptiveParamsEx(args.min_spp, args.step_spp, threshold, LUMINANCE_FLOOR, args.weight)
    t, (_, result) = wall(lambda: r.render_adaptive_ex_device(p, ex, acc.data_ptr(), mom.data_ptr()), args.reps)
    res["render_adaptive_ex"] = dict(t, **result)
    fp = _lib.FinalParams(ex, _lib.DenoiseVarianceParams(W, H, 3, 4.0, LUMINANCE_FLOOR, 0.3, 0.1, _lib.DENOISE_DEMODULATE))
    t, (_, result) = wall(lambda: r.render_final_device(p, fp, acc.data_ptr(), mom.data_ptr(), out.data_ptr(),
                                                        var.data_ptr()), args.reps)
    res["render_final"] = dict(t, **result)
    r.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
