#!/usr/bin/env python3
"""What the thin lens costs: a config's frame with aperture 0 and with the lens on, on one GPU.

    python tools/lens_bench.py --config C3 [--spp 64] [--steps 3] [--warmup 1] [--pixels 3.0]

The lens focuses on the scene's centre (the point the config's camera looks at: eye + direction * the distance to
the octree's centre along it) with the aperture that gives a circle of confusion of --pixels pixels (diameter) at
half and at one and a half times that distance.  Per variant: the median step time (HIP events around each
render), Mrays/s (segments / time) and ESVO iterations per segment.  One JSON line per variant."""
import argparse
import json
import statistics
import sys
from dataclasses import replace
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pixels", type=float, default=3.0)
    ap.add_argument("--only", choices=["pinhole", "lens"], default=None)
    args = ap.parse_args()

    import torch

    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    sc, cam, rs = S.make_config(args.config)
    if args.spp:
        rs.spp = args.spp
    W, H = rs.width, rs.height
    # the scene's centre along the view: the octree spans [0, 2^depth)^3
    centre = np.full(3, 0.5 * (1 << sc.octree.depth))
    eye, d = np.asarray(cam.eye, np.float64), np.asarray(cam.direction, np.float64)
    fd = float(max((centre - eye) @ d, 1.0))
    # circle of confusion on the focal plane of a point at distance z: 2 a |z - fd| / z world units; a pixel there is
    # 2 fd tan(fov / 2) / max(W, H) world units.  At z = fd / 2 (and 3 fd / 2: a third of it) the diameter is 2 a.
    pixel = 2.0 * fd * np.tan(cam.fov / 2.0) / max(W, H)
    aperture = 0.5 * args.pixels * pixel
    lens = replace(cam, aperture=float(aperture), focal_distance=fd)
    variants = {"pinhole": replace(cam, aperture=0.0, focal_distance=0.0), "lens": lens}

    with HipRenderer(device=0) as r:
        r.set_scene(sc)
        r.max_depth, r.seed = rs.max_depth, rs.seed
        acc = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for name, c in variants.items():
            if args.only and name != args.only:
                continue
            r.set_camera(c)
            p = r.params(W, H, 0, rs.spp)
            times, st = [], None
            for i in range(args.warmup + args.steps):
                acc.zero_()
                acc[:, 3] = 1.0
                r.reset_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r.render_device(p, acc.data_ptr(), None, stream)
                e1.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times.append(e0.elapsed_time(e1))
                    st = r.stats()
            ms = statistics.median(times)
            print(json.dumps({"config": args.config, "variant": name, "frame": [W, H, rs.spp],
                              "aperture": c.aperture, "focal_distance": c.focal_distance,
                              "ms_per_step": round(ms, 3), "ms_all": [round(t, 3) for t in times],
                              "mrays_per_s": round(st["segments"] / ms / 1e3, 1),
                              "segments": st["segments"],
                              "esvo_steps_per_segment": round(st["esvo_steps"] / st["segments"], 3),
                              "beam_restarts": st["beam_restarts"],
                              "finite": bool(torch.isfinite(acc).all().item())}), flush=True)


if __name__ == "__main__":
    main()
