#!/usr/bin/env python3
"""Times the temporal reprojection pass on one GPU.

    python3 tools/temporal_bench.py [--config C3] [--size 1920x1080] [--windows 25] [--reps 10] [--out FILE]

HIP events on the current stream around `reps` back-to-back calls, the median over `windows` such windows after a
warm-up, per call (tools/aov_denoise_bench.py's method).  Measured: temporal_kernel on a frame of the config with
a static camera, with the camera yawed by 0.05 rad and translated, and on a first frame (no history); for scale,
one a-trous iteration on the same frame (the difference of a 2- and a 1-iteration chain), a fill of the bytes the
pass must move and a device copy moving the same bytes (half read, half written)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# per pixel: colour, normal, depth, prim of the frame; colour, normal, depth, prim, length of the history;
# colour and length written
READ_BYTES, WRITE_BYTES = (16 + 16 + 4 + 4) + (16 + 16 + 4 + 4 + 4), 16 + 4


def timed(torch, fn, windows, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--windows", type=int, default=25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing measured")
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer, _c_camera
    from octree_pathtracing_amd.scene import Camera

    W, H = map(int, args.size.split("x"))
    n = W * H
    sc, cam0, rs = S.make_config(args.config)
    d, u = np.asarray(cam0.direction, np.float64), np.asarray(cam0.up, np.float64)
    right = np.cross(d, u)
    eye = np.asarray(cam0.eye, np.float64) + 8.0 * right - 3.0 * u + 5.0 * d
    cam1 = Camera.look_at(tuple(eye), tuple(eye + np.cos(0.05) * d + np.sin(0.05) * right), up=tuple(u))
    cam1.fov = cam0.fov
    stream = torch.cuda.current_stream().cuda_stream
    res = {"config": args.config, "width": W, "height": H, "windows": args.windows, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    r = HipRenderer(device=0)
    r.set_scene(sc)
    r.max_depth, r.seed = rs.max_depth, rs.seed

    def frame(cam):
        """An 8-spp colour and the guides at `cam`, on the device."""
        r.set_camera(cam)
        t = {"albedo": torch.zeros((n, 4), device="cuda"), "normal": torch.zeros((n, 4), device="cuda"),
             "depth": torch.zeros(n, device="cuda"), "prim": torch.zeros(n, dtype=torch.int32, device="cuda")}
        r.render_aov_device(r.params(W, H, 0, 0), {k: v.data_ptr() for k, v in t.items()}, stream)
        t["color"] = torch.zeros((n, 4), device="cuda")
        t["color"][:, 3] = 1.0
        r.render_device(r.params(W, H, 0, 8), t["color"].data_ptr(), None, stream)
        torch.cuda.synchronize()
        return t

    f0, f1 = frame(cam0), frame(cam1)
    res["hit_fraction"] = float(torch.isfinite(f0["depth"]).float().mean())
    out = torch.zeros((n, 4), device="cuda")
    out_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    h_color, h_len = torch.zeros((n, 4), device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")

    def params(cam):
        return _lib.TemporalParams(W, H, _c_camera(cam), _c_camera(cam0), 32, 0.1, 0.9, _lib.TEMPORAL_MATCH_PRIM)

    def guides(f):
        return {k: f[k].data_ptr() for k in ("normal", "depth", "prim")}

    # the history: the first frame at cam0
    r.temporal_device(params(cam0), f0["color"].data_ptr(), guides(f0), None, h_color.data_ptr(), h_len.data_ptr(), stream)
    torch.cuda.synchronize()
    prev = dict(guides(f0), color=h_color.data_ptr(), length=h_len.data_ptr())
    for name, f, cam, hist in (("static", f0, cam0, prev), ("moved", f1, cam1, prev), ("first_frame", f0, cam0, None)):
        p = params(cam)
        res[f"temporal_{name}"] = timed(
            torch, lambda: r.temporal_device(p, f["color"].data_ptr(), guides(f), hist, out.data_ptr(),
                                             out_len.data_ptr(), stream), args.windows, args.reps)
        torch.cuda.synchronize()
        res[f"temporal_{name}_with_history_fraction"] = float((out_len > 1).float().mean())
    dn = {k: f0[k].data_ptr() for k in ("albedo", "normal", "depth")}
    for k in (1, 2):
        p = _lib.DenoiseParams(W, H, k, 0.6, 0.3, 0.1, _lib.DENOISE_DEMODULATE)
        res[f"denoise_{k}it"] = timed(torch, lambda: r.denoise_device(p, f0["color"].data_ptr(), dn, out.data_ptr(), stream),
                                      args.windows, args.reps)
    res["atrous_iteration_ms"] = res["denoise_2it"]["median_ms"] - res["denoise_1it"]["median_ms"]
    moved_bytes = n * (READ_BYTES + WRITE_BYTES)
    res["temporal_bytes_per_call"] = moved_bytes
    buf = torch.zeros(moved_bytes // 4, dtype=torch.int32, device="cuda")
    res["fill_same_bytes"] = timed(torch, lambda: buf.fill_(1), args.windows, args.reps)
    half = moved_bytes // 8
    res["copy_same_bytes"] = timed(torch, lambda: buf[:half].copy_(buf[half:2 * half]), args.windows, args.reps)
    for k in ("temporal_static", "temporal_moved", "fill_same_bytes", "copy_same_bytes"):
        res[f"{k}_GBps"] = moved_bytes / res[k]["median_ms"] / 1e6
    r.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
