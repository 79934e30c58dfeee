#!/usr/bin/env python3
"""Times the variance-guided denoising passes on one GPU.

    python3 tools/svgf_bench.py [--config C3] [--size 1920x1080] [--windows 25] [--reps 10] [--out FILE]

HIP events on the current stream around `reps` back-to-back calls, the median over `windows` such windows after a
warm-up, per call (tools/temporal_bench.py's method).  Measured on one frame of the config with a static camera
and a history: the moments instance of temporal_kernel beside the plain one; variance_kernel with every hit pixel
on the spatial branch (min_history above every length) and with none (min_history 1); one iteration of the
variance-guided filter beside one iteration of the plain a-trous filter (each the difference of a 2- and a
1-iteration chain); and a fill of the bytes each of the two memory-bound passes must move."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# per pixel.  temporal (C26): tools/temporal_bench.py's count; the moments instance adds the albedo, four taps'
# moments and the moments written.  variance, temporal branch: depth, length, moments read, one float written
TEMPORAL_BYTES = (16 + 16 + 4 + 4) + (16 + 16 + 4 + 4 + 4) + (16 + 4)
MOMENTS_BYTES = TEMPORAL_BYTES + 16 + 8 + 8
VARIANCE_BYTES = 4 + 4 + 8 + 4


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
    from octree_pathtracing_amd.renderer import LUMINANCE_FLOOR, HipRenderer, _c_camera

    W, H = map(int, args.size.split("x"))
    n = W * H
    sc, cam, rs = S.make_config(args.config)
    stream = torch.cuda.current_stream().cuda_stream
    res = {"config": args.config, "width": W, "height": H, "windows": args.windows, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    r = HipRenderer(device=0)
    r.set_scene(sc)
    r.max_depth, r.seed = rs.max_depth, rs.seed
    r.set_camera(cam)
    # an 8-spp colour and the guides, on the device
    f = {"albedo": torch.zeros((n, 4), device="cuda"), "normal": torch.zeros((n, 4), device="cuda"),
         "depth": torch.zeros(n, device="cuda"), "prim": torch.zeros(n, dtype=torch.int32, device="cuda")}
    r.render_aov_device(r.params(W, H, 0, 0), {k: v.data_ptr() for k, v in f.items()}, stream)
    color = torch.zeros((n, 4), device="cuda")
    color[:, 3] = 1.0
    r.render_device(r.params(W, H, 0, 8), color.data_ptr(), None, stream)
    torch.cuda.synchronize()
    res["hit_fraction"] = float(torch.isfinite(f["depth"]).float().mean())

    out, out_len = torch.zeros((n, 4), device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    out_m = torch.zeros((n, 2), device="cuda")
    h_color, h_len = torch.zeros((n, 4), device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    h_m = torch.zeros((n, 2), device="cuda")
    guides = {k: f[k].data_ptr() for k in ("normal", "depth", "prim", "albedo")}
    plain_guides = {k: f[k].data_ptr() for k in ("normal", "depth", "prim")}
    flags = _lib.TEMPORAL_MATCH_PRIM | _lib.TEMPORAL_DEMODULATE
    pm = _lib.TemporalParams(W, H, _c_camera(cam), _c_camera(cam), 32, 0.1, 0.9, flags)
    pt = _lib.TemporalParams(W, H, _c_camera(cam), _c_camera(cam), 32, 0.1, 0.9, _lib.TEMPORAL_MATCH_PRIM)
    # the history: the first frame (lengths 1 on hits)
    r.temporal_moments_device(pm, color.data_ptr(), guides, None, None, h_color.data_ptr(), h_len.data_ptr(),
                              h_m.data_ptr(), stream)
    torch.cuda.synchronize()
    prev = dict(plain_guides, color=h_color.data_ptr(), length=h_len.data_ptr())
    res["temporal_moments"] = timed(torch, lambda: r.temporal_moments_device(
        pm, color.data_ptr(), guides, prev, h_m.data_ptr(), out.data_ptr(), out_len.data_ptr(), out_m.data_ptr(), stream),
        args.windows, args.reps)
    res["temporal_plain"] = timed(torch, lambda: r.temporal_device(
        pt, color.data_ptr(), plain_guides, prev, out.data_ptr(), out_len.data_ptr(), stream), args.windows, args.reps)
    torch.cuda.synchronize()
    res["with_history_fraction"] = float((out_len > 1).float().mean())

    # variance on the blended frame (lengths 2 on hits): every hit pixel spatial, and none
    var = torch.zeros(n, device="cuda")
    ng = {k: f[k].data_ptr() for k in ("normal", "depth")}
    for name, min_history in (("variance_all_spatial", 4), ("variance_none_spatial", 1)):
        pv = _lib.VarianceParams(W, H, min_history, 0.3, 0.1)
        res[name] = timed(torch, lambda: r.variance_device(pv, out_m.data_ptr(), out_len.data_ptr(), ng, var.data_ptr(),
                                                           stream), args.windows, args.reps)
    pv = _lib.VarianceParams(W, H, 4, 0.3, 0.1)
    r.variance_device(pv, out_m.data_ptr(), out_len.data_ptr(), ng, var.data_ptr(), stream)
    torch.cuda.synchronize()

    dn = {k: f[k].data_ptr() for k in ("albedo", "normal", "depth")}
    filt, filt_v = torch.zeros((n, 4), device="cuda"), torch.zeros(n, device="cuda")
    for k in (1, 2):
        p = _lib.DenoiseVarianceParams(W, H, k, 4.0, LUMINANCE_FLOOR, 0.3, 0.1, _lib.DENOISE_DEMODULATE)
        res[f"denoise_variance_{k}it"] = timed(torch, lambda: r.denoise_variance_device(
            p, out.data_ptr(), var.data_ptr(), dn, filt.data_ptr(), filt_v.data_ptr(), stream), args.windows, args.reps)
        q = _lib.DenoiseParams(W, H, k, 0.6, 0.3, 0.1, _lib.DENOISE_DEMODULATE)
        res[f"denoise_{k}it"] = timed(torch, lambda: r.denoise_device(q, out.data_ptr(), dn, filt.data_ptr(), stream),
                                      args.windows, args.reps)
    res["atrous_var_iteration_ms"] = res["denoise_variance_2it"]["median_ms"] - res["denoise_variance_1it"]["median_ms"]
    res["atrous_iteration_ms"] = res["denoise_2it"]["median_ms"] - res["denoise_1it"]["median_ms"]

    for name, bpp in (("temporal_plain", TEMPORAL_BYTES), ("temporal_moments", MOMENTS_BYTES),
                      ("variance_none_spatial", VARIANCE_BYTES)):
        buf = torch.zeros(n * bpp // 4, dtype=torch.int32, device="cuda")
        res[f"fill_{name}_bytes"] = timed(torch, lambda: buf.fill_(1), args.windows, args.reps)
        res[f"{name}_bytes_per_call"] = n * bpp
        res[f"{name}_GBps"] = n * bpp / res[name]["median_ms"] / 1e6
    r.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
