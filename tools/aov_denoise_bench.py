#!/usr/bin/env python3
"""Times the guide-buffer pass and the a-trous denoiser on one GPU.

    python3 tools/aov_denoise_bench.py [--config C3] [--size 1920x1080] [--windows 25] [--reps 10]
                                       [--lib-b PATH] [--out FILE]

HIP events on the current stream around `reps` back-to-back calls; the figure is the median over `windows`
such windows after a warm-up, per call.  Measured: preview_kernel (the yardstick), gbuffer_kernel with all
five outputs and with depth only, a fill of the five buffers (the time 44 B of stores per pixel take at the
write bandwidth), and the denoiser for 1..5 iterations: iteration i's time is the difference of two chain
lengths, iteration 0's includes the prep pass.  --lib-b: another build of the library (same ABI) whose
guide-buffer pass and denoiser are timed alternately with the default build's (A/B of launch bounds or of a
variant from tools/rejected)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


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
    ap.add_argument("--lib-b", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing measured")
    from octree_pathtracing_amd import _lib
    from octree_pathtracing_amd import scene as S
    from octree_pathtracing_amd.renderer import HipRenderer

    W, H = map(int, args.size.split("x"))
    n = W * H
    sc, cam, rs = S.make_config(args.config)
    rs.width, rs.height, rs.spp = W, H, 8
    stream = torch.cuda.current_stream().cuda_stream
    res = {"config": args.config, "width": W, "height": H, "windows": args.windows, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    def renderer(lib_path=None):
        r = HipRenderer(device=0, lib_path=lib_path)
        r.set_scene(sc)
        r.set_camera(cam)
        return r

    builds = [("a", renderer())]
    if args.lib_b:
        builds.append(("b", renderer(args.lib_b)))
    r = builds[0][1]
    acc = torch.zeros((n, 4), device="cuda")
    acc[:, 3] = 1.0
    t = {"albedo": torch.zeros((n, 4), device="cuda"), "normal": torch.zeros((n, 4), device="cuda"),
         "depth": torch.zeros(n, device="cuda"), "prim": torch.zeros(n, dtype=torch.int32, device="cuda"),
         "material": torch.zeros(n, dtype=torch.int32, device="cuda")}
    all5 = {k: v.data_ptr() for k, v in t.items()}
    p_prev = r.params(W, H, 0, 0, preview=True)
    p_aov = r.params(W, H, 0, 0)
    res["preview"] = timed(torch, lambda: r.render_device(p_prev, acc.data_ptr(), None, stream), args.windows, args.reps)
    res["fill_44B_per_pixel"] = timed(torch, lambda: [v.fill_(1) for v in t.values()], args.windows, args.reps)
    for rnd in range(2):  # alternate the builds
        for tag, rr in builds:
            res[f"gbuffer_all5_{tag}{rnd}"] = timed(torch, lambda: rr.render_aov_device(p_aov, all5, stream),
                                                    args.windows, args.reps)
            res[f"gbuffer_depth_only_{tag}{rnd}"] = timed(
                torch, lambda: rr.render_aov_device(p_aov, {"depth": all5["depth"]}, stream), args.windows, args.reps)

    # denoiser input: an 8-spp render and its guides
    r.render_aov_device(p_aov, all5, stream)
    color = torch.zeros((n, 4), device="cuda")
    color[:, 3] = 1.0
    r.max_depth, r.seed = rs.max_depth, rs.seed
    r.render_device(r.params(W, H, 0, rs.spp), color.data_ptr(), None, stream)
    torch.cuda.synchronize()
    out = torch.zeros_like(color)
    guides = {k: all5[k] for k in ("albedo", "normal", "depth")}
    res["hit_fraction"] = float(torch.isfinite(t["depth"]).float().mean())
    check = {}
    for tag, rr in builds:
        p = _lib.DenoiseParams(W, H, 5, 0.6, 0.3, 0.1, _lib.DENOISE_DEMODULATE)
        rr.denoise_device(p, color.data_ptr(), guides, out.data_ptr(), stream)
        torch.cuda.synchronize()
        check[tag] = out.clone()
    if "b" in check:
        res["denoise_b_equals_a_bitwise"] = bool(torch.equal(check["a"].view(torch.int32), check["b"].view(torch.int32)))
    for rnd in range(2):
        for tag, rr in builds:
            for k in range(1, 6):
                p = _lib.DenoiseParams(W, H, k, 0.6, 0.3, 0.1, _lib.DENOISE_DEMODULATE)
                res[f"denoise_{tag}_{k}it_r{rnd}"] = timed(
                    torch, lambda: rr.denoise_device(p, color.data_ptr(), guides, out.data_ptr(), stream),
                    args.windows, args.reps)
    # bytes an iteration must move: signal + normal + depth read, signal written, once over the frame; and
    # the same with every one of the 25 taps counted (what the caches absorb)
    res["denoise_bytes_per_iteration_min"] = n * (16 + 16 + 4 + 16)
    res["denoise_bytes_per_iteration_25taps"] = n * (25 * (16 + 16 + 4) + 16)
    for tag, _ in builds:
        for k in range(1, 6):
            cur = min(res[f"denoise_{tag}_{k}it_r{q}"]["median_ms"] for q in range(2))
            prev = min(res[f"denoise_{tag}_{k - 1}it_r{q}"]["median_ms"] for q in range(2)) if k > 1 else 0.0
            ms = cur - prev
            res[f"denoise_{tag}_iteration{k - 1}_ms"] = ms
            res[f"denoise_{tag}_iteration{k - 1}_GBps_min_bytes"] = res["denoise_bytes_per_iteration_min"] / ms / 1e6
    for _, rr in builds:
        rr.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
