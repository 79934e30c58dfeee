#!/usr/bin/env python3
"""Refill-policy estimate for a grouped chunk's first extend launch (diagnostic; a record, not a test).

tools/sample_group_estimate.py assumes that the 64 rays a wave starts with stay in step until the last one ends.
wf_extend_kernel refills instead: once `thr` lanes are idle, the idle lanes take the next positions of the wave's claim
of 64, and at G = 64 the next claim is the next pixel.  This replays the oracle's per-ray iteration trace (as
sample_group_estimate.py takes it) through that refill rule: one model wave per 8x8 tile walks the tile's 4096 camera
rays at 64 samples in the item order of G (64 claims of 64 positions), and per threshold it prints

  lanes       the mean number of lanes holding a ray per wave iteration (of 64)
  kinds/step  the mean number of distinct iteration kinds (descend, advance, pop, leaf) among those lanes: the branch
              regions one wave iteration has to issue
  steps/ray   wave iterations per ray
  cost        steps/ray x kinds/step, the region executions per ray, and its ratio to thr = 16

The refill is the kernel's: it happens when at least thr lanes are idle, hands out at most what the owned claim still
holds (a claim that runs out is followed by the next at the following test), and after the last claim the wave runs
until every lane is idle.  thr = 16 is today's rule for C3's long rays.  Not modelled: the beam start, the folds, the
waves that share a segment (a wave's next claim is really a pixel some claims further on), the launch's tail.
A direction, not a forecast.

usage: tools/group_refill_estimate.py [CONFIG] [STRIPS] [TILE_STRIDE]
"""
import ctypes as C
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from sample_group_estimate import SPP, waves_of  # noqa: E402

GROUPS = [("1 px x 64 samples (G=64)", 6), ("2x2 px x 16 samples (G=16)", 4)]
THRESHOLDS = (16, 32, 48, 56, 60, 64)


def simulate(cls, start, length, thr):
    """One wave per row of start / length [tiles, rays in item order] -> (wave steps, lane steps, kind-region runs)."""
    n_w, n_r = start.shape
    rows = np.arange(n_w)
    ptr = np.zeros((n_w, 64), np.int64)
    rem = np.zeros((n_w, 64), np.int64)
    c_next = np.zeros(n_w, np.int64)
    steps = lanes = regions = 0
    while True:
        while True:
            idle = rem == 0
            n_idle = idle.sum(1)
            need = (c_next < n_r) & (n_idle >= thr)
            if not need.any():
                break
            w = rows[need]
            avail = 64 - (c_next[w] & 63)  # what the owned claim still holds; a new claim of 64 when it ran out
            rank = np.cumsum(idle[w], 1) - 1
            take = idle[w] & (rank < avail[:, None])
            r, l = np.nonzero(take)
            p = c_next[w][r] + rank[r, l]
            ptr[w[r], l] = start[w[r], p]
            rem[w[r], l] = length[w[r], p]
            c_next[w] += np.minimum(n_idle[w], avail)
        busy = rem > 0
        if not busy.any():
            return steps, lanes, regions
        k = np.where(busy, cls[ptr], 255)
        regions += int(sum((k == c).any(1).sum() for c in range(4)))
        steps += int(busy.any(1).sum())
        lanes += int(busy.sum())
        ptr += busy
        rem -= busy


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
    n_strips = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    stride = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    from octree_pathtracing_amd import scene as S
    from oracle import cpu_ref

    tmp = tempfile.mkdtemp(prefix="octpt_trace_")
    lib = Path(tmp) / "libcpu_ref_trace.so"
    subprocess.run(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-fPIC", "-ffp-contract=off", "-DREF_ESVO_TRACE",
                    "-shared", "-o", str(lib), str(ROOT / "oracle" / "cpu_ref.c"), "-lm", "-pthread"], check=True)
    L = cpu_ref.load(lib)
    L.ref_esvo_trace_set.argtypes = [C.c_void_p, C.c_size_t]
    L.ref_esvo_trace_len.restype = C.c_size_t
    sc, cam, rs = S.make_config(cfg)
    W, H = rs.width, rs.height
    cap = 8 * W * SPP * 256
    buf = np.zeros(cap, np.uint8)
    acc = {(name, thr): [0, 0, 0, 0] for name, _ in GROUPS for thr in THRESHOLDS}  # steps, lanes, regions, rays
    n_tiles = 0
    for k in range(n_strips):
        y0 = (((2 * k + 1) * H) // (2 * n_strips)) // 8 * 8
        L.ref_esvo_trace_set(buf.ctypes.data, cap)
        cpu_ref.render(sc, cam, W, H, SPP, max_depth=1, seed=rs.seed, threads=1, forward=True, rows=(y0, y0 + 8))
        n = L.ref_esvo_trace_len()
        assert n < cap, "trace buffer too small"
        t = buf[:n]
        cam_first = np.nonzero(((t & 16) != 0) & ((t & 32) == 0))[0]
        any_first = np.nonzero((t & 16) != 0)[0]
        assert len(cam_first) == 8 * W * SPP, (len(cam_first), 8 * W * SPP)
        nxt = np.append(any_first, n)[np.searchsorted(any_first, cam_first) + 1]
        lens = (nxt - cam_first).astype(np.int64).reshape(8, W, SPP)
        starts = cam_first.reshape(8, W, SPP)
        kind = t & 7
        cls = np.where(kind == 3, 0, np.where((kind == 1) | (kind == 2), 3, np.where((t & 8) != 0, 2, 1))).astype(np.uint8)
        cls = np.append(cls, np.uint8(255))  # a lane's pointer one past its last iteration
        tiles = range(0, W // 8, stride)
        n_tiles += len(tiles)
        for name, g in GROUPS:
            st = np.stack([waves_of(starts[:, tx * 8:tx * 8 + 8, :], g).reshape(-1) for tx in tiles])
            ln = np.stack([waves_of(lens[:, tx * 8:tx * 8 + 8, :], g).reshape(-1) for tx in tiles])
            for thr in THRESHOLDS:
                s, la, rg = simulate(cls, st, ln, thr)
                a = acc[(name, thr)]
                a[0] += s
                a[1] += la
                a[2] += rg
                a[3] += st.size
        print(f"strip {k}: rows {y0}..{y0 + 7}, {n} iterations, {n / len(cam_first):.1f} per camera ray", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    print(f"{cfg} {W}x{H}, camera rays, {SPP} samples, {n_tiles} 8x8 tiles on {n_strips} strips; the reference's iterations;")
    print("one model wave per tile, 64 claims of 64 positions each")
    for name, _ in GROUPS:
        print(f"\n{name}")
        print(f"{'thr':>4s} {'lanes':>7s} {'kinds/step':>11s} {'steps/ray':>10s} {'cost':>7s} {'vs thr 16':>10s}")
        base = acc[(name, 16)][2] / acc[(name, 16)][3]
        for thr in THRESHOLDS:
            s, la, rg, rays = acc[(name, thr)]
            print(f"{thr:4d} {la / s:7.2f} {rg / s:11.3f} {s / rays:10.3f} {rg / rays:7.3f} {rg / rays / base:10.3f}")


if __name__ == "__main__":
    main()
