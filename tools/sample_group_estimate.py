#!/usr/bin/env python3
"""Lockstep estimate for the chunk item order (diagnostic; a record, not a test).

Which camera rays share a wave decides how far the wave's lanes walk the octree in step.  This
takes the oracle's per-ray iteration trace (oracle/cpu_ref.c with -DREF_ESVO_TRACE, as
tools/esvo_trace.py does) for a config's camera rays on full-width strips of 8x8 tiles at 64
samples, groups the rays into waves of 64 as each candidate order would, and prints per order

  max/mean    the mean over waves of (max lane iteration count / mean lane iteration count):
              the lanes a wave that runs until its last ray ends leaves idle
  kinds/step  the mean, over the lockstep steps of all waves, of the distinct iteration kinds
              (descend, advance, pop, leaf) among the lanes still walking at that step: the
              branch regions one wave iteration has to issue

The reference's iterations are counted: no beam start, no folds.  A direction, not a forecast.

usage: tools/sample_group_estimate.py [CONFIG] [STRIPS] [TILE_STRIDE]
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

SPP = 64
# (name, log2 of the samples per wave); the pixel block of a wave is 8 >> (g / 2) pixels square
ORDERS = [("8x8 px x 1 sample (G=1)", 0), ("4x4 px x 4 samples (G=4)", 2), ("2x2 px x 16 samples (G=16)", 4),
          ("1 px x 64 samples (G=64)", 6)]


def waves_of(tile, g):
    """tile[y 8, x 8, s 64, ...] -> [wave 64, lane 64, ...] in the order of G = 1 << g."""
    h = g // 2
    nb, npx, G = 1 << h, 8 >> h, 1 << g
    t = tile.reshape((nb, npx, nb, npx, SPP // G, G) + tile.shape[3:])  # by py bx px sg si
    t = t.transpose((4, 0, 2, 1, 3, 5) + tuple(range(6, t.ndim)))       # sg by bx py px si
    return t.reshape((64, 64) + tile.shape[3:])


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
    # one byte per iteration of a strip's 8 * W * SPP camera rays; 256 per ray is twice C3's mean at its longest strip
    cap = 8 * W * SPP * 256
    buf = np.zeros(cap, np.uint8)
    acc = {name: [0.0, 0, 0.0, 0] for name, _ in ORDERS}  # sum of max/mean, waves, sum of kinds, steps
    n_tiles = 0
    for k in range(n_strips):
        y0 = (((2 * k + 1) * H) // (2 * n_strips)) // 8 * 8
        L.ref_esvo_trace_set(buf.ctypes.data, cap)
        # max_depth 1: camera rays only (path_trace stops before the first bounce)
        cpu_ref.render(sc, cam, W, H, SPP, max_depth=1, seed=rs.seed, threads=1, forward=True, rows=(y0, y0 + 8))
        n = L.ref_esvo_trace_len()
        assert n < cap, "trace buffer too small"
        t = buf[:n]
        cam_first = np.nonzero(((t & 16) != 0) & ((t & 32) == 0))[0]
        any_first = np.nonzero((t & 16) != 0)[0]
        assert len(cam_first) == 8 * W * SPP, (len(cam_first), 8 * W * SPP)
        # a camera ray's iterations end at the next ray's first one (a pass-through continuation is another ray)
        nxt = np.append(any_first, n)[np.searchsorted(any_first, cam_first) + 1]
        lens = (nxt - cam_first).astype(np.int64)
        kind = t & 7
        cls = np.where(kind == 3, 0, np.where((kind == 1) | (kind == 2), 3, np.where((t & 8) != 0, 2, 1))).astype(np.uint8)
        starts = cam_first.reshape(8, W, SPP)
        lens = lens.reshape(8, W, SPP)
        for tx in range(0, W // 8, stride):
            st = starts[:, tx * 8:tx * 8 + 8, :]
            ln = lens[:, tx * 8:tx * 8 + 8, :]
            m = int(ln.max())
            idx = st[..., None] + np.arange(m)
            seq = np.where(np.arange(m) < ln[..., None], cls[np.minimum(idx, n - 1)], 255).astype(np.uint8)
            n_tiles += 1
            for name, g in ORDERS:
                w_len = waves_of(ln, g).astype(np.float64)  # [wave, lane]
                w_seq = waves_of(seq, g)                    # [wave, lane, step]
                a = acc[name]
                a[0] += float(np.sum(w_len.max(1) / w_len.mean(1)))
                a[1] += 64
                kinds = sum((w_seq == c).any(1).astype(np.int64) for c in range(4))  # [wave, step]
                a[2] += float(kinds.sum())
                a[3] += int((kinds > 0).sum())
        print(f"strip {k}: rows {y0}..{y0 + 7}, {n} iterations, {n / len(cam_first):.1f} per camera ray", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    print(f"{cfg} {W}x{H}, camera rays, {SPP} samples, {n_tiles} 8x8 tiles on {n_strips} strips; the reference's iterations")
    print(f"{'wave':30s} {'max/mean':>9s} {'kinds/step':>11s}")
    for name, _ in ORDERS:
        a = acc[name]
        print(f"{name:30s} {a[0] / a[1]:9.3f} {a[2] / a[3]:11.3f}")


if __name__ == "__main__":
    main()
