"""Resolve's wave-cooperative read of a grouped chunk's colour records (octpt_resolve_map.h, resolve_pixel_wide): the
lane -> (record, LDS slot) mapping, checked on the host for G in {4, 16, 64} and every batch size the kernel can use
(tools/resolve_map_check.cpp, built here with hipcc as host code and run on the CPU): every record of a wave's span
read exactly once, each record handed to the lane whose pixel owns it at its sample's position, no two lanes on one
LDS slot, and the 16-B reads free of bank conflicts.  On the GPU tests/test_gpu_resolve_wide.py compares the renders."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_resolve_map(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists() and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    exe = tmp_path / "resolve_map_check"
    subprocess.run([hipcc, "-O2", "-std=c++17", str(ROOT / "tools" / "resolve_map_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 mismatches" in p.stdout
