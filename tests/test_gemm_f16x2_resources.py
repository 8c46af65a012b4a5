"""Registers, scratch and occupancy of every gemm_f16x2_pp_kernel instantiation, read from the gfx950 listing of csrc/gemm_f16x2.hip
(the Makefile's flags plus -S --cuda-device-only, as tests/test_abi.py builds its listings).  CPU only.

The kernel runs eight waves per workgroup, two per SIMD, on 144 KiB (128 x 256 tile) or 96 KiB (128 x 128) of LDS: one workgroup per
CU.  Two waves per SIMD need at most 256 of the 512 unified registers each, and nothing may spill: the epilogue holds every operand
quad of a wave's block next to the accumulators, so this is the budget a change to it can break.  Occupancy by registers is
floor(512 / registers rounded up to the granule of 8): 2 for the wide tile and 3 for the narrow one, as before the epilogue batched
its loads (238 / 246 and 150 registers then)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES_PER_SIMD = {"NJ=4": 2, "NJ=2": 3}
EXPECTED = {"bias NJ=2", "bias NJ=4", "resid NJ=2", "resid NJ=4", "gate NJ=4", "gate-state NJ=4", "state NJ=2", "state NJ=4"}


def test_tiled_kernels_keep_registers_scratch_and_occupancy(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the listing checks need the compiler")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gemm_edge_waits
    out = str(tmp_path / "gemm_f16x2.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-S", "--cuda-device-only",
                        "-o", out, "gemm_f16x2.hip"], cwd=os.path.join(ROOT, "d-vqvae_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for label, before, after, (vgpr, agpr, scratch) in gemm_edge_waits.kernels(open(out).read()):
        regs = int(vgpr) + int(agpr)
        seen[label] = regs
        assert int(scratch) == 0, f"{label}: {scratch} bytes of scratch"
        assert regs <= 256, f"{label}: {regs} registers, two waves per SIMD need <= 256"
        assert 512 // ((regs + 7) // 8 * 8) == WAVES_PER_SIMD[label.split()[-1]], f"{label}: {regs} registers change the occupancy"
    assert set(seen) == EXPECTED, sorted(seen)
