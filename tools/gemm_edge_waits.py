"""Counts the vector-memory waits around the K loop of every gemm_f16x2_pp_kernel instantiation in a gfx950 listing of
csrc/gemm_f16x2.hip (the Makefile's flags plus `--cuda-device-only -S`): `s_waitcnt vmcnt` before the first and after the last
s_barrier, with the registers and scratch the listing declares.  CPU only.

    python tools/gemm_edge_waits.py listing.s [more.s ...]
"""
import os, re, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_barriers

EPI = {"0": "bias", "1": "resid", "2": "gate", "5": "state"}


def kernels(text):
    meta = {}
    for blk in text.split("- .agpr_count:")[1:]:
        g = lambda k: (re.search(rf"\.{k}:\s*(\S+)", blk) or [None, "?"])[1]
        meta[g("name")] = (g("vgpr_count"), blk.split()[0], g("private_segment_fixed_size"))
    for name, body in check_barriers.functions(text):
        m = re.search(r"gemm_f16x2_pp_kernelILi(\d+)ELi(\d+)ELb(\d)E", name)
        if not m:
            continue
        lines = [ln.split(";")[0].strip() for ln in body.splitlines()]
        bars = [i for i, ln in enumerate(lines) if ln.startswith("s_barrier")]
        waits = [i for i, ln in enumerate(lines) if ln.startswith("s_waitcnt") and "vmcnt" in ln]
        label = f"{EPI.get(m.group(1), m.group(1))}{'-state' if m.group(3) == '1' else ''} NJ={m.group(2)}"
        yield label, sum(i < bars[0] for i in waits), sum(i > bars[-1] for i in waits), meta.get(name, ("?", "?", "?"))


if __name__ == "__main__":
    for path in sys.argv[1:]:
        print(path)
        for label, before, after, (vgpr, agpr, scratch) in sorted(kernels(open(path).read())):
            print(f"  {label:18s} vmcnt waits before first barrier {before:3d}  after last barrier {after:3d}   vgpr {vgpr} agpr {agpr} scratch {scratch}")
