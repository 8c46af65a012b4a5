"""The K loop of every gemm_f16x2_pp_kernel instantiation, read from the gfx950 listing of csrc/gemm_f16x2.hip (the Makefile's flags
plus -S --cuda-device-only, as tests/test_gemm_f16x2_resources.py builds it).  CPU only.

The loop is walked as a graph of basic blocks (a label starts a block, a branch ends one).  Its *steady-state path* is the cheapest
way round it -- from the loop header back to the loop header, counted in instructions that are not MFMAs -- on which the K-tile
feeds the pipeline (its NJ weight DMA pieces and its two activation loads are issued): a source switch or a descriptor fetch only
ever adds instructions, so this is the path a K-tile takes when neither happens.  Instructions
are classed by tools/isa_count.py.

Checked per instantiation:
  * the steady-state path holds 12 NJ MFMAs per pair of phase barriers (one K-tile: hi a1 w1, lo a1 w2, lo a2 w1 on 4 x NJ blocks);
  * on no path through the loop is a scalar load, or the load of a source's row index (the loop's only 8-byte global load), followed
    by a wait on its counter before the load phase it was issued in ends: a load phase that switches sources waits for nothing it
    started itself (the descriptor of the next source is fetched from the compute phase, the row index a K-tile ahead);
  * the steady-state path is shorter than the parent commit's.
"""
import heapq
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# Non-MFMA instructions per K-tile on the steady-state path at commit 6c81de3 ("Penetration depth against the object mesh: fused
# dvq_grasp_mesh kernel"), the parent of the commit that restructured the loop: steady_path() below on that commit's listing.
PARENT_COMMIT = "6c81de3"
PARENT_NON_MFMA = {"bias NJ=2": 87, "bias NJ=4": 102, "resid NJ=2": 87, "resid NJ=4": 102, "gate NJ=4": 102, "gate-state NJ=4": 102,
                   "state NJ=2": 87, "state NJ=4": 102}

EPI = {"0": "bias", "1": "resid", "2": "gate", "5": "state"}
NAME = re.compile(r"^(_ZN\S*gemm_f16x2_pp_kernelILi(\d)ELi(\d)ELb([01])EEEv\S*):\s*; @\1\n", re.M)


def functions(text):
    """label ('gate-state NJ=4', ...) -> the function's instruction and label lines"""
    out = {}
    for m in NAME.finditer(text):
        epi, nj, init = m.group(2), m.group(3), m.group(4)
        label = f"{EPI[epi]}{'-state' if init == '1' else ''} NJ={nj}"
        body = text[m.end():text.index("s_endpgm", m.end())]
        lines = []
        for line in body.splitlines():
            code = line.split(";")[0].strip()
            if code and not code.startswith("."):
                lines.append(code)
            elif re.match(r"^\.LBB\d+_\d+:", line):
                lines.append(line.split(":")[0] + ":")
        out[label] = (lines, [ln.strip() for ln in body.splitlines()])
    return out


def loop_blocks(lines, raw):
    """The K loop (the function's loop with MFMAs in it) as {block id: (instructions, successors)} plus the header's id."""
    header = None
    for ln in raw:
        m = re.match(r"^(\.LBB\d+_\d+):.*Inner Loop Header", ln)
        if m:
            header = m.group(1)
    assert header, "no loop found"
    blocks, cur, name = {}, [], "entry"
    order = []
    for code in lines:
        if code.endswith(":") and code.startswith(".LBB"):
            blocks[name] = cur
            order.append(name)
            name, cur = code[:-1], []
        else:
            cur.append(code)
            if code.split()[0].startswith(("s_cbranch", "s_branch")):
                blocks[name] = cur
                order.append(name)
                name, cur = f"{name}+{len(order)}", []
    blocks[name] = cur
    order.append(name)
    succ = {}
    for i, b in enumerate(order):
        ins = blocks[b]
        nxt = order[i + 1] if i + 1 < len(order) else None
        last = ins[-1].split() if ins else [""]
        if last[0] == "s_branch":
            succ[b] = [last[1]]
        elif last[0].startswith("s_cbranch"):
            succ[b] = [last[1]] + ([nxt] if nxt else [])
        else:
            succ[b] = [nxt] if nxt else []
    return blocks, succ, header


def steady_path(lines, raw, nj):
    """(non-MFMA instructions, MFMAs, barriers) of the cheapest way from the loop header back to it on which the K-tile feeds the
    pipeline: its NJ weight DMA pieces and its two activation loads are issued"""
    import isa_count
    blocks, succ, header = loop_blocks(lines, raw)

    def cost(b):
        ops = [c.split()[0] for c in blocks[b]]
        k = [isa_count.classify(o) for o in ops]
        return (sum(1 for x in k if x != "MFMA"), sum(1 for x in k if x == "MFMA"), sum(1 for x in k if x == "BARRIER"),
                sum(1 for o in ops if o.startswith("global_load_lds")), sum(1 for o in ops if o == "global_load_dwordx4"))

    def add(a, d):
        return (a[0] + d[0], a[1] + d[1], a[2] + d[2], min(nj, a[3] + d[3]), min(2, a[4] + d[4]))

    heap = [(add((0, 0, 0, 0, 0), cost(header)), header)]
    seen = set()
    while heap:
        c, b = heapq.heappop(heap)
        if (b, c[3], c[4]) in seen:
            continue
        seen.add((b, c[3], c[4]))
        for s in succ[b]:
            if s == header:
                if c[3] == nj and c[4] == 2:
                    return c[:3]
                continue
            if s in blocks:
                heapq.heappush(heap, (add(c, cost(s)), s))
    raise AssertionError("the loop has no feeding path back to its header")


def header_in_load_phase(blocks, succ, header):
    """Where the compiler puts the loop header does not say which phase it is in: the load phase is the barrier-to-barrier region
    that reads fragments and issues the weight DMA.  True when such an instruction stands between the header and the first barrier
    in every direction the code can take from it."""
    seen, work, found = set(), [(header, False)], []
    while work:
        b, hit = work.pop()
        if (b, hit) in seen:
            continue
        seen.add((b, hit))
        done = False
        for code in blocks[b]:
            op = code.split()[0]
            if op.startswith(("ds_read", "global_load_lds")):
                hit = True
            if op == "s_barrier":
                found.append(hit)
                done = True
                break
        if not done:
            work += [(s, hit) for s in succ[b] if s in blocks and s != header]
    assert found and all(f == found[0] for f in found), "the loop header's phase is ambiguous"
    return found[0]


def waits_inside_a_load_phase(lines, raw):
    """Every (load, wait) pair of the loop where a scalar load or the row-index load is waited for inside the load phase that issued it."""
    blocks, succ, header = loop_blocks(lines, raw)
    bad, seen, memo = [], set(), {}
    work = [(header, header_in_load_phase(blocks, succ, header), None, None)]   # block, in a load phase, pending scalar / row-index load
    while work:
        state = work.pop()
        if state in seen:
            continue
        seen.add(state)
        b, load_phase, ps, pv = state
        for code in blocks[b]:
            op = code.split()[0]
            if op == "s_barrier":
                load_phase, ps, pv = not load_phase, None, None
            elif load_phase and op.startswith("s_load"):
                ps = code
            elif load_phase and op == "global_load_dwordx2":
                pv = code
            elif op == "s_waitcnt":
                if ps and "lgkmcnt" in code:
                    bad.append((ps, code))
                if pv and "vmcnt" in code:
                    bad.append((pv, code))
        for s in succ[b]:
            if s == header:
                continue                                    # one trip covers every phase: each ends at a barrier
            if s in blocks and reaches(succ, s, header, memo):
                work.append((s, load_phase, ps, pv))
    return bad


def reaches(succ, b, header, _memo):
    key = b
    if key not in _memo:
        seen, work, ok = set(), [b], False
        while work and not ok:
            x = work.pop()
            if x in seen:
                continue
            seen.add(x)
            for s in succ.get(x, []):
                if s == header:
                    ok = True
                work.append(s)
        _memo[key] = ok
    return _memo[key]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the listing checks need the compiler")
    out = str(tmp_path_factory.mktemp("kloop") / "gemm_f16x2.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-S", "--cuda-device-only",
                        "-o", out, "gemm_f16x2.hip"], cwd=os.path.join(ROOT, "d-vqvae_amd", "csrc"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    fns = functions(open(out).read())
    assert set(fns) == set(PARENT_NON_MFMA), sorted(fns)
    return fns


def test_steady_state_path_holds_the_tile_mfmas(listing):
    for label, (lines, raw) in listing.items():
        nj = int(label[-1])
        non_mfma, mfma, barriers = steady_path(lines, raw, nj)
        print(f"{label}: steady-state path {non_mfma} non-MFMA instructions, {mfma} MFMAs, {barriers} barriers")
        assert barriers >= 2 and barriers % 2 == 0, f"{label}: {barriers} barriers on the steady-state path"
        assert mfma == 12 * nj * (barriers // 2), f"{label}: {mfma} MFMAs for {barriers // 2} K-tile(s)"
        # every barrier-to-barrier stretch of the kernel that multiplies at all -- the loop's compute phase and the three peeled
        # K-tiles behind it -- holds one K-tile's MFMAs
        per_region, n = [], 0
        for code in lines:
            op = code.split()[0]
            if op == "s_barrier":
                per_region.append(n)
                n = 0
            elif op.startswith("v_mfma"):
                n += 1
        per_region.append(n)
        assert [r for r in per_region if r] == [12 * nj] * 4, f"{label}: MFMAs per barrier-to-barrier stretch {per_region}"


def test_no_load_phase_waits_for_a_descriptor_or_row_index_it_issued(listing):
    for label, (lines, raw) in listing.items():
        bad = waits_inside_a_load_phase(lines, raw)
        assert not bad, f"{label}: waited for inside the issuing load phase: {bad[:3]}"


def _toy_loop(load_phase_extra, header_after_barrier):
    """A two-phase loop in the listing's syntax; header_after_barrier: the loop header stands in front of the barrier that opens the
    load phase (this kernel's layout) or behind it (its parent's)."""
    load = ["ds_read_b128 v[0:3], v9", "s_waitcnt vmcnt(0)", "global_load_lds_dwordx4 v[4:5], off"] + load_phase_extra + ["s_waitcnt lgkmcnt(0)"]
    compute = ["v_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]"]
    if header_after_barrier:
        body = load + ["s_barrier"] + compute + ["s_barrier"]
    else:
        body = ["s_barrier"] + load + ["s_barrier"] + compute
    lines = [".LBB0_1:"] + body + ["s_cbranch_scc1 .LBB0_1"]
    return lines, [".LBB0_1:                                ; =>This Inner Loop Header: Depth=1"]


@pytest.mark.parametrize("header_after_barrier", [False, True])
def test_the_phase_walk_sees_a_wait_wherever_the_header_stands(header_after_barrier):
    """The walk flags a descriptor or row-index load issued in the load phase (the phase's closing lgkmcnt(0), or a vmcnt wait behind
    the row load, waits for it), and does not flag a clean load phase, whichever side of the barrier the loop header is on."""
    assert not waits_inside_a_load_phase(*_toy_loop([], header_after_barrier))
    assert waits_inside_a_load_phase(*_toy_loop(["s_load_dwordx2 s[4:5], s[0:1], 0x10"], header_after_barrier))
    assert waits_inside_a_load_phase(*_toy_loop(["global_load_dwordx2 v[6:7], v[6:7], off", "s_waitcnt vmcnt(0)"], header_after_barrier))
    assert not waits_inside_a_load_phase(*_toy_loop(["global_load_dwordx2 v[6:7], v[6:7], off"], header_after_barrier))


def test_steady_state_path_is_shorter_than_the_parents(listing):
    for label, (lines, raw) in listing.items():
        non_mfma, mfma, barriers = steady_path(lines, raw, int(label[-1]))
        per_tile = non_mfma / (barriers // 2)
        assert per_tile < PARENT_NON_MFMA[label], f"{label}: {per_tile} non-MFMA instructions per K-tile, {PARENT_NON_MFMA[label]} at {PARENT_COMMIT}"


if __name__ == "__main__":                                 # python tests/test_gemm_f16x2_kloop_listing.py listing.s: the figures of a listing
    for label, (lines, raw) in sorted(functions(open(sys.argv[1]).read()).items()):
        print(label, "(non-MFMA, MFMA, barriers) on the steady-state path:", steady_path(lines, raw, int(label[-1])), "| waits inside a load phase:",
              len(waits_inside_a_load_phase(lines, raw)))
