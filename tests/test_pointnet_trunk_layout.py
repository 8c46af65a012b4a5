"""The slot / id / group layout of the filtered PointNet trunk on v_mfma_f32_16x16x32_f16 (csrc/pn_slots.h, shared by
pn_trunk_filter_kernel and pn_exact_kernel) and its tile geometry and scratch layout (csrc/pn_filter.h, shared by the launchers and
the workspace plan): a host program checks the maps for whole clouds and the scratch arrays of a set, the wait-state rule of the
v_permlane16_swap_b32 relayout is unit-tested, and on the GPU the filtered features equal the exhaustive evaluation bit for bit at
sizes that put tile, row-block and lane-quarter boundaries on real points."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "d-vqvae_amd", "csrc")

HOST_PROGRAM = r"""
#include "pn_filter.h"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>
static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static void check_tile_maps() {
    // (wave, row block, quarter, register) <-> slot: a bijection onto 0 .. 255; the lane that feeds conv1 / conv2 with the point of
    // slot 64 w + 32 pb + r is row r & 15 of row block 2 pb + (r >> 4), and the accumulator (quarter, register) = row / 4, row % 4
    std::set<int> seen;
    for (int w = 0; w < 4; ++w) for (int rb = 0; rb < 4; ++rb) for (int q = 0; q < 4; ++q) for (int e = 0; e < 4; ++e) {
        const int s = pn_slot(w, rb, q, e);
        CHECK(s >= 0 && s < PN_TILE_SLOTS, "slot %d", s);
        seen.insert(s);
        const int pb = rb >> 1, r = 16 * (rb & 1) + 4 * q + e;
        CHECK(s == 64 * w + 32 * pb + r, "w %d rb %d q %d e %d: slot %d, conv2's lane works on slot %d", w, rb, q, e, s, 64 * w + 32 * pb + r);
        // the id the chain writes + the group tag the publishing wave adds, in front of any ring tag the mask removes
        const unsigned id = pn_group_tag(w, q) | pn_chain_id(rb, e);
        CHECK(id < 256, "id %u", id);
        CHECK(pn_chain_id(rb, e) < 16, "chain id %u does not fit under the ring tag (bits [6:5]) and the quarter (bits [5:4])", pn_chain_id(rb, e));
        CHECK(slot_of_id(id) == s, "slot_of_id(%u) = %d, want %d", id, slot_of_id(id), s);
        CHECK(pn_group_of_id(id) == 4 * w + q, "group of id %u: %d", id, pn_group_of_id(id));
    }
    CHECK((int)seen.size() == PN_TILE_SLOTS, "%d distinct slots", (int)seen.size());
    // a flagged group's sixteen slots: exactly the sixteen points ONE lane (wave, quarter; any column) scored; the groups partition the tile
    std::set<int> all;
    for (int g = 0; g < PN_GROUPS; ++g) {
        std::set<int> want, got;
        for (int rb = 0; rb < 4; ++rb) for (int e = 0; e < 4; ++e) want.insert(pn_slot(g >> 2, rb, g & 3, e));
        for (int k = 0; k < 16; ++k) { got.insert(pn_group_slot(g, k)); all.insert(pn_group_slot(g, k)); }
        CHECK(got == want && got.size() == 16, "group %d", g);
    }
    CHECK((int)all.size() == PN_TILE_SLOTS, "groups cover %d slots", (int)all.size());
}

static void check_cloud(int N, bool tail) {
    const PnGeometry g = pn_geometry(N, tail);              // the library's own geometry (launchers, workspace plan)
    const int tiles = g.tiles, deal = g.deal;
    std::vector<int> hits(N, 0);
    for (int t = 0; t < tiles; ++t) {
        std::set<int> pts;
        for (int s = 0; s < PN_TILE_SLOTS; ++s) {
            int p = point_of_slot(t, s, deal);
            CHECK(p >= 0, "N %d tile %d slot %d: point %d", N, t, s, p);
            if (t < deal) CHECK(p % deal == t && p < 256 * deal, "N %d tile %d slot %d: point %d is not this tile's", N, t, s, p);
            else CHECK(p == 256 * deal + (s & 31), "N %d tail tile slot %d: point %d", N, s, p);
            pts.insert(p);
            if (p >= N) p %= N;                             // a padding slot repeats a real point
            CHECK(p >= 0 && p < N, "N %d tile %d slot %d folds to %d", N, t, s, p);
            ++hits[p];
        }
        // a dealt tile: 256 different points; the tail tile: its 32, each in the slots of row blocks {0, 2} or {1, 3} of every wave
        CHECK((int)pts.size() == (t < deal ? PN_TILE_SLOTS : PN_TAIL_SLOTS), "N %d tile %d: %d distinct points", N, t, (int)pts.size());
        if (t >= deal) {
            for (int q = 0; q < 4; ++q) for (int e = 0; e < 4; ++e) for (int rb = 0; rb < 2; ++rb)
                CHECK(point_of_slot(t, pn_slot(0, rb, q, e), deal) == point_of_slot(t, pn_slot(0, rb + 2, q, e), deal), "tail: row block %d", rb);
            // the tail kernel's wave scores row blocks 0 and 1 (ids of "wave 0"): all 32 points, once
            std::set<int> scored;
            for (int rb = 0; rb < 2; ++rb) for (int q = 0; q < 4; ++q) for (int e = 0; e < 4; ++e)
                scored.insert(point_of_slot(t, slot_of_id(pn_group_tag(0, q) | pn_chain_id(rb, e)), deal));
            CHECK((int)scored.size() == PN_TAIL_SLOTS, "tail: %d points scored", (int)scored.size());
            // and a flagged group of it (quarter q) names the eight points of that quarter, each twice
            for (int q = 0; q < 4; ++q) {
                std::set<int> grp, want;
                for (int k = 0; k < 16; ++k) grp.insert(point_of_slot(t, pn_group_slot(q, k), deal));
                for (int rb = 0; rb < 2; ++rb) for (int e = 0; e < 4; ++e) want.insert(256 * deal + 16 * rb + 4 * q + e);
                CHECK(grp == want, "tail group %d", q);
            }
        }
    }
    for (int p = 0; p < N; ++p) CHECK(hits[p] >= 1, "N %d (tail %d): point %d is in no slot", N, (int)tail, p);
}

// the arrays of a scratch set (pn_set_layout): in order, 256-byte aligned, none reaching into the next; per sample they add up to what
// the workspace plan has always reserved -- 512 B of conv2 row and 96 B of tile records per padded point, 16 B of tile maxima per tile,
// 512 B of centre -- and the evaluated slots are the dealt tiles' 256 each + the tail tile's 32
static void check_scratch(int N, bool tail) {
    const PnGeometry g = pn_geometry(N, tail);
    CHECK(g.Npad == 256 * g.tiles && g.Npad >= N && g.Npad - N < 256, "N %d: Npad %d", N, g.Npad);
    CHECK(g.slots == 256L * g.deal + (g.deal < g.tiles ? 32 : 0), "N %d: slots %ld", N, g.slots);
    CHECK(g.per_sample() == (size_t)g.Npad * 128 * 4 + (size_t)g.Npad * 96 + (size_t)(g.Npad / 256) * 16 + 512, "N %d: %zu B per sample", N, g.per_sample());
    CHECK(g.part() >= (size_t)(g.Npad / 128) * 1024 * 4, "N %d: part does not hold the fused trunk's [tiles128][1024] floats", N);
    const size_t counts[] = {1, 5, 300};                    // (launch sizes below the plan's 4.5 GB per set at every N walked)
    for (size_t n : counts) {
        const PnSetLayout l = pn_set_layout(g, n);
        const size_t off[6] = {l.h2, l.part, l.part2, l.tstat, l.cbuf, l.bytes};
        const size_t len[5] = {n * g.h2, n * g.rec4, n * g.rec2, n * g.tstat, n * g.cbuf};
        CHECK(off[0] == 0, "N %d: the set starts at %zu", N, off[0]);
        for (int i = 0; i < 5; ++i) {
            CHECK(off[i] + len[i] <= off[i + 1], "N %d, %zu samples: array %d [%zu, +%zu) reaches into the next at %zu", N, n, i, off[i], len[i], off[i + 1]);
            CHECK(off[i] % (i == 2 ? 16 : 256) == 0, "N %d, %zu samples: array %d at %zu", N, n, i, off[i]);
        }
        CHECK(l.part2 == l.part + n * g.rec4, "N %d: the float2 records do not follow the float4 records", N);
        CHECK(l.bytes - n * g.per_sample() < 4 * 256, "N %d, %zu samples: %zu B for %zu B of arrays", N, n, l.bytes, n * g.per_sample());
        if (tail) printf("SET %d %zu %zu\n", N, n, l.bytes);
    }
}

int main() {
    check_tile_maps();
    const int sizes[] = {1024, 778, 3000, 16, 17, 33, 255, 256, 257, 288, 289};
    for (int N : sizes) { check_cloud(N, true); check_cloud(N, false); check_scratch(N, true); check_scratch(N, false); }
    if (fails) printf("%d check(s) failed\n", fails);
    else printf("OK\n");
    return fails ? 1 : 0;
}
"""


def _host_compiler():
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if gxx:
        return [gxx, "-std=c++17", "-O1"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        return [hipcc, "-x", "c++", "-std=c++17", "-O1"]                      # no offload target: a plain host compile
    return None


def _run_host_program(tmp_path):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++ / hipcc) found")
    src = tmp_path / "pn_slots_check.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "pn_slots_check"
    r = subprocess.run(cc + ["-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-1000:]
    return r.stdout


def test_slot_id_and_group_maps_on_the_host(tmp_path):
    """csrc/pn_slots.h compiled for the host: slot <-> (wave, row block, lane quarter, register) <-> point is a bijection onto a
    tile's points (padding slots fold onto real points), slot_of_id inverts the id the chain and the publishing wave write, and a
    flagged group's sixteen slots are the sixteen points one lane scored -- for every tile of N = 1024, 778 (tail tile) and 3000,
    with and without the tail tile, and for small clouds.  The geometry is the library's own (csrc/pn_filter.h: pn_geometry)."""
    _run_host_program(tmp_path)


def test_scratch_set_layout_is_what_the_workspace_plan_reserves(tmp_path):
    """csrc/pn_filter.h compiled for the host, for the same sizes and both tail settings: the arrays of a scratch set (conv2 rows,
    float4 and float2 tile records, tile maxima, centres) lie in order without overlap and add up, per sample, to the bytes the plan
    reserves; and the library's dvq_pointnet_workspace_bytes grows by exactly pn_set_layout(...).bytes per additional scratch set
    (DVQ_PN_SLOTS 2 -> 3 at a fixed launch size).  No GPU."""
    from dvqvae_amd import _lib
    lib = _lib.load()
    sets = [tuple(int(v) for v in ln.split()[1:]) for ln in _run_host_program(tmp_path).splitlines() if ln.startswith("SET ")]
    assert len(sets) == 11 * 3

    def workspace(env, B, N):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        lib.dvq_reload_env()
        try:
            return lib.dvq_pointnet_workspace_bytes(B, N)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
            lib.dvq_reload_env()
    for N, samples, set_bytes in sets:
        env = {"DVQ_PN_CHUNK": str(samples)}
        two = workspace(dict(env, DVQ_PN_SLOTS="2"), 4 * samples, N)
        three = workspace(dict(env, DVQ_PN_SLOTS="3"), 4 * samples, N)
        assert three - two == set_bytes, (N, samples, two, three, set_bytes)


def test_hazard_checker_permlane_swap_rule():
    """tools/check_hazards.py, rule R10: a VALU write of a register needs two wait states before v_permlane16_swap_b32 (or
    v_permlane32_swap_b32) reads it -- BOTH operands of the exchange count, and a swap's own results too.  The listing of
    pointnet_filter.hip, whose relayout feeds the swaps from inline-asm conversions the compiler's own hazard recognizer does not
    look into, must contain the swaps and pass; the same listing with a swap moved directly behind the producer of its operand
    must be flagged."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_hazards as ch
    for swap in ("v_permlane16_swap_b32_e32", "v_permlane32_swap_b32_e32"):
        for pair in (["v_add_f32_e32 v1, v2, v3", f"{swap} v4, v1"], ["v_add_f32_e32 v4, v2, v3", f"{swap} v4, v1"],
                     [f"{swap} v7, v1", f"{swap} v1, v9"]):
            assert [b[1] for b in ch.check_lines(pair)] == ["R10"], pair
            assert [b[1] for b in ch.check_lines([pair[0], "s_nop 0", pair[1]])] == ["R10"], pair
            assert ch.check_lines([pair[0], "s_nop 1", pair[1]]) == [], pair
            assert ch.check_lines([pair[0], "v_mov_b32_e32 v20, v21", "v_mov_b32_e32 v22, v23", pair[1]]) == [], pair
        assert ch.check_lines(["v_add_f32_e32 v5, v2, v3", f"{swap} v4, v1"]) == []          # an unrelated register
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the listing check needs the compiler")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-S",
                        "--cuda-device-only", "-o", "-", "pointnet_filter.hip"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    swaps = mutated = 0
    for name, body in ch.functions(r.stdout):
        if "pn_trunk_filter_kernel" not in name:
            continue
        lines = body.splitlines()
        assert [b for b in ch.check_lines(lines, strict=True, name=name[:60]) if b[1] == "R10"] == [], name
        idx = [i for i, ln in enumerate(lines) if ln.strip().startswith("v_permlane16_swap")]
        swaps += len(idx)
        if idx:
            # the first swap directly behind a VALU write of its first operand: the wait states "removed"
            op = lines[idx[0]].split()[1].rstrip(",")
            mutant = lines[:idx[0]] + [f"\tv_mov_b32_e32 {op}, {op}"] + lines[idx[0]:]
            assert "R10" in [b[1] for b in ch.check_lines(mutant, strict=True, name=name[:60])], name
            mutated += 1
    assert swaps >= 2 * 32 + 2 * 16 and mutated == 4, (swaps, mutated)     # 16 per point block: two full-tile and two tail kernels


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("N", [16, 17, 33, 255, 256, 257, 778, 1024, 3000])
def test_filtered_features_equal_exhaustive_at_layout_boundaries(C, N):
    """Filtered features == DVQ_PN_EXHAUSTIVE=1 features bit for bit, and no run-time consistency fault counted, at sizes that put
    the tile (256), row-block (16) and lane-quarter (4) boundaries of the 16x16x32 layout, and the tail tile (257, 778), on real
    points."""
    import torch
    from conftest import SEED
    from util import load_synth
    from dvqvae_amd import _lib, ops, synth
    from dvqvae_amd.network.pointnet_encoder import PointNetEncoder

    def with_env(env, fn):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        _lib.load().dvq_reload_env()
        try:
            return fn()
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
            _lib.load().dvq_reload_env()

    net = PointNetEncoder(channel=C)
    load_synth(net, SEED + 7 * C)
    net = net.to("cuda:0")
    B = 5
    x = synth.synthetic_clouds(B, N, seed=4100 + N, channels=C).to("cuda:0")
    ops.pointnet_fault_counters(reset=True)
    # DVQ_PN_FILTER=2: the filtered trunk also where the default prefers the six-product one (tiles less than 3/4 full)
    feat, trans, _ = with_env({"DVQ_PN_FILTER": "2"}, lambda: net(x))
    torch.cuda.synchronize()
    faults = ops.pointnet_fault_counters(reset=True)
    feat_all, trans_all, _ = with_env({"DVQ_PN_FILTER": "2", "DVQ_PN_EXHAUSTIVE": "1"}, lambda: net(x))
    assert torch.equal(trans, trans_all), "STN trunk: filtered != exhaustive"
    assert torch.equal(feat, feat_all), "main trunk: filtered != exhaustive"
    assert faults == (0, 0), f"dvq_pointnet_fault_counters after the filtered pass: {faults}"
