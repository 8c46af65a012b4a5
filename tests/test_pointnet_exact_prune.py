"""CPU model of what pn_exact_kernel evaluates (d-vqvae_amd/csrc/pointnet_filter.hip): the trunk kernel's tile records
restated with numpy / torch -- the deal and the groups of pn_slots.h, fp16 images with per-wave and per-channel power-of-two scales,
fp32 accumulation, the id in the low mantissa bits, the top two per 16-point group, the five per tile, the flag rule u >= c1 - 2 E_t --
and the exact stage's decision under its two pruning rules:

  rule 1  a flagged group is expanded only if u_g + E_t >= L, u_g = the smaller of the group's published pair where both are among
          the five, else c5;
  rule 2  L = max(lb, x1 - slack), x1 the exact score of the anchor (the top kept point of the tile that sets lb).

For every channel the maximum of the fp64 exact scores over the evaluated set must equal the maximum over ALL points.  It does not
run the HIP kernels (tests/test_pointnet_exact_prune_gpu.py does: filtered == exhaustive, bit for bit)."""
import numpy as np
import pytest
import torch

C_ID, DELTA = 5.0e-5, 1.0e-6          # the constants of pointnet_filter.hip
SLACK = 4.0e-7                        # rule 2's slack and the consistency check's: SLACK * (|v| + |w.c|)
TILE, GROUPS = 256, 16                # pn_slots.h


def _point_of_slot(tile, slot, deal):
    return ((slot * 67) & 255) * deal + tile


def _slot_of_id(i):
    return 64 * ((i >> 6) & 3) + 16 * ((i >> 2) & 3) + 4 * ((i >> 4) & 3) + (i & 3)


def _group_of_id(i):
    return 4 * ((i >> 6) & 3) + ((i >> 4) & 3)


def _id_of_slot(slot):
    wave, rb, q, e = slot >> 6, (slot >> 4) & 3, (slot >> 2) & 3, slot & 3
    return (wave << 6) | (q << 4) | (rb << 2) | e


def _pow2_scale(amax):
    out = np.ones_like(amax, dtype=np.float32)
    ok = (amax > 2.0 ** -106) & (amax < 2.0 ** 108)
    e = np.floor(np.log2(amax[ok].astype(np.float64)))
    out[ok] = (2.0 ** (14 - e)).astype(np.float32)
    return out


def _records(h, w, c):
    """h [P,128] (P a multiple of 256), w [NC,128], c [128] -> the tile records and the fp64 exact scores (relative to w.c)."""
    P, NC = h.shape[0], w.shape[0]
    tiles = P // TILE
    slots = np.arange(TILE)
    assert all(_slot_of_id(_id_of_slot(s)) == s for s in range(TILE))
    ids = np.array([_id_of_slot(s) for s in range(TILE)], dtype=np.uint32)
    t_n = _pow2_scale(np.abs(w).max(1))
    w16 = torch.from_numpy(w * t_n[:, None]).to(torch.float16)
    rn = np.sqrt((((w * t_n[:, None]).astype(np.float64) - w16.double().numpy()) ** 2).sum(1)) / t_n * 1.00001
    wn = np.sqrt((w.astype(np.float64) ** 2).sum(1)) * 1.00001
    cn = np.sqrt((c.astype(np.float64) ** 2).sum())
    top5 = np.empty((tiles, 5, NC), np.float32)
    flags = np.empty((tiles, GROUPS, NC), bool)
    E = np.empty((tiles, NC))
    pts = np.empty((tiles, TILE), np.int64)
    for t in range(tiles):
        pts[t] = _point_of_slot(t, slots, tiles)
        d = (h[pts[t]] - c[None, :]).astype(np.float32)
        dn = np.sqrt((d.astype(np.float64) ** 2).sum(1))
        approx = np.empty((TILE, NC), np.float32)
        rd = np.empty(TILE)
        for wave in range(4):                           # one power-of-two scale per wave of 64 slots
            sl = slice(64 * wave, 64 * wave + 64)
            s = _pow2_scale(np.array([dn[sl].max() * 1.0001], dtype=np.float32))[0]
            d16 = torch.from_numpy(d[sl] * s).to(torch.float16)
            rd[sl] = np.sqrt((((d[sl] * s).astype(np.float64) - d16.double().numpy()) ** 2).sum(1)) / s
            acc = (d16.float() @ w16.float().t()).numpy()
            bits = (acc.view(np.uint32) & np.uint32(0xFFFFFF00)) | ids[sl, None]
            approx[sl] = bits.view(np.float32) * (np.float32(1.0) / (np.float32(s) * t_n[None, :]))   # powers of two: the id bits stay
        dmx, rdm, hm = dn.max() * 1.00001, rd.max() * 1.00001, (dn.max() + cn) * 1.0001 * 1.00001
        E[t] = rn * dmx + wn * rdm + C_ID * wn * dmx + 2 * DELTA * wn * hm
        pairs = np.empty((GROUPS, 2, NC), np.float32)
        for g in range(GROUPS):
            member = np.array([_group_of_id(int(i)) == g for i in ids])
            assert member.sum() == 16
            v = -np.sort(-approx[member], axis=0)
            pairs[g] = v[:2]
        top5[t] = -np.sort(-pairs.reshape(2 * GROUPS, NC), axis=0)[:5]
        c1, c5 = top5[t, 0], top5[t, 4]
        u = np.where(pairs[:, 0] < c5[None, :], pairs[:, 0], pairs[:, 1])
        flags[t] = u >= (c1.astype(np.float64) - 2 * E[t])[None, :]
    exact = (h.astype(np.float64) - c.astype(np.float64)[None, :]) @ w.astype(np.float64).T
    wc = w.astype(np.float64) @ c.astype(np.float64)
    return dict(top5=top5, flags=flags, E=E, pts=pts, exact=exact, wc=wc, tiles=tiles)


def _evaluate(rec, rule1=True, rule2=True, gate="pair"):
    """-> (evaluated [P,NC] bool, candidate dots per channel [NC], expanded groups [tiles,GROUPS,NC] bool)."""
    top5, flags, E, pts, exact, wc = rec["top5"], rec["flags"], rec["E"], rec["pts"], rec["exact"], rec["wc"]
    tiles, NC = rec["tiles"], exact.shape[1]
    ch = np.arange(NC)
    ids = top5.view(np.uint32) & np.uint32(255)                                    # [tiles, 5, NC]
    slot_of = np.array([_slot_of_id(i) for i in range(256)])
    group_of = np.array([_group_of_id(i) for i in range(256)])
    point = np.stack([pts[t][slot_of[ids[t]]] for t in range(tiles)])              # [tiles, 5, NC]
    lbs = top5[:, 0].astype(np.float64) - E
    t_star = lbs.argmax(0)                                                         # the first tile that attains lb
    lb = lbs.max(0)
    anchor = point[t_star, 0, ch]
    L = lb.copy()
    if rule2:
        x1 = exact[anchor, ch]
        v = x1 + wc
        L = np.maximum(lb, x1 - SLACK * (np.abs(v) + np.abs(wc)))
    evaluated = np.zeros(exact.shape, bool)
    evaluated[anchor, ch] = True
    ndots = np.ones(NC, np.int64)
    expanded = np.zeros(flags.shape, bool)
    for t in range(tiles):
        live = top5[t, 0] + E[t] >= L                                              # the tile is in contention
        for k in range(5):
            take = live & (top5[t, k] + E[t] >= L) & ~((t_star == t) & (k == 0))
            evaluated[point[t, k, take], ch[take]] = True
            ndots += take
        for g in range(GROUPS):
            mine = group_of[ids[t]] == g                                           # [5, NC]
            both = mine.sum(0) >= 2
            second = np.where(mine, top5[t], np.float32(np.inf)).min(0)            # the smaller of the group's kept scores
            if gate == "pair":
                u = np.where(both, second, top5[t, 4])
            else:                                                                  # the unsound shortcut: c5 alone
                u = top5[t, 4]
            keep = ~(u + E[t] < L) if rule1 else np.ones(NC, bool)
            ex = flags[t, g] & live & keep
            expanded[t, g] = ex
            members = pts[t][[s for s in range(TILE) if group_of[_id_of_slot(s)] == g]]
            for n in ch[ex]:
                evaluated[members, n] = True
    return evaluated, ndots, expanded


def _misses(rec, evaluated):
    exact = rec["exact"]
    found = np.where(evaluated, exact, -np.inf).max(0)
    return np.nonzero(found != exact.max(0))[0]


def _cloud(case, rng, P=1024, NC=512):
    h = np.maximum(rng.standard_normal((P, 128)), 0).astype(np.float32) * 3.0
    w = (rng.standard_normal((NC, 128)) * 0.1).astype(np.float32)
    if case == "random":
        # a random cloud through random conv1 / conv2 layers: rows on a three-dimensional sheet, as the trunk's are -- neighbours in
        # space are near ties in every channel (independent rows, the "iid" case, have hardly any)
        xyz = rng.uniform(-1, 1, (P, 3))
        h1 = np.maximum(xyz @ rng.standard_normal((3, 64)) + 0.3 * rng.standard_normal(64), 0)
        h = np.maximum(h1 @ (rng.standard_normal((64, 128)) / 8) + 0.3 * rng.standard_normal(128), 0).astype(np.float32)
    elif case == "relu_sparse":
        h *= (rng.random((P, 128)) < 0.2)
    elif case == "tiny_spread":
        h = (h[:1] + 1e-4 * rng.standard_normal((P, 128))).astype(np.float32)
    elif case == "clusters":
        # eight near-duplicates of a strong point, all in tile 1 (residue 1 modulo the four tiles); the strong point itself, a little
        # stronger, is in tile 0: for the channels it wins, tile 1 is in contention with six or more scores in range and is not the best
        strong = (h[0] * 2.5).astype(np.float32)
        h[0] = strong
        for i in range(8):
            h[1 + 4 * (7 * i + 3)] = strong * np.float32(0.9995) * (1 + 1e-5 * rng.standard_normal(128)).astype(np.float32)
    elif case == "third_above_c5":
        # three near-duplicates of a strong point in ONE group of tile 0 (slots 0, 1, 2: wave 0, quarter 0): the group's pair is
        # kept, its third is hidden and beats every other score of the tile, c5 included
        strong = (h[0] * 2.5).astype(np.float32)
        for s in (0, 1, 2):
            h[_point_of_slot(0, s, P // TILE)] = strong * (1 + 1e-5 * rng.standard_normal(128)).astype(np.float32)
    c = h[[0, P // 4, P // 2, 3 * P // 4]].mean(0).astype(np.float32)
    return h, w, c


@pytest.mark.parametrize("case", ["random", "iid", "relu_sparse", "tiny_spread", "clusters", "third_above_c5"])
def test_pruned_exact_stage_never_drops_the_true_maximum(case):
    rng = np.random.default_rng(11)
    for cloud in range(3):
        h, w, c = _cloud(case, rng)
        rec = _records(h, w, c)
        for rule1, rule2 in ((True, True), (True, False), (False, True), (False, False)):
            evaluated, _, _ = _evaluate(rec, rule1, rule2)
            bad = _misses(rec, evaluated)
            assert bad.size == 0, f"{case}, cloud {cloud}, rule1={rule1} rule2={rule2}: channels {bad[:8].tolist()} lose their maximum"


def test_rules_prune_but_not_everything():
    """Non-vacuity on random clouds: the rules remove flagged groups and candidate dots, and still expand a group somewhere."""
    rng = np.random.default_rng(12)
    dots = [0, 0]
    groups = [0, 0]
    for cloud in range(4):
        rec = _records(*_cloud("random", rng, NC=1024))
        for i, on in enumerate((False, True)):
            _, ndots, expanded = _evaluate(rec, on, on)
            dots[i] += int(ndots.sum())
            groups[i] += int(expanded.sum())
    print(f"candidate dots {dots[0]} -> {dots[1]}, flagged groups {groups[0]} -> {groups[1]} (4 clouds x 1024 channels)")
    assert dots[1] < dots[0] and groups[1] < groups[0]
    assert groups[1] >= 1


def test_clusters_put_a_second_tile_in_contention():
    rng = np.random.default_rng(13)
    rec = _records(*_cloud("clusters", rng))
    _, _, expanded = _evaluate(rec)
    best_tile = (rec["top5"][:, 0].astype(np.float64) - rec["E"]).argmax(0)
    assert (expanded[1].any(0) & (best_tile != 1)).any(), "the cluster's tile should have a group expanded where it is not the best tile"


def test_c5_alone_is_not_a_bound_on_a_groups_hidden_points():
    """The trap: a group whose first two are kept may hide a third ABOVE c5.  Gating on c5 alone drops a true maximum; rule 1 does not."""
    rng = np.random.default_rng(14)
    dropped = 0
    for cloud in range(3):
        rec = _records(*_cloud("third_above_c5", rng))
        assert _misses(rec, _evaluate(rec, gate="pair")[0]).size == 0
        dropped += _misses(rec, _evaluate(rec, gate="c5")[0]).size
    assert dropped > 0, "the c5-only gate should lose a maximum on this data"
