"""Numpy restatement of the object-side contact map (include/dvq.h: dvq_segment_contact) -- test infrastructure.  The per-row,
per-point quantities are tests/grasp_score_ref.py's ``point_terms`` (the oracle's bits: normals, nearest vertex with the lowest index
on ties, the tangent-plane test); this file states rules 1-5 of the header literally:

    1. a row is valid iff its 3 V hand coordinates and its 3 N cloud coordinates are all finite; an invalid row takes part in nothing
    3. touch[o,p] = #valid rows with d_p < thr, inside[o,p] = #valid rows with inside_p, dmin[o,p] = min d_p over them (+inf: none)
    4. near_sum[o,p]: chain g = +0.0f + sqrt(d_p) over ascending segment positions i = g (mod 4) of the valid rows with d_p < thr,
       S = (c0 + c1) + (c2 + c3), every operation in fp32
    5. a rows entry outside [0, B): bit 0 of err, the segment's integers -1, its floats NaN, nothing read through the index
"""
import numpy as np

import grasp_score_ref as score_ref

f32 = np.float32


def meshes(V):
    """(vertices [V,3] f32, faces [F,3]) of the test hands: one vertex with a degenerate face, a triangular bipyramid, and the closed
    spheres of tests/grasp_score_ref.py with 776 and 778 vertices (778 = 8 * 97 + 2: MANO's vertex count, two beyond a multiple of 4)."""
    if V == 1:
        return np.asarray([[0.0, 0.0, 0.05]], f32), np.asarray([[0, 0, 0]], np.int64)
    if V == 5:
        v = np.asarray([[0, 0, 0.05], [0.05, 0, 0], [-0.025, 0.043, 0], [-0.025, -0.043, 0], [0, 0, -0.05]], f32)
        f = np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 1], [4, 2, 1], [4, 3, 2], [4, 1, 3]], np.int64)
        return v, f
    if V == 776:
        return score_ref.sphere_mesh()
    if V == 778:
        return score_ref.sphere_mesh(8, 97)
    raise ValueError(V)


def row_terms(hand, faces, obj, rows):
    """{row: (d [N] f32, inside [N] bool)} of the valid rows among ``rows``, and {row: valid}: every row evaluated once."""
    valid, terms = {}, {}
    for r in sorted(set(int(r) for r in rows)):
        valid[r] = bool(np.isfinite(hand[r]).all() and np.isfinite(obj[r]).all())
        if valid[r]:
            d, inside, _ = score_ref.point_terms(hand[r:r + 1], faces, obj[r:r + 1])
            terms[r] = (d[0], inside[0])
    return terms, valid


def segment_contact(hand, faces, obj, O, K, rows=None, contact_threshold=0.02 ** 2):
    """dict of touch, inside int32 [O,N]; dmin, near_sum f32 [O,N]; n_valid int32 [O]; row_status int32 [O*K]; err int.
    hand [B,V,3], obj [B,N,3] arrays (any strides); rows: O*K integers, or None for the identity (B must be O*K)."""
    hand, obj = np.asarray(hand, f32), np.asarray(obj, f32)
    B, N = hand.shape[0], obj.shape[1]
    thr = f32(contact_threshold)
    if rows is None:
        assert B == O * K
        rows = np.arange(O * K)
    rows = np.asarray(rows, np.int64).reshape(O, K)
    ok = [bool(((seg >= 0) & (seg < B)).all()) for seg in rows]
    terms, valid = row_terms(hand, faces, obj, [r for seg, good in zip(rows, ok) if good for r in seg])
    touch, inside = np.zeros((O, N), np.int32), np.zeros((O, N), np.int32)
    dmin, near_sum = np.full((O, N), np.inf, f32), np.zeros((O, N), f32)
    n_valid, status, err = np.zeros(O, np.int32), np.zeros((O, K), np.int32), 0
    for o, seg in enumerate(rows):
        if not ok[o]:                                                   # rule 5
            err |= 1
            touch[o], inside[o], n_valid[o], status[o] = -1, -1, -1, -1
            dmin[o], near_sum[o] = np.nan, np.nan
            continue
        chains = np.zeros((4, N), f32)                                  # +0.0
        for i, r in enumerate(int(r) for r in seg):
            if not valid[r]:                                            # rule 1
                status[o, i] = 1
                continue
            n_valid[o] += 1
            d, ins = terms[r]
            near = d < thr
            touch[o] += near
            inside[o] += ins
            dmin[o] = np.where(d < dmin[o], d, dmin[o])
            g = i % 4
            chains[g] = np.where(near, (chains[g] + np.sqrt(d).astype(f32)).astype(f32), chains[g])
        near_sum[o] = ((chains[0] + chains[1]).astype(f32) + (chains[2] + chains[3]).astype(f32)).astype(f32)
    return {"touch": touch, "inside": inside, "dmin": dmin, "near_sum": near_sum, "n_valid": n_valid, "row_status": status.reshape(-1),
            "err": err}


def brute_force(hand, faces, obj, O, K, contact_threshold):
    """An independent float64 statement on finite inputs, identity rows: (touch [O,N], inside [O,N], dmin [O,N] f64, rel_gap: how close,
    relatively, the nearest distance of any (row, point) comes to the threshold, dot_margin: the smallest |dot| of the interior test,
    tie_gap: the smallest relative gap between a point's two nearest vertices)."""
    hand, obj = np.asarray(hand, np.float64), np.asarray(obj, np.float64)
    faces = np.asarray(faces, np.int64)
    B, N = obj.shape[:2]
    touch, inside, dmin = np.zeros((O, N), np.int64), np.zeros((O, N), np.int64), np.full((O, N), np.inf)
    rel_gap, dot_margin, tie_gap = np.inf, np.inf, np.inf
    for r in range(B):
        o = r // K
        v = hand[r]
        fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
        n = np.zeros_like(v)
        for c in range(3):
            np.add.at(n, faces[:, c], fn)
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)
        d2 = ((obj[r][:, None, :] - v[None, :, :]) ** 2).sum(-1)       # [N,V]
        j = d2.argmin(1)
        d = d2[np.arange(N), j]
        if v.shape[0] > 1:
            second = np.partition(d2, 1, axis=1)[:, 1]
            tie_gap = min(tie_gap, float(((second - d) / np.maximum(second, 1e-300)).min()))
        dot = ((v[j] - obj[r]) * n[j]).sum(-1)
        rel_gap = min(rel_gap, float(np.abs(d / contact_threshold - 1.0).min()))
        dot_margin = min(dot_margin, float(np.abs(dot).min()))
        touch[o] += d < contact_threshold
        inside[o] += dot > 0
        dmin[o] = np.minimum(dmin[o], d)
    return touch, inside, dmin, rel_gap, dot_margin, tie_gap


def object_contact_stats(touch, dmin, near_sum, n_valid):
    """Independent of contact.object_contact_stats: plain Python floats, object by object."""
    import math
    out = []
    for t, d, s, n in zip(np.asarray(touch).tolist(), np.asarray(dmin, np.float64).tolist(), np.asarray(near_sum, np.float64).tolist(),
                          np.asarray(n_valid).tolist()):
        total = sum(t)
        entropy = None
        if total > 0:
            entropy = -math.fsum((k / total) * math.log(k / total) for k in t if k > 0)
        out.append({"grasps": n, "coverage": sum(1 for k in t if k >= 1) / len(t), "entropy": entropy,
                    "min_dist": [100.0 * math.sqrt(x) for x in d] if n > 0 else [None] * len(t),
                    "contact_dist": [100.0 * x / k if k > 0 else None for x, k in zip(s, t)]})
    return out
