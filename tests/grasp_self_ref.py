"""Numpy restatement of the self-collision figures (include/dvq.h: dvq_grasp_self) -- test infrastructure.  The nearest target of
every source is oracle/contact_oracle.nn_points, per source part, on the ASCENDING subset of the vertices that part is tested
against (an ascending subset keeps the tie order: the first minimum of the subset is the lowest index of the hand that attains it),
mapped back; the normals are oracle/contact_oracle.vertex_normals, as tests/grasp_score_ref.py takes them; the depth is the
oracle's fp32 fma.  This file adds the thresholds, the per-part figures, the mask words and the no-figure rows, and plain-Python
versions of the host statistics that share no code with contact.SelfTable / self_stats / self_class.

    d[v], idx[v] = nearest target u (label[u] in pairs[label[v]])      depth[v] = (hand[idx] - hand[v]) . n[idx]
    pen[v] = source[v] and idx[v] >= 0 and d[v] < reach2 and depth[v] > margin
    per part a: pen_count, max depth over pen (+0), min d over sources (+inf), OR of 1 << label[idx] over pen
    a row with a non-finite coordinate: status 1, -1 / NaN / NaN / 0 / 0
"""
import math

import numpy as np

from oracle import contact_oracle

f32 = np.float32


def grasp_self(hand, faces, labels, source, n_parts, pairs, reach2, margin):
    """hand [B,V,3], faces [F,3], labels [V], source [V], pairs [P] -> dict of pen_count [B,P] i32, pen_depth [B,P] f32, gap_min [B,P]
    f32, pair_bits [B,P] i32, mask [B,W] i32, status [B] i32, and per vertex vert_dist [B,V] f32, vert_idx [B,V] i32, vert_depth
    [B,V] f32 (NaN where idx < 0) for the tests' own use."""
    hand = np.ascontiguousarray(hand, f32)
    labels, source = np.asarray(labels, np.int64), np.asarray(source, np.int64)
    pairs = [int(w) & 0xffffffff for w in np.asarray(pairs).tolist()]
    B, V = hand.shape[:2]
    P, W = int(n_parts), (V + 31) // 32
    reach2, margin = f32(reach2), f32(margin)
    valid = (labels >= 0) & (labels < P)
    out = {"pen_count": np.zeros((B, P), np.int32), "pen_depth": np.zeros((B, P), f32), "gap_min": np.full((B, P), np.inf, f32),
           "pair_bits": np.zeros((B, P), np.int32), "mask": np.zeros((B, W), np.int32), "status": np.zeros(B, np.int32),
           "vert_dist": np.full((B, V), np.inf, f32), "vert_idx": np.full((B, V), -1, np.int32), "vert_depth": np.full((B, V), np.nan, f32)}
    for b in range(B):
        if not np.isfinite(hand[b]).all():
            out["status"][b] = 1
            out["pen_count"][b] = -1
            out["pen_depth"][b], out["gap_min"][b] = np.nan, np.nan
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            normals = contact_oracle.vertex_normals(hand[b:b + 1], faces)[0]
            d, idx = out["vert_dist"][b], out["vert_idx"][b]
            for a in range(P):
                mine = np.flatnonzero(valid & (labels == a))
                allowed = [q for q in range(P) if (pairs[a] >> q) & 1]
                trg = np.flatnonzero(valid & np.isin(labels, allowed))          # ascending
                if not len(mine) or not len(trg):
                    continue
                dd, ii = contact_oracle.nn_points(hand[b:b + 1, mine], hand[b:b + 1, trg])
                d[mine], idx[mine] = dd[0], trg[ii[0]]
            have = idx >= 0
            w = hand[b, idx[have]] - hand[b, have]
            n = normals[idx[have]]
            out["vert_depth"][b, have] = contact_oracle._fma(w[:, 2], n[:, 2], contact_oracle._fma(w[:, 1], n[:, 1], (w[:, 0] * n[:, 0]).astype(f32)))
        words, bits, depth = [0] * W, [0] * P, out["vert_depth"][b]
        for v in range(V):
            if not valid[v]:
                continue
            a = int(labels[v])
            if source[v] != 0 and d[v] < out["gap_min"][b, a]:
                out["gap_min"][b, a] = d[v]
            if source[v] != 0 and idx[v] >= 0 and d[v] < reach2 and depth[v] > margin:
                words[v >> 5] |= 1 << (v & 31)
                out["pen_count"][b, a] += 1
                if depth[v] > out["pen_depth"][b, a]:
                    out["pen_depth"][b, a] = depth[v]
                bits[a] |= 1 << int(labels[idx[v]])
        out["mask"][b] = np.asarray(words, np.uint32).view(np.int32)
        out["pair_bits"][b] = np.asarray(bits, np.uint32).view(np.int32)
    return out


def seam_sources(labels, faces, seam):
    """1 where the vertex may count as a source: breadth-first over the edges, `seam` rings from the edges that join two labels."""
    labels = [int(x) for x in labels]
    nbr = [set() for _ in labels]
    for a, b, c in np.asarray(faces).tolist():
        for i, j in ((a, b), (b, c), (c, a)):
            nbr[i].add(j)
            nbr[j].add(i)
    ring = {v for v in range(len(labels)) if any(labels[u] != labels[v] for u in nbr[v])} if seam >= 1 else set()
    for _ in range(seam - 1):
        ring = ring | {u for v in ring for u in nbr[v]}
    return [0 if v in ring else 1 for v in range(len(labels))]


def default_pairs(n_parts, palm, n_fingers=5):
    words = []
    for a in range(n_parts):
        w = 0
        for b in range(n_parts):
            if a < n_fingers and b != a and (b < n_fingers or palm):
                w |= 1 << b
        words.append(w)
    return words


def self_stats(out):
    """Per row (total, counts, depth in cm, pairs, clearance in cm or None) or None, in plain Python."""
    rows = []
    for c, d, g, w, s in zip(np.asarray(out["pen_count"]).tolist(), np.asarray(out["pen_depth"], np.float64).tolist(),
                             np.asarray(out["gap_min"], np.float64).tolist(), np.asarray(out["pair_bits"]).tolist(),
                             np.asarray(out["status"]).tolist()):
        if s != 0:
            rows.append(None)
            continue
        pairs = sorted([a, b] for a in range(len(c)) for b in range(len(c)) if ((w[a] & 0xffffffff) >> b) & 1)
        rows.append((sum(c), [int(k) for k in c], max(d) * 100.0, pairs, None if math.isinf(min(g)) else math.sqrt(min(g)) * 100.0))
    return rows


def self_class(pen_count, status, max_verts):
    return [2 if s != 0 else int(sum(c) > max_verts) for c, s in zip(np.asarray(pen_count).tolist(), np.asarray(status).tolist())]
