"""Numpy restatement of hand-side contact (include/dvq.h: dvq_grasp_parts) -- test infrastructure.  The per-vertex quantities are
oracle/contact_oracle.nn_points with the HAND as the source (imported: the arithmetic lives there); this file adds the threshold,
the per-part minima and counts, the mask words and the no-figure rows, and plain-Python versions of the host statistics that share
no code with contact.part_stats / contact_map / parts_class.

    d[v], idx[v] = nn_points(hand, obj)            touch[v] = d[v] < thr
    part_min[q] = min d[v] over label[v] == q (+inf if none)    part_count[q] = #(touch[v] and label[v] == q)
    mask word v >> 5, bit v & 31 = touch[v]
    a row with a non-finite coordinate: status 1, NaN / -1 / 0
"""
import math

import numpy as np

from oracle import contact_oracle

f32 = np.float32


def grasp_parts(hand, labels, n_parts, obj, contact_threshold):
    """hand [B,V,3], labels [V], obj [B,N,3], a squared threshold -> dict of part_min [B,P] f32, part_count [B,P] i32, mask [B,W]
    i32, status [B] i32, vert_dist [B,V] f32, vert_idx [B,V] i32."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    labels = np.asarray(labels, np.int64)
    B, V = hand.shape[:2]
    W, thr = (V + 31) // 32, f32(contact_threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        d, idx = contact_oracle.nn_points(hand, obj)
    out = {"part_min": np.full((B, n_parts), np.inf, f32), "part_count": np.zeros((B, n_parts), np.int32),
           "mask": np.zeros((B, W), np.int32), "status": np.zeros(B, np.int32), "vert_dist": d.astype(f32),
           "vert_idx": idx.astype(np.int32)}
    for b in range(B):
        if not (np.isfinite(hand[b]).all() and np.isfinite(obj[b]).all()):
            out["status"][b] = 1
            out["part_min"][b], out["vert_dist"][b] = np.nan, np.nan
            out["part_count"][b], out["vert_idx"][b] = -1, -1
            continue
        words = [0] * W
        for v in range(V):
            touch = bool(d[b, v] < thr)
            if touch:
                words[v >> 5] |= 1 << (v & 31)
            q = int(labels[v])
            if 0 <= q < n_parts:
                if d[b, v] < out["part_min"][b, q]:
                    out["part_min"][b, q] = d[b, v]
                out["part_count"][b, q] += touch
        out["mask"][b] = np.asarray(words, np.uint32).view(np.int32)
    return out


def part_stats(part_min, part_count, status, min_verts=1, n_fingers=5):
    """Per row (fingers, counts, distances in cm) or None, in plain Python floats."""
    rows = []
    for m, c, s in zip(np.asarray(part_min).tolist(), np.asarray(part_count).tolist(), np.asarray(status).tolist()):
        if s != 0:
            rows.append(None)
            continue
        rows.append((sum(1 for k in c[:n_fingers] if k >= min_verts), [int(k) for k in c],
                     [None if math.isinf(x) else math.sqrt(x) * 100.0 for x in m]))
    return rows


def contact_map(mask, n_verts):
    rows = np.asarray(mask).astype(np.int64) & 0xffffffff
    return [sum((int(r[v >> 5]) >> (v & 31)) & 1 for r in rows) for v in range(n_verts)]


def parts_class(part_count, status, min_fingers, need_thumb, min_verts=1, n_fingers=5):
    out = []
    for c, s in zip(np.asarray(part_count).tolist(), np.asarray(status).tolist()):
        on = [k >= min_verts for k in c[:n_fingers]]
        out.append(2 if s != 0 else int(sum(on) < min_fingers or (bool(need_thumb) and not on[0])))
    return out
