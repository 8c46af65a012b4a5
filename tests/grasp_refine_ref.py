"""Numpy restatement of the translation push-out (include/dvq.h: dvq_grasp_refine) -- test infrastructure.  The per-point
quantities are oracle/contact_oracle.py's (vertex_normals, nn_points, interior) and every sum is grasp_score_ref.tree_sum; this
file adds the loop: the translation taken from the object points, the two mean pull vectors, the key and the best iterate.

    t = +0;  for k = 0 .. steps:
        o' = obj - t;  d, j, inside on o' (the normals once, of the hand as given);  g = o' - hand[j];  near = !inside & (d < thr)
        pen = tree_sum(inside | isnan(d) ? d : +0);  S_in = tree_sum(inside ? g : +0);  S_nr = tree_sum(near ? g : +0)   per component
        key = (2 if isnan(pen) else 1 if n_ct < min_contact else 0, pen);  best iff strictly smaller (iterate 0 starts)
        stop at k == steps, on a NaN pen or a zero step;  step = push * (S_in / n_in) [n_in > 0] + pull * (S_nr / n_nr) [n_nr > 0]
"""
import numpy as np

from oracle import contact_oracle

import grasp_score_ref as ref

f32 = np.float32


def sphere_cloud(n=1000, radius=0.04, centre=(0.07, 0.01, 0.0)):
    """n points on a sphere (the golden-angle spiral), fp32 [n,3]."""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    ph = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return (np.stack([r * np.cos(ph), r * np.sin(ph), z], 1) * radius + np.asarray(centre)).astype(f32)


def refine_one(hand, normals, obj, steps, push, pull, min_contact, thr):
    """One grasp: hand [V,3], normals [V,3], obj [N,3] -> (offset [3] f32, iter, pen f32, n_in, n_ct, trace): trace lists every
    iterate's (t, cls, pen, n_in, n_ct)."""
    push, pull, thr = f32(push), f32(pull), f32(thr)
    t = np.zeros(3, f32)
    best, trace = None, []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(steps + 1):
            o = (obj - t[None]).astype(f32)
            d, j = contact_oracle.nn_points(o[None], hand[None])
            inside = contact_oracle.interior(normals[None], hand[None], o[None], j)[0]
            d, j = d[0], j[0]
            g = (o - hand[j]).astype(f32)
            near = ~inside & (d < thr)
            pen = ref.tree_sum(np.where(inside | np.isnan(d), d, f32(0.0)).astype(f32))
            s_in = [ref.tree_sum(np.where(inside, g[:, c], f32(0.0)).astype(f32)) for c in range(3)]
            s_nr = [ref.tree_sum(np.where(near, g[:, c], f32(0.0)).astype(f32)) for c in range(3)]
            n_in, n_ct, n_nr = int(inside.sum()), int((d < thr).sum()), int(near.sum())
            cls = 2 if np.isnan(pen) else (1 if n_ct < min_contact else 0)
            trace.append((t.copy(), cls, pen, n_in, n_ct))
            if best is None or cls < best[1] or (cls == best[1] and pen < best[2]):
                best = (k, cls, pen, n_in, n_ct, t.copy())
            if k == steps or np.isnan(pen):
                break
            step = np.zeros(3, f32)
            for c in range(3):
                if n_in > 0:
                    step[c] = f32(step[c] + f32(push * f32(s_in[c] / f32(n_in))))
                if n_nr > 0:
                    step[c] = f32(step[c] + f32(pull * f32(s_nr[c] / f32(n_nr))))
            if (step == 0).all():
                break
            t = (t + step).astype(f32)
    k, cls, pen, n_in, n_ct, t = best
    return t, k, f32(pen), n_in, n_ct, trace


def grasp_refine(hand, faces, obj, steps, push=1.0, pull=0.25, min_contact=1, contact_threshold=0.02 ** 2, traces=None):
    """(offset [B,3] f32, iter [B] i32, penetration [B] f32, n_interior [B] i32, n_contact [B] i32) of hand [B,V,3] against
    obj [B,N,3]; ``traces``: a list that receives each grasp's trace."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        normals = contact_oracle.vertex_normals(hand, faces)
    B = hand.shape[0]
    off, it = np.zeros((B, 3), f32), np.zeros(B, np.int32)
    pen, n_in, n_ct = np.zeros(B, f32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        off[b], it[b], pen[b], n_in[b], n_ct[b], trace = refine_one(hand[b], normals[b], obj[b], int(steps), push, pull, int(min_contact),
                                                                    contact_threshold)
        if traces is not None:
            traces.append(trace)
    return off, it, pen, n_in, n_ct
