"""Numpy restatement of the contact-wrench sums (include/dvq.h: dvq_grasp_wrench) -- test infrastructure.  The per-point quantities
are oracle/contact_oracle.py's (nn_points, vertex_normals, interior: imported, the arithmetic lives there), the reduction is
tests/grasp_score_ref.tree_sum; this file adds the centre, the wrenches, the 27 columns and the key in the stated fp32 order, and
a float64 computation of the host statistics that shares no code with contact.wrench_stats.

    centre[c] = tree_sum(obj[:, c]) / float32(N)
    f = n[j];  r = (obj - centre) * inv_length;  tau = cross(r, f) with every product rounded;  w = (f, tau)
    column c of point p: w[c] (c < 6), then w[a] * w[b] for a <= b row-major; +0.0 where d >= contact_threshold or d is NaN
    sums[c] = tree_sum(column c)
    key = NaN if penetration is NaN, else +inf if n_contact == 0, else fma chain of S0 .. S5 squared / (nf * nf)
"""
import math

import numpy as np

from oracle import contact_oracle

import grasp_score_ref as score_ref

f32 = np.float32
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]           # the upper triangle, row-major: columns 6 .. 26


def _fma(a, b, c):
    return contact_oracle._fma(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))


def grasp_wrench(hand, faces, obj, inv_length, contact_threshold=0.02 ** 2):
    """hand [B,V,3], obj [B,N,3] -> dict of penetration [B] f32, n_interior, n_contact [B] int32, centre [B,3], sums [B,27], key [B]."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    B, N = obj.shape[:2]
    inv_length, thr = f32(inv_length), f32(contact_threshold)
    pen, n_in, n_ct = score_ref.grasp_scores(hand, faces, obj, contact_threshold)
    normals = contact_oracle.vertex_normals(hand, faces)
    centre, sums, key = np.empty((B, 3), f32), np.empty((B, 27), f32), np.empty(B, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        d, idx = contact_oracle.nn_points(obj, hand)
        for b in range(B):
            for c in range(3):
                centre[b, c] = f32(score_ref.tree_sum(obj[b, :, c])) / f32(N)
            contact = d[b] < thr
            f = normals[b, idx[b]]                                                     # [N,3]
            r = ((obj[b] - centre[b][None]).astype(f32) * inv_length).astype(f32)
            mul = lambda x, y: (x * y).astype(f32)
            tau = [mul(r[:, 1], f[:, 2]) - mul(r[:, 2], f[:, 1]), mul(r[:, 2], f[:, 0]) - mul(r[:, 0], f[:, 2]),
                   mul(r[:, 0], f[:, 1]) - mul(r[:, 1], f[:, 0])]
            w = [f[:, 0], f[:, 1], f[:, 2]] + [t.astype(f32) for t in tau]
            cols = w + [mul(w[a], w[e]) for a, e in PAIRS]
            for c, col in enumerate(cols):
                sums[b, c] = score_ref.tree_sum(np.where(contact, col, f32(0.0)).astype(f32))
            S = sums[b]
            q = (S[0:1] * S[0:1]).astype(f32)
            for c in range(1, 6):
                q = _fma(S[c:c + 1], S[c:c + 1], q)
            nf = f32(n_ct[b])
            key[b] = f32(np.nan) if np.isnan(pen[b]) else (f32(np.inf) if n_ct[b] == 0 else f32(q[0]) / f32(nf * nf))
    return {"penetration": pen, "n_interior": n_in, "n_contact": n_ct, "centre": centre, "sums": sums, "key": key}


def wrench_stats(sums, n_contact):
    """float64, one grasp at a time: (force_residual, torque_residual, lambda_min of G / n, trace of G / n), or None where n == 0."""
    out = []
    for S, n in zip(np.asarray(sums, np.float64), np.asarray(n_contact)):
        n = int(n)
        if n == 0:
            out.append(None)
            continue
        force = math.sqrt(math.fsum(float(x) * float(x) for x in S[0:3])) / n
        torque = math.sqrt(math.fsum(float(x) * float(x) for x in S[3:6])) / n
        G = [[0.0] * 6 for _ in range(6)]
        for c, (a, e) in enumerate(PAIRS):
            G[a][e] = G[e][a] = float(S[6 + c]) / n
        lam = np.linalg.eigh(np.asarray(G, np.float64))[0]                            # ascending
        out.append((force, torque, float(lam[0]), float(sum(G[a][a] for a in range(6)))))
    return out


def unit_directions(n=1000, seed=0):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)
