"""Numpy restatement of the force-closure quality with friction (include/dvq.h: dvq_grasp_closure) -- test infrastructure.  The
per-point quantities are oracle/contact_oracle.py's (nn_points, vertex_normals: imported, the arithmetic lives there), the centre's
reduction is tests/grasp_score_ref.tree_sum, as in tests/grasp_wrench_ref.py; this file adds, operation by operation in fp32,

    r = (obj - centre) * inv_length;  n = normal of the nearest vertex           (per contact: d < contact_threshold)
    a = uf + cross(ut, r);  s = dot(n, a);  c = cross(n, a);  h = fma(mu, sqrt(dot(c, c)), s)       (per direction u = (uf, ut))
    support[k] = (max over contacts of h, a NaN never taken) + 0.0;  quality = min over k;  worst_dir = the lowest k that attains it

a float64 computation of the support function from contacts given (support64), which shares no code with it, and a pure-Python
restatement of the direction table (directions)."""
import math

import numpy as np

from oracle import contact_oracle

import grasp_score_ref as score_ref

f32 = np.float32
BASES = (2, 3, 5, 7, 11, 13)


def _fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    return contact_oracle._fma(a, b, c)


def _dot(a, b):
    """fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)) over lists of three broadcastable fp32 arrays."""
    return _fma(a[2], b[2], _fma(a[1], b[1], (a[0] * b[0]).astype(f32)))


def _cross(a, b):
    """Every product rounded, no fma."""
    mul = lambda x, y: (x * y).astype(f32)
    return [(mul(a[1], b[2]) - mul(a[2], b[1])).astype(f32), (mul(a[2], b[0]) - mul(a[0], b[2])).astype(f32),
            (mul(a[0], b[1]) - mul(a[1], b[0])).astype(f32)]


def support32(n, r, dirs, mu):
    """Contacts n [C,3], r [C,3] and directions dirs [D,6], all fp32 -> support [D] fp32 in the kernel's arithmetic; -inf without a
    contact."""
    n, r, dirs, mu = np.asarray(n, f32).reshape(-1, 3), np.asarray(r, f32).reshape(-1, 3), np.asarray(dirs, f32), f32(mu)
    if n.shape[0] == 0:
        return np.full(dirs.shape[0], -np.inf, f32)
    uf = [dirs[:, None, c] for c in range(3)]                                          # [D,1] against [1,C]
    ut = [dirs[:, None, 3 + c] for c in range(3)]
    rr, nn = [r[None, :, c] for c in range(3)], [n[None, :, c] for c in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        a = [(uf[c] + x).astype(f32) for c, x in enumerate(_cross(ut, rr))]
        s = _dot(nn, a)
        c = _cross(nn, a)
        h = _fma(mu, np.sqrt(_dot(c, c)).astype(f32), s)                               # [D,C]
        best = np.fmax.reduce(h, axis=1, initial=f32(-np.inf))                         # h > best replaces: a NaN never does
    return (best.astype(f32) + f32(0.0)).astype(f32)


def support64(n, r, dirs, mu):
    """float64, contacts given: h(u_k) = max over contacts of n . a + mu |n x a| with a = uf + ut x r -> [D]."""
    n, r, dirs = np.asarray(n, np.float64).reshape(-1, 3), np.asarray(r, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64)
    a = dirs[:, None, :3] + np.cross(dirs[:, None, 3:], r[None])                       # [D,C,3]
    s = np.einsum("ci,dci->dc", n, a)
    c = np.cross(np.broadcast_to(n[None], a.shape), a)
    return (s + float(mu) * np.sqrt(np.einsum("dci,dci->dc", c, c))).max(axis=1)


def quality(support):
    """(min, the lowest index that attains it) of a support row without a NaN."""
    support = np.asarray(support)
    k = int(np.argmin(support))
    return support[k], k


def contacts(hand, faces, obj, inv_length, contact_threshold=0.02 ** 2):
    """hand [B,V,3], obj [B,N,3] -> (centre [B,3] f32, contact [B,N] bool, n [B,N,3] f32, r [B,N,3] f32, finite [B] bool): per point
    the normal of its nearest vertex and its scaled arm, whether it is a contact, and whether all of a row's coordinates are finite."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    B, N = obj.shape[:2]
    inv_length, thr = f32(inv_length), f32(contact_threshold)
    normals = contact_oracle.vertex_normals(hand, faces)
    centre = np.empty((B, 3), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        d, idx = contact_oracle.nn_points(obj, hand)
        for b in range(B):
            for c in range(3):
                centre[b, c] = f32(score_ref.tree_sum(obj[b, :, c])) / f32(N)
        contact = d < thr
        n = np.stack([normals[b, idx[b]] for b in range(B)])
        r = ((obj - centre[:, None]).astype(f32) * inv_length).astype(f32)
    finite = np.isfinite(hand).all(axis=(1, 2)) & np.isfinite(obj).all(axis=(1, 2))
    return centre, contact, n, r, finite


def grasp_closure(hand, faces, obj, inv_length, mu, dirs, contact_threshold=0.02 ** 2):
    """-> dict of quality [B] f32, worst_dir, status, n_contact [B] int32, centre [B,3] f32, support [B,D] f32, and -- for the tests'
    own assertions -- contact [B,N] bool, n and r [B,N,3]."""
    dirs = np.asarray(dirs, f32)
    centre, contact, n, r, finite = contacts(hand, faces, obj, inv_length, contact_threshold)
    B, D = contact.shape[0], dirs.shape[0]
    q, k, st = np.empty(B, f32), np.empty(B, np.int32), np.empty(B, np.int32)
    sup = np.empty((B, D), f32)
    for b in range(B):
        n_ct = int(contact[b].sum())
        if not finite[b]:
            st[b], q[b], k[b], sup[b] = 2, np.nan, -1, np.nan
        elif n_ct == 0:
            st[b], q[b], k[b], sup[b] = 1, -np.inf, -1, -np.inf
        else:
            sup[b] = support32(n[b][contact[b]], r[b][contact[b]], dirs, mu)
            st[b] = 0
            q[b], k[b] = quality(sup[b])
    return {"quality": q, "worst_dir": k, "status": st, "n_contact": contact.sum(axis=1).astype(np.int32), "centre": centre, "support": sup,
            "contact": contact, "n": n, "r": r}


def cut(full, D):
    """The reference at the first D directions from the one at more: the table of D directions is the head of every longer table."""
    out = dict(full, support=full["support"][:, :D])
    q, k = full["quality"].copy(), full["worst_dir"].copy()
    for b in np.nonzero(full["status"] == 0)[0]:
        q[b], k[b] = quality(out["support"][b])
    return dict(out, quality=q, worst_dir=k)


def radical_inverse(i, base):
    f, r = 1.0, 0.0
    while i:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def directions(D):
    """[D,6] float32: +e_0, -e_0, ..., -e_5, then u, -u for the accepted Halton points, cut at D."""
    rows = []
    for axis in range(6):
        for sign in (1.0, -1.0):
            rows.append([sign if c == axis else 0.0 for c in range(6)])
    i = 1
    while len(rows) < D:
        x = [2.0 * radical_inverse(i, b) - 1.0 for b in BASES]
        q = 0.0
        for v in x:
            q += v * v
        if 0.01 <= q <= 1.0:
            length = math.sqrt(q)
            rows.append([v / length for v in x])
            rows.append([-(v / length) for v in x])
        i += 1
    return np.asarray(rows[:D], np.float64).astype(f32)


def unit_directions(n=1000, seed=0):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)
