"""Numpy restatement of the per-grasp scores (include/dvq.h: dvq_grasp_scores) and of the per-object selection order
(dvq_segment_topk) -- test infrastructure.  The per-point quantities are oracle/contact_oracle.py's (nn_points, vertex_normals,
interior: imported, the arithmetic lives there); this file adds the canonical reduction and the total order.

    term[p]  = d[p] where the point is interior or d[p] is NaN, else +0.0
    part[t]  = +0.0 + term[t] + term[t + 256] + ...            (fp32, ascending p)            t = 0 .. 255
    for s in 128, 64, ..., 1:  part[t] += part[t + s]  for every t < s
    penetration = part[0];  n_interior = #interior;  n_contact = #(d < contact_threshold)

    a before b  <=>  (cls, key, index) smaller, a NaN key after every number of its class, -0.0 == +0.0
"""
import math

import numpy as np

from oracle import contact_oracle

f32 = np.float32
THREADS = 256


def sphere_mesh(n_lat=18, n_lon=43, radius=0.05):
    """Closed lat-long sphere, outward winding, V = n_lat * n_lon + 2 (776 for the defaults): the mesh of tests/test_contact.py."""
    th = np.linspace(0, np.pi, n_lat + 2)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    v = [[0, 0, radius]]
    for t in th:
        for p in ph:
            v.append([radius * np.sin(t) * np.cos(p), radius * np.sin(t) * np.sin(p), radius * np.cos(t)])
    v.append([0, 0, -radius])
    v = np.asarray(v, f32)
    ring = lambda i, j: 1 + i * n_lon + (j % n_lon)
    f = []
    for j in range(n_lon):
        f.append([0, ring(0, j), ring(0, j + 1)])
        f.append([len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(n_lat - 1):
        for j in range(n_lon):
            f.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            f.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return v, np.asarray(f, np.int64)


def tree_sum(terms):
    """The canonical fp32 sum of one grasp's terms [N]."""
    terms = np.asarray(terms, f32)
    part = np.zeros(THREADS, f32)                                 # +0.0
    for lo in range(0, terms.shape[0], THREADS):                  # thread t adds its points in ascending p
        chunk = terms[lo:lo + THREADS]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    s = THREADS // 2
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def point_terms(hand, faces, obj):
    """(d [B,N] f32, interior [B,N] bool, term [B,N] f32) of hand [B,V,3] against obj [B,N,3]."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    normals = contact_oracle.vertex_normals(hand, faces)
    with np.errstate(invalid="ignore"):
        d, idx = contact_oracle.nn_points(obj, hand)
        inside = contact_oracle.interior(normals, hand, obj, idx)
    term = np.where(inside | np.isnan(d), d, f32(0.0)).astype(f32)
    return d, inside, term


def grasp_scores(hand, faces, obj, contact_threshold=0.02 ** 2):
    """(penetration [B] f32, n_interior [B] int32, n_contact [B] int32)."""
    d, inside, term = point_terms(hand, faces, obj)
    with np.errstate(invalid="ignore"):
        pen = np.asarray([tree_sum(row) for row in term], f32)
        n_contact = (d < f32(contact_threshold)).sum(1).astype(np.int32)
    return pen, inside.sum(1).astype(np.int32), n_contact


def order_key(cls, key, index):
    k = float(key)
    return (int(cls), 1, 0.0, index) if math.isnan(k) else (int(cls), 0, k, index)        # -0.0 == 0.0 as Python floats


def segment_topk(cls, key, n_objects, n_candidates, keep):
    """int64 [O,keep]: each object's best candidates, best first (Python's stable sort over the total order)."""
    cls = np.asarray(cls).reshape(n_objects, n_candidates)
    key = np.asarray(key, f32).reshape(n_objects, n_candidates)
    out = np.empty((n_objects, keep), np.int64)
    for o in range(n_objects):
        ranked = sorted(range(n_candidates), key=lambda i: order_key(cls[o, i], key[o, i], i))
        out[o] = ranked[:keep]
    return out
