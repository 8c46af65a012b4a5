"""Test infrastructure: a numpy restatement of dvq_mesh_sample and dvq_cloud_fps, stated literally from include/dvq.h (every fp32
operation rounded on its own; the sequential uint64 ``cumsum`` IS the definition of the cdf).  Only tests import this file."""
import numpy as np

from oracle.philox import philox4x32_10

F = np.float32
TAG = 0xFFFFFFF0
SCALE = F(1048575.0)
MAX_FACES = 262144


def face_weights(verts, faces):
    """fp32 ``w`` [nf] of step 1 and the mask of faces with every index inside the object's vertices."""
    verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    idx = np.where(ok[:, None], faces, 0)
    if len(verts) == 0:
        return np.zeros(len(faces), F), ok
    a, b, c = verts[idx[:, 0]], verts[idx[:, 1]], verts[idx[:, 2]]
    e1, e2 = (b - a).astype(F), (c - a).astype(F)
    with np.errstate(all="ignore"):
        nx = (e1[:, 1] * e2[:, 2]).astype(F) - (e1[:, 2] * e2[:, 1]).astype(F)
        ny = (e1[:, 2] * e2[:, 0]).astype(F) - (e1[:, 0] * e2[:, 2]).astype(F)
        nz = (e1[:, 0] * e2[:, 1]).astype(F) - (e1[:, 1] * e2[:, 0]).astype(F)
        w = np.sqrt(((nx * nx).astype(F) + (ny * ny).astype(F)).astype(F) + (nz * nz).astype(F)).astype(F)
    w = np.where(np.isfinite(w) & ok, w, F(0.0)).astype(F)
    return w, ok


def face_cdf(verts, faces):
    """uint64 [nf]: the inclusive sums of the integer weights q of step 1, and whether a face index was out of range."""
    w, ok = face_weights(verts, faces)
    q = np.zeros(len(w), np.uint64)
    if len(w) and w.max() > 0:
        amax = F(w.max())
        live = w != 0
        share = (w[live] / amax).astype(F)
        q[live] = 1 + np.trunc((share * SCALE).astype(F)).astype(np.uint64)
    return np.cumsum(q, dtype=np.uint64), bool((~ok).any())


def _mulhi64(x, T):
    """The high 64 bits of x * T for uint64 arrays x and a uint64 T, by 32-bit halves."""
    m = np.uint64(0xFFFFFFFF)
    s = np.uint64(32)
    T = np.uint64(T)
    x0, x1, t0, t1 = x & m, x >> s, T & m, T >> s
    lo = x0 * t0
    mid1 = x1 * t0 + (lo >> s)
    mid2 = x0 * t1 + (mid1 & m)
    return x1 * t1 + (mid1 >> s) + (mid2 >> s)


def mesh_sample(meshes, S, seed, stream_ids):
    """``meshes``: a list of (verts [n,3], faces [m,3]) -> points fp32 [O,S,3], face int32 [O,S], status int32 [O], cdf uint64 [sum m]
    (zeros for an object of status 4) and the err bits.  A range cannot leave a list, so status 4 comes from a stream id only."""
    O = len(meshes)
    points, face = np.full((O, S, 3), np.nan, F), np.full((O, S), -1, np.int32)
    status, cdfs, err = np.zeros(O, np.int32), [], 0
    s_idx = np.arange(S, dtype=np.uint64)
    for o, (verts, faces) in enumerate(meshes):
        verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
        sid = int(stream_ids[o])
        if not 0 <= sid < 2 ** 32 or len(faces) > MAX_FACES:
            status[o], err = 4, err | (2 if len(faces) > MAX_FACES else 1)
            cdfs.append(np.zeros(len(faces), np.uint64))
            continue
        cdf, bad = face_cdf(verts, faces)
        err |= 2 if bad else 0
        cdfs.append(cdf)
        T = cdf[-1] if len(cdf) else np.uint64(0)
        if T == 0:
            status[o] = 1
            continue
        c = np.stack([np.full(S, TAG, np.uint64), s_idx, np.zeros(S, np.uint64), np.full(S, sid, np.uint64)], -1)
        X = philox4x32_10(c, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        t = _mulhi64((X[:, 0] << np.uint64(32)) | X[:, 1], T)
        f = np.searchsorted(cdf, t, side="right")                    # the smallest f with cdf[f] > t
        r1 = ((X[:, 2] >> np.uint64(8)).astype(F) + F(0.5)) * F(2.0 ** -24)
        r2 = ((X[:, 3] >> np.uint64(8)).astype(F) + F(0.5)) * F(2.0 ** -24)
        fold = (r1 + r2).astype(F) > F(1.0)
        r1, r2 = np.where(fold, F(1.0) - r1, r1).astype(F), np.where(fold, F(1.0) - r2, r2).astype(F)
        a = verts[faces[f, 0]]
        e1, e2 = (verts[faces[f, 1]] - a).astype(F), (verts[faces[f, 2]] - a).astype(F)
        points[o] = ((a + (r1[:, None] * e1).astype(F)).astype(F) + (r2[:, None] * e2).astype(F)).astype(F)
        face[o] = f.astype(np.int32)
    return points, face, status, (np.concatenate(cdfs) if cdfs else np.zeros(0, np.uint64)), err


def dist2(p, c):
    """fp32 d = ((dx*dx) + (dy*dy)) + (dz*dz) of rows p [n,3] against one point c [3]."""
    with np.errstate(all="ignore"):
        d = (np.asarray(p, F) - np.asarray(c, F)).astype(F)
        q = (d * d).astype(F)
        return ((q[:, 0] + q[:, 1]).astype(F) + q[:, 2]).astype(F)


def cloud_fps(points, keep):
    """points [P,3] of one object -> sel int32 [keep], gap fp32 [keep], status."""
    p = np.asarray(points, F).reshape(-1, 3)
    if not np.isfinite(p).all():
        return np.full(keep, -1, np.int32), np.full(keep, -1.0, F), 1
    sel, gap = np.zeros(keep, np.int32), np.full(keep, -1.0, F)
    picked = np.zeros(len(p), bool)
    picked[0] = True
    mind = dist2(p, p[0])
    for r in range(1, keep):
        key = np.where(picked, F(-1.0), mind)
        i = int(np.argmax(key))                                      # the first (lowest) position among equals
        sel[r], gap[r] = i, key[i]
        picked[i] = True
        d = dist2(p, p[i])
        mind = np.where(d < mind, d, mind)
    return sel, gap, 0
