"""Two references for dvq_grasp_mesh (include/dvq.h) -- test infrastructure.

(a) ``grasp_mesh``: the header's definition in numpy fp32, operation for operation (every array is float32, so every operation
    rounds to fp32 on its own; the fused multiply-adds are emulated in float64 as tests/grasp_volume_ref.py does).  It follows the
    DEFINITION, not the kernel: no tiles, no passes, no keys.  GPU results are compared with it exactly.
(b) ``brute_force``: an independent float64 evaluation -- inside by the generalised winding number (the sum of the faces' solid
    angles, Van Oosterom-Strackee), which shares nothing with ray casting, and the distance by grasp_volume_ref's closest-point
    routine.
"""
import numpy as np

from grasp_volume_ref import _fma, _point_triangle_distance, f32, object_frame

MAX_FACES = 262144
NO_LOOPS = (np.zeros(1, np.int32), np.zeros(0, np.int32))


# ---------------------------------------------------------------------------------------------- (a) the definition in fp32
def inside(p, mv, faces):
    """Step 2: bool [V] for points p [V,3] (object frame, fp32) against the faces [m,3] (local indices) of vertices mv [n,3];
    and whether a face index was out of range."""
    p, mv = np.ascontiguousarray(p, f32), np.ascontiguousarray(mv, f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    par = np.zeros(len(p), bool)
    bad = False
    with np.errstate(all="ignore"):
        for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
            if not (0 <= a < len(mv) and 0 <= b < len(mv) and 0 <= c < len(mv)):
                bad = True
                continue
            pa, pb, pc = mv[a], mv[b], mv[c]
            A = f32(f32(pb[0] - pa[0]) * f32(pc[1] - pa[1])) - f32(f32(pb[1] - pa[1]) * f32(pc[0] - pa[0]))
            if not (A > 0 or A < 0):
                continue
            xmn, xmx = min(pa[0], pb[0], pc[0]), max(pa[0], pb[0], pc[0])
            ymn, ymx = min(pa[1], pb[1], pc[1]), max(pa[1], pb[1], pc[1])
            ok = (xmn <= x) & (x <= xmx) & (ymn <= y) & (y <= ymx)
            if not ok.any():
                continue
            w = []
            for s, q in ((b, c), (c, a), (a, b)):                        # the edges opposite a, b, c
                P, Q = (s, q) if s < q else (q, s)
                dx, dy = f32(mv[Q, 0] - mv[P, 0]), f32(mv[Q, 1] - mv[P, 1])
                e = ((dx * (y - mv[P, 1]).astype(f32)).astype(f32) - (dy * (x - mv[P, 0]).astype(f32)).astype(f32)).astype(f32)
                rev = s > q
                tie = bool(dy < 0 or (dy == 0 and dx > 0))
                ok &= ((e > 0) | ((e == 0) & tie)) == ((A > 0) != rev)
                ok &= ~np.isnan(e)
                w.append(-e if rev else e)
            if not ok.any():
                continue
            wa, wb, wc = (k[ok] for k in w)
            zc = (((wa * pa[2]).astype(f32) + (wb * pb[2]).astype(f32)).astype(f32) + (wc * pc[2]).astype(f32)).astype(f32) \
                / ((wa + wb).astype(f32) + wc).astype(f32)
            par[ok] ^= zc.astype(f32) > z[ok]
    return par, bad


def _dot(u, w):
    return _fma(u[..., 2], w[..., 2], _fma(u[..., 1], w[..., 1], (u[..., 0] * w[..., 0]).astype(f32)))


def tri_d2(p, a, b, c):
    """Step 3 for one face: fp32 [n] squared distances of the points p [n,3] to the triangle (a, b, c)."""
    p, a, b, c = (np.asarray(k, f32) for k in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, cb = (b - a).astype(f32), (c - a).astype(f32), (c - b).astype(f32)
        ap, bp, cp = (p - a).astype(f32), (p - b).astype(f32), (p - c).astype(f32)
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc = ((d1 * d4).astype(f32) - (d3 * d2).astype(f32)).astype(f32)
        vb = ((d5 * d2).astype(f32) - (d1 * d6).astype(f32)).astype(f32)
        va = ((d3 * d6).astype(f32) - (d5 * d4).astype(f32)).astype(f32)
        u, w = (d4 - d3).astype(f32), (d5 - d6).astype(f32)
        along = lambda s, d, o: np.stack([_fma(s, d[i], o[..., i]) for i in range(3)], axis=-1)
        full = lambda k: np.broadcast_to(k, p.shape).astype(f32)
        n = ((va + vb).astype(f32) + vc).astype(f32)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (u >= 0) & (w >= 0)]
        qs = [full(a), full(b), along((d1 / (d1 - d3).astype(f32)).astype(f32), ab, full(a)), full(c),
              along((d2 / (d2 - d6).astype(f32)).astype(f32), ac, full(a)), along((u / (u + w).astype(f32)).astype(f32), cb, full(b))]
        q = along((vc / n).astype(f32), ac, along((vb / n).astype(f32), ab, full(a)))
        for cond, cand in reversed(list(zip(conds, qs))):               # the first that applies wins
            q = np.where(cond[:, None], cand, q)
        e = (p - q).astype(f32)
        return _dot(e, e)


def nearest(p, mv, faces):
    """Step 3: (dist2 fp32 [n], face int32 [n]) of the points p [n,3] over the faces in ascending order."""
    best, face = np.full(len(p), np.inf, f32), np.full(len(p), -1, np.int32)
    if len(p) == 0:
        return best, face
    for i, (a, b, c) in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if not (0 <= a < len(mv) and 0 <= b < len(mv) and 0 <= c < len(mv)):
            continue
        d = tri_d2(p, mv[a], mv[b], mv[c])
        with np.errstate(invalid="ignore"):
            better = d < best
        best, face = np.where(better, d, best).astype(f32), np.where(better, i, face).astype(np.int32)
    return best, face


def grasp_mesh(hand, mesh_verts, vert_off, mesh_faces, face_off, obj_of_row, R=None, t=None):
    """The batch: dict of n_inside, deep_vertex, deep_face, status int32 [B], depth f32 [B], mask int32 [B,W], vert_d2 f32 [B,V],
    vert_face int32 [B,V] and ``err``, the bits of the error flag."""
    hand = np.ascontiguousarray(hand, f32)
    mesh_verts, mesh_faces = np.asarray(mesh_verts, f32).reshape(-1, 3), np.asarray(mesh_faces).reshape(-1, 3)
    B, V = hand.shape[:2]
    W, O = (V + 31) // 32, len(vert_off) - 1
    out = {"n_inside": np.zeros(B, np.int32), "depth": np.zeros(B, f32), "deep_vertex": np.full(B, -1, np.int32),
           "deep_face": np.full(B, -1, np.int32), "mask": np.zeros((B, W), np.int32), "status": np.zeros(B, np.int32),
           "vert_d2": np.full((B, V), np.inf, f32), "vert_face": np.full((B, V), -1, np.int32), "err": 0}
    for b in range(B):
        o = int(obj_of_row[b])
        ranges_ok = False
        if 0 <= o < O:
            v0, nv = int(vert_off[o]), int(vert_off[o + 1]) - int(vert_off[o])
            f0, nf = int(face_off[o]), int(face_off[o + 1]) - int(face_off[o])
            ranges_ok = (nv >= 0 and 0 <= nf <= MAX_FACES and 0 <= v0 <= len(mesh_verts) - nv and 0 <= f0 <= len(mesh_faces) - nf)
        if not ranges_ok or not np.isfinite(hand[b]).all():
            if not ranges_ok:
                out["err"] |= 2 if 0 <= o < O else 1
            out["n_inside"][b], out["depth"][b], out["status"][b] = -1, np.nan, (3 if ranges_ok else 4)
            out["vert_d2"][b] = np.nan
            continue
        if nf == 0:
            out["status"][b] = 1
            continue
        mv, mf = mesh_verts[v0:v0 + nv], mesh_faces[f0:f0 + nf]
        p = object_frame(hand[b], *NO_LOOPS, None if R is None else R[b], t)
        ins, bad = inside(p, mv, mf)
        if bad:
            out["err"] |= 2
        idx = np.nonzero(ins)[0]
        d2, face = nearest(p[idx], mv, mf)
        out["vert_d2"][b, idx], out["vert_face"][b, idx] = d2, face
        out["n_inside"][b] = len(idx)
        words = np.zeros(W, np.uint32)
        for v in idx:
            words[v >> 5] |= np.uint32(1) << np.uint32(v & 31)
        out["mask"][b] = words.view(np.int32)
        deep = -1
        for k, v in enumerate(idx):                                     # ascending: the first, then every larger one
            if deep < 0 or d2[k] > d2[deep]:
                deep = k
        if deep >= 0:
            out["depth"][b], out["deep_vertex"][b], out["deep_face"][b] = np.sqrt(f32(d2[deep])), idx[deep], face[deep]
    return out


# ---------------------------------------------------------------------------------------------- (b) the float64 brute force
def winding_number(points, verts, faces):
    """Generalised winding number of the closed mesh about every point, float64 [n]: the solid angles of the faces by Van Oosterom
    and Strackee, summed and divided by 4 pi."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    a, b, c = (v[f[:, k]][None] - p[:, None] for k in range(3))          # [n,m,3]
    la, lb, lc = (np.linalg.norm(k, axis=2) for k in (a, b, c))
    num = np.einsum("nmk,nmk->nm", a, np.cross(b, c))
    den = la * lb * lc + np.einsum("nmk,nmk->nm", a, b) * lc + np.einsum("nmk,nmk->nm", b, c) * la + np.einsum("nmk,nmk->nm", c, a) * lb
    return (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)


def surface_distance(points, verts, faces):
    """Distance of every point to the mesh's surface, float64 [n]."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    best = np.full(len(p), np.inf)
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        best = np.minimum(best, _point_triangle_distance(p, v[a], v[b], v[c]))
    return best


def brute_force(points, verts, faces):
    """(inside bool [n], distance float64 [n]) of points against a closed mesh, everything in float64."""
    return np.abs(winding_number(points, verts, faces)) > 0.5, surface_distance(points, verts, faces)
