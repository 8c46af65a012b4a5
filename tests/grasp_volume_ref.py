"""Two references for dvq_grasp_volume (include/dvq.h) -- test infrastructure.

(a) ``grasp_volume``: the header's definition in numpy fp32, operation for operation (every array below is float32, so every
    operation rounds to fp32 on its own; the three fused multiply-adds of the definition are emulated in float64 as
    oracle/contact_oracle.py does).  It follows the DEFINITION, not the kernel: a dense parity array over the box, no tiles, no bit
    words.  GPU results are compared with it exactly.
(b) ``brute_force``: an independent float64 evaluation of what the definition approximates -- per-voxel plane tests, inside-the-hand
    by the parity of Moeller-Trumbore hits along an oblique ray -- with the list of UNCERTAIN voxels: centres within ``tol`` of the
    hand's surface or of a hull plane whose membership in the intersection can flip there, where fp32 and float64 may legitimately
    disagree.
"""
import numpy as np

f32 = np.float32
MAX_CELLS, IDX_LIMIT, MAX_PLANES = 1024, 4194302, 8192
RAY = np.asarray([0.3713906763541037, 0.2785430072655778, 0.8857] / np.linalg.norm([0.3713906763541037, 0.2785430072655778, 0.8857]))

# the half-spaces of the sphere tests (n, d): a box off the lattice values (i + 1/2) h of both spacings, cut by one oblique plane
SPHERE_PLANES = np.asarray([[1, 0, 0, 0.0237], [-1, 0, 0, 0.0311], [0, 1, 0, 0.0193], [0, -1, 0, 0.0271], [0, 0, 1, 0.0149],
                            [0, 0, -1, 0.0333], [0.6, 0.8, 0, 0.03]], f32)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def centres(i, h):
    """c(i) = ((float)i + 0.5f) * h"""
    return ((np.asarray(i).astype(f32) + f32(0.5)) * f32(h)).astype(f32)


def mesh_volume(verts, faces):
    """Signed-tetrahedra volume of a closed mesh, float64."""
    v = np.asarray(verts, np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def object_frame(hand, loop_off, loop_vert, R, t):
    """Steps 1 and 2: [V,3] fp32 -> [V+L,3] fp32 in the object's frame."""
    hand = np.ascontiguousarray(hand, f32)
    rows = [hand]
    for l in range(len(loop_off) - 1):
        s = np.zeros(3, f32)
        for q in range(int(loop_off[l]), int(loop_off[l + 1])):
            s = (s + hand[int(loop_vert[q])]).astype(f32)
        rows.append((s / f32(int(loop_off[l + 1]) - int(loop_off[l])))[None].astype(f32))
    v = np.concatenate(rows).astype(f32)
    if R is None:
        return v
    R = np.asarray(R, f32)
    u = (v - np.asarray(t, f32)[None]).astype(f32) if t is not None else v
    return np.stack([_fma(R[2, i], u[:, 2], _fma(R[1, i], u[:, 1], (R[0, i] * u[:, 0]).astype(f32))) for i in range(3)], axis=1)


def box_of(v, h):
    """Step 3: (lo [3], n [3]) or None when the box is refused (status 2)."""
    h = f32(h)
    with np.errstate(all="ignore"):
        fl, fh = np.floor(v.min(0) / h), np.floor(v.max(0) / h)
    if np.isnan(v).any() or not (np.abs(fl) <= IDX_LIMIT).all() or not (np.abs(fh) <= IDX_LIMIT).all():
        return None
    lo = fl.astype(np.int64) - 1
    n = fh.astype(np.int64) + 1 - lo + 1
    return (lo, n) if (n <= MAX_CELLS).all() else None


def hand_voxels(v, faces, lo, n, h):
    """Steps 4 - 8: bool [nx,ny,nk], True where the voxel is in the hand; and the number of covering triangles per column."""
    h = f32(h)
    cz = centres(lo[2] + np.arange(n[2]), h)
    parity = np.zeros(tuple(n), bool)
    covers = np.zeros((n[0], n[1]), np.int64)
    for a, b, c in np.asarray(faces).tolist():
        pa, pb, pc = v[a], v[b], v[c]
        A = f32(f32(pb[0] - pa[0]) * f32(pc[1] - pa[1])) - f32(f32(pb[1] - pa[1]) * f32(pc[0] - pa[0]))
        if not (A > 0 or A < 0):
            continue
        xmn, xmx = min(pa[0], pb[0], pc[0]), max(pa[0], pb[0], pc[0])
        ymn, ymx = min(pa[1], pb[1], pc[1]), max(pa[1], pb[1], pc[1])
        i0, i1 = int(np.floor(xmn / h)) - 1 - lo[0], int(np.floor(xmx / h)) + 1 - lo[0]     # a superset of the columns in the xy box
        j0, j1 = int(np.floor(ymn / h)) - 1 - lo[1], int(np.floor(ymx / h)) + 1 - lo[1]
        ii, jj = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1), indexing="ij")
        x, y = centres(lo[0] + ii, h), centres(lo[1] + jj, h)
        ok = (xmn <= x) & (x <= xmx) & (ymn <= y) & (y <= ymx)
        w = []
        for p, q in ((b, c), (c, a), (a, b)):                        # the edges opposite a, b, c
            P, Q = (p, q) if p < q else (q, p)
            dx, dy = v[Q, 0] - v[P, 0], v[Q, 1] - v[P, 1]
            e = (dx * (y - v[P, 1]) - dy * (x - v[P, 0])).astype(f32)
            rev = p > q
            tie = bool(dy < 0 or (dy == 0 and dx > 0))                # what e == 0 counts as: the sign at the column moved by (eps, eps^2)
            ok &= ((e > 0) | ((e == 0) & tie)) == ((A > 0) != rev)    # the edge's side, not the traversal, breaks the tie
            ok &= ~np.isnan(e)
            w.append(-e if rev else e)
        if not ok.any():
            continue
        wa, wb, wc = (k[ok] for k in w)
        with np.errstate(all="ignore"):
            zc = (((wa * pa[2] + wb * pb[2]).astype(f32) + wc * pc[2]).astype(f32) / ((wa + wb).astype(f32) + wc).astype(f32)).astype(f32)
        parity[ii[ok], jj[ok]] ^= zc[:, None] > cz[None, :]
        covers[ii[ok], jj[ok]] += 1
    return parity, covers


def hull_voxels(planes, lo, n, h):
    """Step 9: bool [nx,ny,nk], True where the voxel is in the hull."""
    h = f32(h)
    x = centres(lo[0] + np.arange(n[0]), h)[:, None]
    y = centres(lo[1] + np.arange(n[1]), h)[None, :]
    cz = centres(lo[2] + np.arange(n[2]), h)
    zlo = np.full((n[0], n[1]), -np.inf, f32)
    zhi = np.full((n[0], n[1]), np.inf, f32)
    keep = np.ones((n[0], n[1]), bool)
    with np.errstate(all="ignore"):
        for nx_, ny_, nz_, d in np.asarray(planes, f32):
            q = ((nx_ * x).astype(f32) + (ny_ * y).astype(f32)).astype(f32)
            r = (d - q).astype(f32)
            if nz_ < 0:
                z = (r / nz_).astype(f32)
                zlo = np.where(z > zlo, z, zlo)
            elif nz_ > 0:
                z = (r / nz_).astype(f32)
                zhi = np.where(z < zhi, z, zhi)
            else:
                keep &= q <= d
    return keep[..., None] & (zlo[..., None] <= cz) & (cz <= zhi[..., None])


def vertex_depth(v_orig, planes):
    """Step 11."""
    p = np.asarray(planes, f32)
    s = _fma(p[None, :, 2], v_orig[:, None, 2], _fma(p[None, :, 1], v_orig[:, None, 1], (p[None, :, 0] * v_orig[:, None, 0]).astype(f32)))
    g = (p[None, :, 3] - s).astype(f32)
    with np.errstate(invalid="ignore"):
        g = np.where(np.isnan(g), np.inf, g).min(axis=1)              # a NaN replaces nothing
    deep = f32(0.0)
    for x in g:
        if x > deep:
            deep = f32(x)
    return deep


def grasp_volume_one(hand, faces, loop_off, loop_vert, planes, R=None, t=None, h=0.001, voxels=False):
    """One grasp: (count, depth, status) -- with ``voxels`` also (both bool [nx,ny,nk], lo [3], v_o [V+L,3])."""
    hand = np.ascontiguousarray(hand, f32)
    V = hand.shape[0]
    extra = (None, None, None) if voxels else ()
    if not np.isfinite(hand).all():
        return (-1, f32(np.nan), 3) + extra
    if len(planes) == 0:
        return (0, f32(0.0), 1) + extra
    v = object_frame(hand, loop_off, loop_vert, R, t)
    depth = vertex_depth(v[:V], planes)
    box = box_of(v, h)
    if box is None:
        return (-1, depth, 2) + extra
    lo, n = box
    hull = hull_voxels(planes, lo, n, h)
    if not hull.any():
        return (0, f32(0.0), 1) + extra
    both = hand_voxels(v, faces, lo, n, h)[0] & hull
    return (int(both.sum()), depth, 0) + ((both, lo, v) if voxels else ())


def grasp_volume(hand, faces, loop_off, loop_vert, planes, plane_off, obj_of_row, R=None, t=None, h=0.001):
    """The batch: dict of count int32 [B], depth f32 [B], status int32 [B]; an object index out of range gives (-1, NaN, 4)."""
    hand = np.ascontiguousarray(hand, f32)
    out = []
    for b in range(hand.shape[0]):
        o = int(obj_of_row[b])
        if not 0 <= o < len(plane_off) - 1:
            out.append((-1, f32(np.nan), 4))
            continue
        pl = np.asarray(planes, f32).reshape(-1, 4)[int(plane_off[o]):int(plane_off[o + 1])]
        out.append(grasp_volume_one(hand[b], faces, loop_off, loop_vert, pl, None if R is None else R[b], t, h))
    return {"count": np.asarray([r[0] for r in out], np.int32), "depth": np.asarray([r[1] for r in out], f32),
            "status": np.asarray([r[2] for r in out], np.int32)}


# ---------------------------------------------------------------------------------------------- (b) the float64 brute force
def _point_triangle_distance(p, a, b, c):
    """Distances of points p [n,3] to the triangle (a, b, c), float64: the closest point by regions (Ericson, Real-Time Collision
    Detection 5.1.5), vectorised with clipping instead of branches."""
    ab, ac = b - a, c - a
    nrm = np.cross(ab, ac)
    ap = p - a
    # barycentric coordinates of the projection
    d00, d01, d11 = ab @ ab, ab @ ac, ac @ ac
    d20, d21 = ap @ ab, ap @ ac
    den = d00 * d11 - d01 * d01
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    inside = (v >= 0) & (w >= 0) & (v + w <= 1)
    plane = np.abs(ap @ nrm) / np.linalg.norm(nrm)

    def seg(p0, p1):
        d = p1 - p0
        s = np.clip(((p - p0) @ d) / (d @ d), 0.0, 1.0)
        return np.linalg.norm(p - (p0 + s[:, None] * d), axis=1)
    edge = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    return np.where(inside, plane, edge)


def brute_force(hand, faces, loop_off, loop_vert, planes, lo, n, R=None, t=None, h=0.001, tol=1e-6):
    """(both bool [nx,ny,nk], uncertain bool [nx,ny,nk]) over the box (lo, n) of reference (a), everything in float64: a voxel is
    in the hull iff n.x <= d for every plane, in the hand iff the ray from its centre along RAY hits an odd number of triangles.
    Uncertain: the voxels whose membership in BOTH can flip under a perturbation of ``tol`` metres -- no plane excludes the centre
    by more than ``tol``, and either the centre is within ``tol`` of a triangle, or it is within ``tol`` of a plane and in the hand.
    The hand test runs on the voxels no plane excludes by more than ``tol`` only (the others cannot be in both, nor uncertain)."""
    hand = np.asarray(hand, np.float64)
    rows = [hand] + [hand[np.asarray(loop_vert[int(loop_off[l]):int(loop_off[l + 1])], np.int64)].mean(0, keepdims=True)
                     for l in range(len(loop_off) - 1)]
    v = np.concatenate(rows)
    if R is not None:
        v = (v - (np.asarray(t, np.float64) if t is not None else 0.0)) @ np.asarray(R, np.float64)      # R^T (v - t), row-wise
    h = float(f32(h))
    axes = [(lo[k] + np.arange(n[k]) + 0.5) * h for k in range(3)]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    pl = np.asarray(planes, np.float64)
    signed = (grid @ pl[:, :3].T - pl[:, 3]) / np.linalg.norm(pl[:, :3], axis=1)       # [voxels, planes], metres
    in_hull = (signed <= 0).all(axis=1)
    near_plane = (np.abs(signed) < tol).any(axis=1)
    near_hand = np.zeros(len(grid), bool)
    tri = v[np.asarray(faces)]                                                          # [F,3,3]
    shape = tuple(n)
    for a, b, c in tri:                                                                 # near the surface: the voxels of each triangle's box
        mn, mx = np.minimum(np.minimum(a, b), c) - tol, np.maximum(np.maximum(a, b), c) + tol
        sl = [np.nonzero((axes[k] >= mn[k]) & (axes[k] <= mx[k]))[0] for k in range(3)]
        if min(len(s) for s in sl) == 0:
            continue
        idx = np.ravel_multi_index(np.meshgrid(*sl, indexing="ij"), shape).reshape(-1)
        near_hand[idx] |= _point_triangle_distance(grid[idx], a, b, c) < tol
    cand = (signed <= tol).all(axis=1)
    todo = np.nonzero(cand)[0]
    hits = np.zeros(len(todo), np.int64)
    o = grid[todo]
    for f0 in range(0, len(tri), 64):                                                   # Moeller-Trumbore, 64 triangles at a time
        a, b, c = (tri[f0:f0 + 64, k][None] for k in range(3))                          # [1,64,3]
        e1, e2 = b - a, c - a
        pv = np.cross(RAY[None, None], e2)
        det = np.einsum("ijk,ijk->ij", e1, pv)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o[:, None] - a
            u = np.einsum("ijk,ijk->ij", tv, np.broadcast_to(pv, tv.shape)) * inv
            qv = np.cross(tv, np.broadcast_to(e1, tv.shape))
            w = np.einsum("ijk,k->ij", qv, RAY) * inv
            tt = np.einsum("ijk,ijk->ij", qv, np.broadcast_to(e2, qv.shape)) * inv
        hits += ((det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (tt > 0)).sum(axis=1)
    in_hand = np.zeros(len(grid), bool)
    in_hand[todo] = hits % 2 == 1
    return (in_hull & in_hand).reshape(shape), (cand & (near_hand | (near_plane & in_hand))).reshape(shape)
