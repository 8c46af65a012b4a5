"""Two references for dvq_grasp_mesh_volume (include/dvq.h) -- test infrastructure.

(a) ``grasp_mesh_volume``: the header's definition in numpy fp32, operation for operation.  The hand's side (steps 1 - 8) is
    grasp_volume_ref's; the object's side (step 9') applies the same rules 4 - 7 to the object's faces with the edges ordered by the
    LOCAL vertex index, the face's column range cut to the box in float before any conversion to an integer, and the rule that a face
    wholly at or below the lowest cell centre never counts.  It follows the DEFINITION, not the kernel: a dense parity array over the
    box, no tiles, no bit words, no cull list.  GPU results are compared with it exactly.
(b) ``brute_force``: an independent float64 evaluation -- inside the hand by the parity of Moeller-Trumbore hits along the oblique ray
    of grasp_volume_ref.brute_force, inside the object by the generalised winding number of grasp_mesh_ref -- with the UNCERTAIN
    voxels: centres within ``tol`` of either surface, where fp32 and float64 may legitimately disagree.
"""
import numpy as np

import grasp_mesh_ref as mref
import grasp_volume_ref as vref
from grasp_volume_ref import centres, f32

MAX_FACES = mref.MAX_FACES


# ---------------------------------------------------------------------------------------------- meshes for the tests
def torus(n_major=16, n_minor=8, R=0.05, r=0.015, centre=(0.0, 0.0, 0.0)):
    """Closed torus about the z axis, outward winding: n_major * n_minor vertices, 2 * n_major * n_minor faces."""
    u = np.linspace(0, 2 * np.pi, n_major, endpoint=False)[:, None]
    w = np.linspace(0, 2 * np.pi, n_minor, endpoint=False)[None, :]
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w) * np.ones_like(u)], axis=-1)
    idx = lambda i, j: (i % n_major) * n_minor + (j % n_minor)
    f = []
    for i in range(n_major):
        for j in range(n_minor):
            f.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            f.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
    return (v.reshape(-1, 3) + np.asarray(centre)).astype(f32), np.asarray(f, np.int64)


def box(half, centre=(0.0, 0.0, 0.0)):
    """Closed axis-aligned box of 8 vertices and 12 faces, outward winding."""
    half = np.broadcast_to(np.asarray(half, np.float64), (3,))
    s = np.asarray([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)
    f = [[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]]
    return (s * half + np.asarray(centre)).astype(f32), np.asarray(f, np.int64)


def pack(meshes):
    """[(verts, faces)] -> (mesh_verts f32 [n,3], vert_off int32 [O+1], mesh_faces int32 [m,3], face_off int32 [O+1])."""
    vo, fo = np.cumsum([0] + [len(v) for v, _ in meshes]), np.cumsum([0] + [len(f) for _, f in meshes])
    verts = np.concatenate([np.asarray(v, f32).reshape(-1, 3) for v, _ in meshes]) if meshes else np.zeros((0, 3), f32)
    faces = np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes]) if meshes else np.zeros((0, 3), np.int32)
    return verts.astype(f32), vo.astype(np.int32), faces.astype(np.int32), fo.astype(np.int32)


# ---------------------------------------------------------------------------------------------- (a) the definition in fp32
def _span(mn, mx, h, a, b):
    """floorf(mn / h) - 1 .. floorf(mx / h) + 1 cut to [a, b] in fp32, then integers; None when empty."""
    with np.errstate(all="ignore"):
        f0 = max(f32(np.floor(f32(mn) / h) - f32(1)), f32(a))
        f1 = min(f32(np.floor(f32(mx) / h) + f32(1)), f32(b))
    return (int(f0), int(f1)) if f0 <= f1 else None


def object_voxels(mv, faces, lo, n, h):
    """Step 9': (bool [nx,ny,nk], True where the voxel is in the object; the number of covering faces per column; whether a face
    index was out of range)."""
    h = f32(h)
    mv = np.ascontiguousarray(mv, f32)
    cz = centres(lo[2] + np.arange(n[2]), h)
    zbot = cz[0]
    parity = np.zeros(tuple(n), bool)
    covers = np.zeros((n[0], n[1]), np.int64)
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
            if pa[2] <= zbot and pb[2] <= zbot and pc[2] <= zbot:        # wholly at or below the lowest cell centre: never counts
                continue
            xmn, xmx = min(pa[0], pb[0], pc[0]), max(pa[0], pb[0], pc[0])
            ymn, ymx = min(pa[1], pb[1], pc[1]), max(pa[1], pb[1], pc[1])
            si, sj = _span(xmn, xmx, h, lo[0], lo[0] + n[0] - 1), _span(ymn, ymx, h, lo[1], lo[1] + n[1] - 1)
            if si is None or sj is None:
                continue
            ii, jj = np.meshgrid(np.arange(si[0], si[1] + 1) - lo[0], np.arange(sj[0], sj[1] + 1) - lo[1], indexing="ij")
            x, y = centres(lo[0] + ii, h), centres(lo[1] + jj, h)
            ok = (xmn <= x) & (x <= xmx) & (ymn <= y) & (y <= ymx)
            w = []
            for p, q in ((b, c), (c, a), (a, b)):                        # the edges opposite a, b, c
                P, Q = (p, q) if p < q else (q, p)
                dx, dy = f32(mv[Q, 0] - mv[P, 0]), f32(mv[Q, 1] - mv[P, 1])
                e = ((dx * (y - mv[P, 1]).astype(f32)).astype(f32) - (dy * (x - mv[P, 0]).astype(f32)).astype(f32)).astype(f32)
                rev = p > q
                tie = bool(dy < 0 or (dy == 0 and dx > 0))
                ok &= ((e > 0) | ((e == 0) & tie)) == ((A > 0) != rev)
                ok &= ~np.isnan(e)
                w.append(-e if rev else e)
            if not ok.any():
                continue
            wa, wb, wc = (k[ok] for k in w)
            zc = (((wa * pa[2]).astype(f32) + (wb * pb[2]).astype(f32)).astype(f32) + (wc * pc[2]).astype(f32)).astype(f32) \
                / ((wa + wb).astype(f32) + wc).astype(f32)
            parity[ii[ok], jj[ok]] ^= zc.astype(f32)[:, None] > cz[None, :]
            covers[ii[ok], jj[ok]] += 1
    return parity, covers, bad


def grasp_mesh_volume_one(hand, faces, loop_off, loop_vert, mv, mf, R=None, t=None, h=0.001, voxels=False):
    """One grasp against one object's vertices ``mv`` and LOCAL faces ``mf``: (count, status, a face index was out of range) -- with
    ``voxels`` also (both, in the hand, in the object: bool [nx,ny,nk]; lo [3]; v_o [V+L,3])."""
    hand = np.ascontiguousarray(hand, f32)
    extra = (None,) * 5 if voxels else ()
    if not np.isfinite(hand).all():
        return (-1, 3, False) + extra
    if len(mf) == 0:
        return (0, 1, False) + extra
    v = vref.object_frame(hand, loop_off, loop_vert, R, t)
    got = vref.box_of(v, h)
    if got is None:
        return (-1, 2, False) + extra
    lo, n = got
    obj, _, bad = object_voxels(mv, mf, lo, n, h)
    if not obj.any():
        return (0, 1, bad) + extra
    in_hand = vref.hand_voxels(v, faces, lo, n, h)[0]
    both = in_hand & obj
    return (int(both.sum()), 0, bad) + ((both, in_hand, obj, lo, v) if voxels else ())


def grasp_mesh_volume(hand, faces, loop_off, loop_vert, mesh_verts, vert_off, mesh_faces, face_off, obj_of_row, R=None, t=None, h=0.001):
    """The batch: dict of count, status int32 [B] and ``err``, the bits of the error flag the object's side sets."""
    hand = np.ascontiguousarray(hand, f32)
    mesh_verts, mesh_faces = np.asarray(mesh_verts, f32).reshape(-1, 3), np.asarray(mesh_faces).reshape(-1, 3)
    B, O = hand.shape[0], len(vert_off) - 1
    out = {"count": np.zeros(B, np.int32), "status": np.zeros(B, np.int32), "err": 0}
    for b in range(B):
        o = int(obj_of_row[b])
        ranges_ok = False
        if 0 <= o < O:
            v0, nv = int(vert_off[o]), int(vert_off[o + 1]) - int(vert_off[o])
            f0, nf = int(face_off[o]), int(face_off[o + 1]) - int(face_off[o])
            ranges_ok = (nv >= 0 and 0 <= nf <= MAX_FACES and 0 <= v0 <= len(mesh_verts) - nv and 0 <= f0 <= len(mesh_faces) - nf)
        if not ranges_ok:
            out["err"] |= 2 if 0 <= o < O else 1
            out["count"][b], out["status"][b] = -1, 4
            continue
        count, status, bad = grasp_mesh_volume_one(hand[b], faces, loop_off, loop_vert, mesh_verts[v0:v0 + nv], mesh_faces[f0:f0 + nf],
                                                   None if R is None else R[b], t, h)
        out["count"][b], out["status"][b] = count, status
        if bad:
            out["err"] |= 2
    return out


# ---------------------------------------------------------------------------------------------- (b) the float64 brute force
def brute_force(hand, faces, loop_off, loop_vert, mv, mf, lo, n, R=None, t=None, h=0.001, tol=1e-6):
    """(both bool [nx,ny,nk], uncertain bool [nx,ny,nk]) over the box (lo, n) of reference (a), everything in float64.  In the hand:
    grasp_volume_ref.brute_force's oblique ray (its hull: the object's padded bounding box).  In the object: |winding number| > 1/2, on the
    voxels in or near the hand only (no other voxel can be in both, nor uncertain).  Uncertain: within ``tol`` metres of the hand's
    surface, or in the hand and within ``tol`` of the object's."""
    mv, mf = np.asarray(mv, np.float64), np.asarray(mf).reshape(-1, 3)
    # the hand test runs inside the object's bounding box, padded well beyond ``tol``: no voxel outside it is in the object or near it
    pad = 64.0 * tol
    around = np.concatenate([np.concatenate([np.eye(3), (mv.max(0) + pad)[:, None]], axis=1),
                             np.concatenate([-np.eye(3), (pad - mv.min(0))[:, None]], axis=1)])
    in_hand, near_hand = vref.brute_force(hand, faces, loop_off, loop_vert, around, lo, n, R, t, h, tol)
    hh = float(f32(h))
    axes = [(lo[k] + np.arange(n[k]) + 0.5) * hh for k in range(3)]
    todo = np.nonzero((in_hand | near_hand).reshape(-1))[0]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)[todo]
    in_obj = np.zeros(len(todo), bool)
    for s in range(0, len(todo), 4096):                                # (the winding number's temporaries are [points, faces, 3])
        in_obj[s:s + 4096] = np.abs(mref.winding_number(grid[s:s + 4096], mv, mf)) > 0.5
    near_obj = mref.surface_distance(grid, mv, mf) < tol
    both, uncertain = np.zeros(in_hand.size, bool), np.zeros(in_hand.size, bool)
    both[todo] = in_hand.reshape(-1)[todo] & in_obj
    uncertain[todo] = (near_hand.reshape(-1)[todo] & (in_obj | near_obj)) | (near_obj & in_hand.reshape(-1)[todo])
    return both.reshape(in_hand.shape), uncertain.reshape(in_hand.shape)
