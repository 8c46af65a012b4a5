"""Numpy restatement of the rigid push-out (include/dvq.h: dvq_grasp_refine_rigid) -- test infrastructure.  The per-point quantities
are oracle/contact_oracle.py's (vertex_normals, nn_points, interior), every sum is grasp_score_ref.tree_sum, and everything else is
one fp32 operation at a time, in the header's order.

    t = +0, q = (1, 0, 0, 0), turned = False;  for k = 0 .. steps:
        u = obj - t;  o' = u if not turned else R^T (u - c) + c;  d, j, inside, near on o';  g = o' - hand[j];  r = hand[j] - c
        pen and, per set (inside, near): G = sum g, A = sum r, X = sum cross(r, g), Q = sum |r|^2  (21 tree sums, three counts)
        key and best iterate as dvq_grasp_refine;  stop at k == steps, on a NaN pen or when st and om are all zero
        st as dvq_grasp_refine;  om = spin * (push * (X_in - A_in x m_in) / Q_in + pull * (X_nr - A_nr x m_nr) / Q_nr), m = G / n
        t += R st (st before the first turn);  q = normalised q (x) (1, om / 2)

Also the float64 rigid-motion helpers the tests compare contact.apply_rigid / contact.compose_orient with."""
import numpy as np

from oracle import contact_oracle

import grasp_score_ref as ref

f32 = np.float32
ONE, TWO, HALF = f32(1.0), f32(2.0), f32(0.5)


def matrix(q):
    """R(q) [3,3] fp32 of q = (w, x, y, z) fp32, the header's operation order."""
    w, x, y, z = (f32(v) for v in q)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return np.asarray([[ONE - TWO * (yy + zz), TWO * (xy - wz), TWO * (xz + wy)],
                       [TWO * (xy + wz), ONE - TWO * (xx + zz), TWO * (yz - wx)],
                       [TWO * (xz - wy), TWO * (yz + wx), ONE - TWO * (xx + yy)]], f32)


def cross(a, b):
    """cross(a, b) for [..., 3] fp32 arrays or triples, each product and the difference rounded."""
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], -1).astype(f32)


def set_sums(mask, g, r):
    """The ten sums of one set: G[3], A[3], X[3], Q."""
    zero = f32(0.0)
    x = cross(r, g)
    q = ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]).astype(f32)
    cols = [g[:, 0], g[:, 1], g[:, 2], r[:, 0], r[:, 1], r[:, 2], x[:, 0], x[:, 1], x[:, 2], q]
    return np.asarray([ref.tree_sum(np.where(mask, c, zero).astype(f32)) for c in cols], f32)


def turn_of(S, n, factor, om):
    """om += factor * ((X - cross(A, m)) / Q), m = G / n, on one set's sums S."""
    n = f32(n)
    m = np.asarray([S[0] / n, S[1] / n, S[2] / n], f32)
    tau = (S[6:9] - cross(S[3:6], m)).astype(f32)
    for c in range(3):
        om[c] = f32(om[c] + f32(factor * f32(tau[c] / S[9])))


def refine_one(hand, normals, obj, pivot, steps, push, pull, spin, min_contact, thr):
    """One grasp: hand [V,3], normals [V,3], obj [N,3], pivot [3] -> (offset [3] f32, quat [4] f32, iter, pen f32, n_in, n_ct, trace):
    trace lists every iterate's (t, q, cls, pen, n_in, n_ct)."""
    push, pull, spin, thr = f32(push), f32(pull), f32(spin), f32(thr)
    c = np.asarray(pivot, f32)
    t, q, turned = np.zeros(3, f32), np.asarray([1, 0, 0, 0], f32), False
    R = matrix(q)
    best, trace = None, []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(steps + 1):
            o = (obj - t[None]).astype(f32)
            if turned:
                w = (o - c[None]).astype(f32)
                o = np.stack([((R[0, i] * w[:, 0] + R[1, i] * w[:, 1]) + R[2, i] * w[:, 2]) + c[i] for i in range(3)], 1).astype(f32)
            d, j = contact_oracle.nn_points(o[None], hand[None])
            inside = contact_oracle.interior(normals[None], hand[None], o[None], j)[0]
            d, j = d[0], j[0]
            g = (o - hand[j]).astype(f32)
            r = (hand[j] - c[None]).astype(f32)
            near = ~inside & (d < thr)
            pen = ref.tree_sum(np.where(inside | np.isnan(d), d, f32(0.0)).astype(f32))
            S_in, S_nr = set_sums(inside, g, r), set_sums(near, g, r)
            n_in, n_ct, n_nr = int(inside.sum()), int((d < thr).sum()), int(near.sum())
            cls = 2 if np.isnan(pen) else (1 if n_ct < min_contact else 0)
            trace.append((t.copy(), q.copy(), cls, pen, n_in, n_ct))
            if best is None or cls < best[1] or (cls == best[1] and pen < best[2]):
                best = (k, cls, pen, n_in, n_ct, t.copy(), q.copy())
            if k == steps or np.isnan(pen):
                break
            st, om = np.zeros(3, f32), np.zeros(3, f32)
            for i in range(3):
                if n_in > 0:
                    st[i] = f32(st[i] + f32(push * f32(S_in[i] / f32(n_in))))
                if n_nr > 0:
                    st[i] = f32(st[i] + f32(pull * f32(S_nr[i] / f32(n_nr))))
            if spin > 0:
                if n_in > 0 and S_in[9] > 0:
                    turn_of(S_in, n_in, push, om)
                if n_nr > 0 and S_nr[9] > 0:
                    turn_of(S_nr, n_nr, pull, om)
                om = (spin * om).astype(f32)
            if (st == 0).all() and (om == 0).all():
                break
            if turned:
                t = np.asarray([t[i] + ((R[i, 0] * st[0] + R[i, 1] * st[1]) + R[i, 2] * st[2]) for i in range(3)], f32)
            else:
                t = (t + st).astype(f32)
            if not (om == 0).all():
                h = (HALF * om).astype(f32)
                p = np.asarray([((q[0] - q[1] * h[0]) - q[2] * h[1]) - q[3] * h[2],
                                ((q[1] + q[0] * h[0]) + q[2] * h[2]) - q[3] * h[1],
                                ((q[2] + q[0] * h[1]) - q[1] * h[2]) + q[3] * h[0],
                                ((q[3] + q[0] * h[2]) + q[1] * h[1]) - q[2] * h[0]], f32)
                n2 = f32(f32(f32(p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3])
                q = (p * f32(ONE / np.sqrt(n2))).astype(f32)
                turned = True
                R = matrix(q)
    k, cls, pen, n_in, n_ct, t, q = best
    return t, q, k, f32(pen), n_in, n_ct, trace


def grasp_refine_rigid(hand, faces, obj, pivot, steps, push=1.0, pull=0.25, spin=1.0, min_contact=1, contact_threshold=0.02 ** 2,
                       traces=None):
    """(offset [B,3] f32, quat [B,4] f32, iter [B] i32, penetration [B] f32, n_interior [B] i32, n_contact [B] i32) of hand [B,V,3]
    against obj [B,N,3] about pivot [B,3]; ``traces``: a list that receives each grasp's trace."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    pivot = np.ascontiguousarray(pivot, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        normals = contact_oracle.vertex_normals(hand, faces)
    B = hand.shape[0]
    off, quat, it = np.zeros((B, 3), f32), np.zeros((B, 4), f32), np.zeros(B, np.int32)
    pen, n_in, n_ct = np.zeros(B, f32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        off[b], quat[b], it[b], pen[b], n_in[b], n_ct[b], trace = refine_one(hand[b], normals[b], obj[b], pivot[b], int(steps), push, pull,
                                                                             spin, int(min_contact), contact_threshold)
        if traces is not None:
            traces.append(trace)
    return off, quat, it, pen, n_in, n_ct


# ------------------------------------------------------------------------------------------------------ float64 rigid motions
def quat_angle(q):
    """The rotation angle [B] (radians, float64) of quaternions [B,4]."""
    q = np.asarray(q, np.float64)
    return 2.0 * np.arctan2(np.sqrt((q[..., 1:] ** 2).sum(-1)), np.abs(q[..., 0]))


def quat_matrix64(q):
    """Rotation matrices [B,3,3] of quaternions [B,4] (normalised here), float64."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def apply_rigid64(hand, pivot, offset, quat):
    """R (v - c) + c + t in float64: hand [B,V,3], pivot [B,3], offset [B,3], quat [B,4]."""
    hand, c, t = (np.asarray(a, np.float64) for a in (hand, pivot, offset))
    return np.einsum("bij,bvj->bvi", quat_matrix64(quat), hand - c[:, None]) + c[:, None] + t[:, None]


def axis_angle_quat64(a):
    """Axis-angle [B,3] -> unit quaternions [B,4], float64."""
    a = np.asarray(a, np.float64)
    th = np.sqrt((a * a).sum(-1, keepdims=True))
    k = np.where(th < 1e-6, 0.5 - th * th / 48.0, np.sin(0.5 * th) / np.where(th < 1e-6, 1.0, th))
    return np.concatenate([np.cos(0.5 * th), k * a], -1)


def compose_orient64(global_orient, quat):
    """The axis-angle [B,3] of Q * exp(global_orient), float64, through quaternions; w >= 0, angle = 2 atan2(|v|, w)."""
    a, b = np.asarray(quat, np.float64), axis_angle_quat64(global_orient)
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    p = np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                  aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)
    p = np.where(p[..., :1] < 0, -p, p)
    n = np.sqrt((p[..., 1:] ** 2).sum(-1, keepdims=True))
    safe = np.where(n > 0, n, 1.0)
    return np.where(n > 0, 2.0 * np.arctan2(n, p[..., :1]) / safe, 0.0) * p[..., 1:]
