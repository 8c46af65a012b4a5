"""Numpy restatement of the articulated push-out (include/dvq.h: dvq_grasp_refine_fingers) -- test infrastructure.  The per-point
quantities are oracle/contact_oracle.py's (vertex_normals, nn_points, interior), every sum is grasp_score_ref.tree_sum, the rigid part
is grasp_refine_rigid_ref's helpers, and everything else is one fp32 operation at a time, in the header's order.

    state: grasp_refine_rigid_ref's (t, q, turned) plus q_f = (1, 0, 0, 0) and turned_f = False per finger;  hand = the hand as given
    for k = 0 .. steps:
        the rigid iterate on `hand` and its normals: o', d, j, inside, near, g, r, the 21 sums, the three counts, key, best iterate
        (the best iterate keeps q_f too);  stop at k == steps or on a NaN pen
        st, om as dvq_grasp_refine_rigid
        if curl > 0, per finger f: the four sums per set of w_j (a x g), (w_j w_j) |a|^2 over the points whose vertex is f's, a = hand[j] - c_f
            of = curl * (push * X_in / Q_in [Q_in > 0] + pull * X_nr / Q_nr [Q_nr > 0]);  if some of != 0: the candidate
            normalised (1, of / 2) (x) q_f is accepted iff its w >= min_w
        stop when st, om are all zero and no finger was accepted;  t, q as dvq_grasp_refine_rigid
        if a finger was accepted: hand = base + w (R_f (base - c_f) + c_f - base) on the vertices of turned fingers, normals recomputed

Also the float64 helpers the tests compare contact.apply_fingers / contact.compose_finger_pose with."""
import math

import numpy as np

from oracle import contact_oracle

import grasp_refine_rigid_ref as rref
import grasp_score_ref as ref

f32 = np.float32
ONE, HALF, ZERO = f32(1.0), f32(0.5), f32(0.0)
IDENT = np.asarray([1, 0, 0, 0], f32)


def min_w_of(max_curl):
    """cos(max_curl / 2) in float64, rounded once to fp32: what the host hands the kernel."""
    return f32(math.cos(0.5 * float(max_curl)))


def blend_hand(base, vert_part, vert_w, knuckle, qf, turned_f):
    """The hand of an iterate [V,3] fp32: vertices of turned fingers blended, every other vertex's bits kept."""
    hand = base.copy()
    for f in range(len(knuckle)):
        if not turned_f[f]:
            continue
        sel = np.nonzero(vert_part == f)[0]
        if sel.size == 0:
            continue
        M, c, b, w = rref.matrix(qf[f]), knuckle[f], base[sel], vert_w[sel].astype(f32)
        d = (b - c[None]).astype(f32)
        for i in range(3):
            rot = (((M[i, 0] * d[:, 0] + M[i, 1] * d[:, 1]).astype(f32) + M[i, 2] * d[:, 2]).astype(f32) + c[i]).astype(f32)
            hand[sel, i] = (b[:, i] + (w * (rot - b[:, i]).astype(f32)).astype(f32)).astype(f32)
    return hand


def finger_sums(mask, w, a, g):
    """The four sums of one (set, finger): X[3] = sum w (a x g), Q = sum (w w) |a|^2, the terms masked as (mask ? x : +0)."""
    x = rref.cross(a, g)
    q = ((w * w).astype(f32) * ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]).astype(f32) + a[:, 2] * a[:, 2]).astype(f32)).astype(f32)
    cols = [(w * x[:, 0]).astype(f32), (w * x[:, 1]).astype(f32), (w * x[:, 2]).astype(f32), q]
    return np.asarray([ref.tree_sum(np.where(mask, c, ZERO).astype(f32)) for c in cols], f32)


def refine_one(base, faces, obj, pivot, vert_part, vert_w, knuckle, steps, push, pull, spin, curl, min_w, min_contact, thr):
    """One grasp -> (offset [3], quat [4], finger_quat [P,4], iter, pen, n_in, n_ct, pen0, n_in0, n_ct0, trace); trace lists every
    iterate's (t, q, cls, pen, n_in, n_ct, q_f [P,4], accepted [P] of the step taken FROM it (None: no step), refused [P])."""
    push, pull, spin, curl, thr, min_w = f32(push), f32(pull), f32(spin), f32(curl), f32(thr), f32(min_w)
    c = np.asarray(pivot, f32)
    P = len(knuckle)
    vert_part = np.where((vert_part >= 0) & (vert_part < P), vert_part, -1)
    t, q, turned = np.zeros(3, f32), IDENT.copy(), False
    qf, turned_f = np.stack([IDENT] * P), [False] * P
    R = rref.matrix(q)
    hand = base.copy()
    best, trace, first = None, [], None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        normals = contact_oracle.vertex_normals(hand[None], faces)[0]
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
            pen = ref.tree_sum(np.where(inside | np.isnan(d), d, ZERO).astype(f32))
            S_in, S_nr = rref.set_sums(inside, g, r), rref.set_sums(near, g, r)
            n_in, n_ct, n_nr = int(inside.sum()), int((d < thr).sum()), int(near.sum())
            cls = 2 if np.isnan(pen) else (1 if n_ct < min_contact else 0)
            if k == 0:
                first = (f32(pen), n_in, n_ct)
            trace.append([t.copy(), q.copy(), cls, pen, n_in, n_ct, qf.copy(), None, None])
            if best is None or cls < best[1] or (cls == best[1] and pen < best[2]):
                best = (k, cls, pen, n_in, n_ct, t.copy(), q.copy(), qf.copy())
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
                    rref.turn_of(S_in, n_in, push, om)
                if n_nr > 0 and S_nr[9] > 0:
                    rref.turn_of(S_nr, n_nr, pull, om)
                om = (spin * om).astype(f32)
            accepted, refused = [False] * P, [False] * P
            if curl > 0:
                fj = vert_part[j]
                wj = vert_w[j].astype(f32)
                new_qf = qf.copy()
                for f in range(P):
                    mine = fj == f
                    a = (hand[j] - knuckle[f][None]).astype(f32)
                    F_in, F_nr = finger_sums(mine & inside, wj, a, g), finger_sums(mine & near, wj, a, g)
                    of = np.zeros(3, f32)
                    for i in range(3):
                        if F_in[3] > 0:
                            of[i] = f32(of[i] + f32(push * f32(F_in[i] / F_in[3])))
                        if F_nr[3] > 0:
                            of[i] = f32(of[i] + f32(pull * f32(F_nr[i] / F_nr[3])))
                    of = (curl * of).astype(f32)
                    if (of == 0).all():
                        continue
                    h, a0 = (HALF * of).astype(f32), qf[f]
                    p = np.asarray([f32(f32(f32(a0[0] - f32(h[0] * a0[1])) - f32(h[1] * a0[2])) - f32(h[2] * a0[3])),
                                    f32(f32(f32(a0[1] + f32(h[0] * a0[0])) + f32(h[1] * a0[3])) - f32(h[2] * a0[2])),
                                    f32(f32(f32(a0[2] + f32(h[1] * a0[0])) - f32(h[0] * a0[3])) + f32(h[2] * a0[1])),
                                    f32(f32(f32(a0[3] + f32(h[2] * a0[0])) + f32(h[0] * a0[2])) - f32(h[1] * a0[1]))], f32)
                    n2 = f32(f32(f32(p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3])
                    cand = (p * f32(ONE / np.sqrt(n2))).astype(f32)
                    if cand[0] >= min_w:
                        new_qf[f], accepted[f] = cand, True
                    else:
                        refused[f] = True
                qf = new_qf
            trace[-1][7], trace[-1][8] = accepted, refused
            if (st == 0).all() and (om == 0).all() and not any(accepted):
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
                R = rref.matrix(q)
            if any(accepted):
                for f in range(P):
                    turned_f[f] = turned_f[f] or accepted[f]
                hand = blend_hand(base, vert_part, vert_w, knuckle, qf, turned_f)
                normals = contact_oracle.vertex_normals(hand[None], faces)[0]
    k, cls, pen, n_in, n_ct, t, q, qf = best
    return (t, q, qf, k, f32(pen), n_in, n_ct) + first + (trace,)


NAMES = ("offset", "quat", "finger_quat", "iter", "penetration", "n_interior", "n_contact", "penetration0", "n_interior0", "n_contact0")


def grasp_refine_fingers(hand, faces, obj, pivot, vert_part, vert_w, knuckle, steps, push=1.0, pull=0.25, spin=1.0, curl=1.0,
                         max_curl=0.35, min_contact=1, contact_threshold=0.02 ** 2, traces=None):
    """The ten outputs (NAMES) of hand [B,V,3] against obj [B,N,3] about pivot [B,3] and knuckle [B,P,3]; ``traces``: a list that
    receives each grasp's trace."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    pivot, knuckle = np.ascontiguousarray(pivot, f32), np.ascontiguousarray(knuckle, f32)
    vert_part, vert_w = np.asarray(vert_part, np.int64), np.asarray(vert_w, f32)
    B, P = hand.shape[0], knuckle.shape[1]
    out = (np.zeros((B, 3), f32), np.zeros((B, 4), f32), np.zeros((B, P, 4), f32), np.zeros(B, np.int32), np.zeros(B, f32),
           np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, f32), np.zeros(B, np.int32), np.zeros(B, np.int32))
    for b in range(B):
        *vals, trace = refine_one(hand[b], faces, obj[b], pivot[b], vert_part, vert_w, knuckle[b], int(steps), push, pull, spin, curl,
                                  min_w_of(max_curl), int(min_contact), contact_threshold)
        for o, v in zip(out, vals):
            o[b] = v
        if traces is not None:
            traces.append(trace)
    return out


# ------------------------------------------------------------------------------------------------------ float64 helpers
def apply_fingers64(hand, vert_part, vert_w, knuckle, finger_quat):
    """The blend model in float64: hand [B,V,3], knuckle [B,P,3], finger_quat [B,P,4]."""
    hand, knuckle = np.asarray(hand, np.float64), np.asarray(knuckle, np.float64)
    out = hand.copy()
    R = rref.quat_matrix64(np.asarray(finger_quat, np.float64))                       # [B,P,3,3]
    for f in range(knuckle.shape[1]):
        sel = np.nonzero(np.asarray(vert_part) == f)[0]
        v, c = hand[:, sel], knuckle[:, f][:, None]
        rot = np.einsum("bij,bvj->bvi", R[:, f], v - c) + c
        out[:, sel] = v + np.asarray(vert_w, np.float64)[None, sel, None] * (rot - v)
    return out


def quat_mul64(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def compose_finger_pose64(comps, mean, global_orient, hand_pose, finger_quat, joints):
    """contact.compose_finger_pose in numpy float64: comps [45,45], mean [45], global_orient [B,3], hand_pose [B,45] (PCA),
    finger_quat [B,P,4], joints = the knuckles' joint indices."""
    comps, mean = np.asarray(comps, np.float64), np.asarray(mean, np.float64)
    full = np.asarray(hand_pose, np.float64) @ comps + mean
    q0 = rref.axis_angle_quat64(global_orient)
    q0c = q0 * np.asarray([1.0, -1.0, -1.0, -1.0])
    fq = np.asarray(finger_quat, np.float64)
    fq = fq / np.sqrt((fq * fq).sum(-1, keepdims=True))
    for f, j in enumerate(joints):
        lo = 3 * (j - 1)
        new = quat_mul64(quat_mul64(quat_mul64(q0c, fq[:, f]), q0), rref.axis_angle_quat64(full[:, lo:lo + 3]))
        full[:, lo:lo + 3] = rref.compose_orient64(np.zeros_like(full[:, lo:lo + 3]), new)
    return np.linalg.solve(comps.T, (full - mean).T).T
