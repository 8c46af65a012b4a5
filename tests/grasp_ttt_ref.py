"""Restatements of the test-time loss and its gradient (include/dvq.h: dvq_grasp_ttt) -- test infrastructure.

``grasp_ttt``: numpy, fp32, to the bit.  The per-point figures are oracle/contact_oracle.py's (nn_points, vertex_normals, interior:
imported, the arithmetic lives there); the target-restricted minimum is ``nn_points`` against the target vertices alone, with the
indices mapped back (the targets ascend, so the first minimum is the lowest index); the sums are tests/grasp_score_ref.py's
``tree_sum``; the per-vertex sums run in ascending p in ``np.float32``:

    Gp[v] = +0.0 + (hand[v] - obj[p]) ...  over the points with inside_p and j_p == v        (fp32, ascending p)
    Gc[v] = the same over the points with contact_p and jc_p == v
    a = 2 * w_pen;  c = 2 * w_con, with mean_contact (2 * w_con) / max(n_contact, 1)
    grad[v] = fma(c, Gc[v], a * Gp[v])

``ttt_terms_t``: torch, any dtype, differentiable -- the two terms of the published TTT_loss (the sum of the squared nearest-vertex
distances over the interior object points; the sum of the squared distances to the nearest contact vertex over the object points
within the threshold of the hand), brute-force nearest neighbours, area-weighted vertex normals, the interior test against the
nearest vertex's tangent plane.  The masks and indices are recomputed (and constants of the differentiation, as boolean indexing
makes them) or frozen to given arrays."""
import numpy as np
import torch

from oracle import contact_oracle
import grasp_score_ref as score_ref

f32 = np.float32
THRESHOLD = 0.02 ** 2


def _vertex_sums(hand, obj, flag, index):
    """[V,3] fp32: for every vertex the sum from +0.0, in ascending p, of hand[v] - obj[p] over the points with flag and index == v."""
    G = np.zeros(hand.shape, f32)
    for p in np.flatnonzero(flag):
        v = index[p]
        G[v] = (G[v] + (hand[v] - obj[p]).astype(f32)).astype(f32)
    return G


def grasp_ttt(hand, faces, obj, targets=None, w_pen=None, w_con=None, mean_contact=False, contact_threshold=THRESHOLD, want_grad=True):
    """hand [B,V,3], obj [B,N,3]; ``targets``: ascending vertex indices or None.  -> dict of ``penetration``, ``contact_sum`` [B] f32,
    ``n_interior``, ``n_contact`` [B] i32, ``grad`` [B,V,3] f32 (or None), and the per-point ``j``, ``inside``, ``jc``, ``contact``
    [B,N] the gradient was gathered with (rows with a non-finite coordinate: NaN contact sum and gradient)."""
    hand, obj = np.ascontiguousarray(hand, f32), np.ascontiguousarray(obj, f32)
    B, V = hand.shape[:2]
    T = np.arange(V) if targets is None else np.asarray(targets, np.int64)
    assert T.size and np.all(np.diff(T) > 0)
    pen, n_in, n_ct = score_ref.grasp_scores(hand, faces, obj, contact_threshold)
    normals = contact_oracle.vertex_normals(hand, faces)
    with np.errstate(invalid="ignore", over="ignore"):
        d, j = contact_oracle.nn_points(obj, hand)
        inside = contact_oracle.interior(normals, hand, obj, j)
        dc, ic = contact_oracle.nn_points(obj, hand[:, T])
        jc = T[ic]
        contact = d < f32(contact_threshold)
    odd = ~(np.isfinite(hand).all((1, 2)) & np.isfinite(obj).all((1, 2)))
    con = np.asarray([f32(np.nan) if odd[b] else score_ref.tree_sum(np.where(contact[b], dc[b], f32(0.0))) for b in range(B)], f32)
    grad = None
    if want_grad:
        grad = np.full(hand.shape, np.nan, f32)
        wp = np.ones(B, f32) if w_pen is None else np.asarray(w_pen, f32)
        wc = np.ones(B, f32) if w_con is None else np.asarray(w_con, f32)
        for b in np.flatnonzero(~odd):
            Gp = _vertex_sums(hand[b], obj[b], inside[b], j[b])
            Gc = _vertex_sums(hand[b], obj[b], contact[b], jc[b])
            a = f32(2.0) * wp[b]
            c = f32(2.0) * wc[b]
            if mean_contact:
                c = f32(c / f32(max(int(n_ct[b]), 1)))
            aGp = (a * Gp).astype(f32)
            grad[b] = contact_oracle._fma(np.full_like(Gc, c), Gc, aGp)
    return {"penetration": pen, "contact_sum": con, "n_interior": n_in, "n_contact": n_ct, "grad": grad,
            "j": j, "inside": inside, "jc": jc, "contact": contact}


def combine(pen, con, n_ct, w_pen, w_con):
    """fp32: w_pen * penetration + contact_sum * (w_con / max(n_contact, 1)) -- contact.ttt_loss' expression."""
    scale = (np.full(pen.shape, w_con, f32) / np.maximum(n_ct, 1).astype(f32)).astype(f32)
    return ((pen * f32(w_pen)).astype(f32) + (con * scale).astype(f32)).astype(f32)


def vertex_normals_t(hand, faces):
    """[B,V,3] -> unit normals, area weighted (the sum of cross(v1 - v0, v2 - v0) over the incident faces, / max(|n|, 1e-6))."""
    f = torch.as_tensor(np.asarray(faces, np.int64))
    v0, v1, v2 = hand[:, f[:, 0]], hand[:, f[:, 1]], hand[:, f[:, 2]]
    fn = torch.cross(v1 - v0, v2 - v0, dim=-1)
    n = torch.zeros_like(hand)
    for c in range(3):
        n = n.index_add(1, f[:, c], fn)
    return n / n.norm(dim=-1, keepdim=True).clamp(min=1e-6)


def masks_t(hand, faces, obj, targets=None, contact_threshold=THRESHOLD):
    """The masks and indices of the published algorithm at ``hand`` (no gradient): dict of j, inside, jc, contact [B,N] tensors."""
    with torch.no_grad():
        V = hand.shape[1]
        T = torch.arange(V) if targets is None else torch.as_tensor(np.asarray(targets, np.int64))
        d2 = ((obj[:, :, None, :] - hand[:, None, :, :]) ** 2).sum(-1)
        d, j = d2.min(-1)
        jc = T[d2[:, :, T].min(-1)[1]]
        n = vertex_normals_t(hand, faces)
        rows = torch.arange(hand.shape[0])[:, None]
        inside = ((hand[rows, j] - obj) * n[rows, j]).sum(-1) > 0
        return {"j": j, "inside": inside, "jc": jc, "contact": d < contact_threshold}


def ttt_terms_t(hand, faces, obj, targets=None, contact_threshold=THRESHOLD, frozen=None):
    """(penetration [B], contact_sum [B], n_contact [B]) in ``hand``'s dtype, differentiable with respect to ``hand``.  ``frozen``: a
    dict with any of ``j``, ``inside``, ``jc``, ``contact`` (arrays or tensors [B,N]) to use in the place of the recomputed ones."""
    m = masks_t(hand.detach(), faces, obj, targets, contact_threshold)
    for k, v in (frozen or {}).items():
        m[k] = torch.as_tensor(np.asarray(v)).to(m[k].dtype)
    rows = torch.arange(hand.shape[0])[:, None]
    dp = ((obj - hand[rows, m["j"]]) ** 2).sum(-1)
    dc = ((obj - hand[rows, m["jc"]]) ** 2).sum(-1)
    zero = torch.zeros((), dtype=hand.dtype)
    return torch.where(m["inside"], dp, zero).sum(1), torch.where(m["contact"], dc, zero).sum(1), m["contact"].sum(1)


def ttt_loss_t(hand, faces, obj, targets=None, w_pen=840.0, w_con=7500.0, frozen=None):
    """[B]: w_pen * penetration + w_con * contact_sum / max(n_contact, 1)."""
    pen, con, n = ttt_terms_t(hand, faces, obj, targets, frozen=frozen)
    return w_pen * pen + w_con * con / n.clamp(min=1).to(hand.dtype)
