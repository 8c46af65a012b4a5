"""numpy restatement of dvq_segment_diverse (include/dvq.h): the eight-chain squared distance and the greedy farthest-point order
inside a quality pool -- test infrastructure.  Every operation is a numpy float32 operation, so each is rounded on its own."""
import numpy as np

F32 = np.float32


def dist2(x, c):
    """x [P,D], c [D] float32 -> [P] float32: d(x_i, c).  Zero-padding to a multiple of eight adds +0.0 to non-negative sums: the
    bits of the definition, whose tail chains simply stop earlier."""
    x, c = np.asarray(x, F32), np.asarray(c, F32)
    P, D = x.shape
    Dp = -(-D // 8) * 8
    xp, cp = np.zeros((P, Dp), F32), np.zeros(Dp, F32)
    xp[:, :D], cp[:D] = x, c
    acc = np.zeros((P, 8), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, Dp, 8):
            t = (xp[:, s:s + 8] - cp[s:s + 8]).astype(F32)
            acc = (acc + (t * t).astype(F32)).astype(F32)
        a = (acc[:, 0::2] + acc[:, 1::2]).astype(F32)            # (0+1) (2+3) (4+5) (6+7)
        b = (a[:, 0::2] + a[:, 1::2]).astype(F32)
        return (b[:, 0] + b[:, 1]).astype(F32)


def select_one(rows, keep):
    """rows [P,D] in pool order -> (positions int32 [keep], gap float32 [keep])."""
    rows = np.asarray(rows, F32)
    P = rows.shape[0]
    valid = np.isfinite(rows).all(axis=1)
    picked = np.zeros(P, bool)
    pos, gap = np.zeros(keep, np.int32), np.full(keep, -1.0, F32)
    picked[0] = True
    mind = dist2(rows, rows[0])
    for r in range(1, keep):
        key = np.where(valid & ~picked & ~np.isnan(mind), mind, F32(-1.0)).astype(F32)
        key[picked] = -2.0                                        # never chosen: keep <= P leaves an unpicked position
        p = int(np.argmax(key))                                   # the first maximum: the lowest pool position wins ties
        pos[r], gap[r] = p, key[p]
        picked[p] = True
        d = dist2(rows, rows[p])
        with np.errstate(invalid="ignore"):
            mind = np.where(d < mind, d, mind).astype(F32)        # a NaN never lowers anything
    return pos, gap


def segment_diverse(feat, pool, n_objects, n_candidates, keep):
    """feat [O*M,D] float32, pool [O,P] int64 -> (sel int64, rank int32, gap float32), each [O,keep]."""
    feat, pool = np.asarray(feat, F32), np.asarray(pool, np.int64)
    O, M = int(n_objects), int(n_candidates)
    assert feat.shape[0] == O * M and pool.shape[0] == O and 1 <= keep <= pool.shape[1] <= M
    sel, rank, gap = np.zeros((O, keep), np.int64), np.zeros((O, keep), np.int32), np.zeros((O, keep), F32)
    for o in range(O):
        assert pool[o].min() >= 0 and pool[o].max() < M
        rank[o], gap[o] = select_one(feat[o * M + pool[o]], keep)
        sel[o] = pool[o][rank[o]]
    return sel, rank, gap
