"""numpy restatement of dvq_segment_kmeans (include/dvq.h): the eight-chain squared distance of the diverse selection, the
lowest-index argmin, the four-chain centre sums and the Lloyd loop -- test infrastructure.  Every operation is a numpy float32
operation, so each is rounded on its own; a chain is a sequential ``cumsum(dtype=float32)`` from +0.0."""
import numpy as np

from diverse_select_ref import dist2

F32 = np.float32


def assign_rows(x, centres, valid):
    """x [M,D], centres [k,D], valid [M] -> (assign int32 [M], dist float32 [M]); invalid rows: -1, NaN."""
    M = x.shape[0]
    assign, best = np.full(M, -1, np.int32), np.full(M, np.nan, F32)
    rows = np.flatnonzero(valid)
    if rows.size:
        xv = x[rows]
        a, d = np.zeros(rows.size, np.int32), dist2(xv, centres[0])
        for j in range(1, centres.shape[0]):
            dj = dist2(xv, centres[j])
            with np.errstate(invalid="ignore"):
                take = (dj < d) | (np.isnan(d) & ~np.isnan(dj))
            a[take], d[take] = j, dj[take]
        assign[rows], best[rows] = a, d
    return assign, best


def chain_sum(v):
    """[n,D] float32 -> [D]: +0.0f, then the rows added one at a time."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumsum(np.concatenate([np.zeros((1, v.shape[1]), F32), v]), axis=0, dtype=F32)[-1]


def update_centres(x, assign, centres):
    """(new centres [k,D], counts int32 [k]): four chains over the positions i = g (mod 4), S = (ch0 + ch1) + (ch2 + ch3), S / count."""
    k = centres.shape[0]
    new, counts = centres.copy(), np.zeros(k, np.int32)
    pos = np.arange(x.shape[0])
    for c in range(k):
        mine = assign == c
        counts[c] = int(mine.sum())
        if counts[c] == 0:
            continue
        ch = [chain_sum(x[mine & (pos % 4 == g)]) for g in range(4)]
        with np.errstate(invalid="ignore", over="ignore"):
            s = ((ch[0] + ch[1]).astype(F32) + (ch[2] + ch[3]).astype(F32)).astype(F32)
            new[c] = (s / F32(counts[c])).astype(F32)
    return new, counts


def bad_init(x, init):
    """True when the kernel must refuse ``init``: an entry outside [0, M), a repeated entry or the position of an invalid row."""
    x, init = np.asarray(x, F32), np.asarray(init, np.int64)
    if init.min() < 0 or init.max() >= x.shape[0] or len(set(init.tolist())) != init.size:
        return True
    return not np.isfinite(x[init]).all()


def kmeans_one(x, init, iters):
    """x [M,D] float32, init [k] -> (centres [k,D], counts int32 [k], assign int32 [M], dist float32 [M], iters_used); a bad init:
    -1 in the integers, NaN in the floats."""
    x = np.asarray(x, F32)
    init = np.asarray(init, np.int64)
    if bad_init(x, init):
        M, k = x.shape[0], init.size
        return np.full((k, x.shape[1]), np.nan, F32), np.full(k, -1, np.int32), np.full(M, -1, np.int32), np.full(M, np.nan, F32), -1
    valid = np.isfinite(x).all(axis=1)
    centres = x[init].copy()
    assign, dist = assign_rows(x, centres, valid)
    used = int(iters)
    for u in range(1, int(iters) + 1):
        centres, _ = update_centres(x, assign, centres)
        new, dist = assign_rows(x, centres, valid)
        same = np.array_equal(new, assign)
        assign = new
        if same:
            used = u
            break
    counts = np.bincount(assign[assign >= 0], minlength=centres.shape[0]).astype(np.int32)
    return centres, counts, assign, dist, used


def segment_kmeans(feat, init, n_objects, n_rows, iters):
    """feat [O*M,D] float32, init [O,k] int64 -> (centres [O,k,D], counts [O,k], assign [O*M], dist [O*M], iters_used [O])."""
    feat, init = np.asarray(feat, F32), np.asarray(init, np.int64)
    O, M = int(n_objects), int(n_rows)
    k, D = init.shape[1], feat.shape[1]
    assert feat.shape[0] == O * M and init.shape[0] == O and 1 <= k <= M
    centres, counts = np.zeros((O, k, D), F32), np.zeros((O, k), np.int32)
    assign, dist, used = np.zeros(O * M, np.int32), np.zeros(O * M, F32), np.zeros(O, np.int32)
    for o in range(O):
        centres[o], counts[o], assign[o * M:(o + 1) * M], dist[o * M:(o + 1) * M], used[o] = kmeans_one(feat[o * M:(o + 1) * M], init[o], iters)
    return centres, counts, assign, dist, used


def statistics(counts, dist):
    """The two figures of diverse_grasp/diversity.py from one segment's counts [k] and dist [M], in float64: the entropy of the
    cluster histogram (natural logarithm, over the valid rows) and the mean Euclidean distance to the assigned centre."""
    counts, d = np.asarray(counts, np.float64), np.asarray(dist, np.float64)
    n = counts.sum()
    if n == 0:
        return float("nan"), float("nan")
    p = counts[counts > 0] / n
    return float(-(p * np.log(p)).sum()), float(np.sqrt(d[~np.isnan(d)]).mean())           # no valid row at a NaN distance assumed
