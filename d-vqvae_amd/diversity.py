"""Diversity statistic of generated grasps (reference: diverse_grasp/diversity.py:7-15): k-means (20 clusters) over
the [n,61] parameter vectors, entropy of the cluster histogram and mean distance to the assigned centre.
``diversity`` is the offline analysis on the host, as in the reference (scipy: the best of 20 random starts); ``device_diversity``
is ONE deterministic Lloyd run on the device (ops.segment_kmeans) with the same two figures computed from its result."""
import json
from typing import Dict, Iterable, List, Sequence, Tuple, Union

import numpy as np
import scipy.cluster.vq
from scipy.stats import entropy


def diversity(params_list, cls_num: int = 20, seed: int = 0) -> Tuple[float, float]:
    """The paper-protocol tool: scipy's k-means (the best of 20 random starts, float64) on the host."""
    x = np.asarray(params_list, dtype=np.float64)
    codes, _ = scipy.cluster.vq.kmeans(x, cls_num, seed=seed)
    vecs, dist = scipy.cluster.vq.vq(x, codes)
    counts, _ = np.histogram(vecs, len(codes))
    return float(entropy(counts)), float(np.mean(dist))


def coverage(params_list) -> Tuple[float, float]:
    """(min, mean) over the set of each row's Euclidean distance to its nearest other row, in float64: how close the closest pair
    is, and how far apart neighbours are on average.  The plain-language counterpart of the ``novelty`` (squared, fp32) that
    ``--diverse_pool`` writes, to compare runs with; new here (the reference has the k-means statistic above only).  Fewer than two
    rows: (nan, nan)."""
    x = np.asarray(params_list, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    if x.shape[0] < 2:
        return float("nan"), float("nan")
    nearest = np.empty(x.shape[0])
    for i in range(x.shape[0]):                                   # row by row: no [n,n,D] intermediate
        d = np.sqrt(((x - x[i]) ** 2).sum(axis=1))
        d[i] = np.inf
        nearest[i] = d.min()
    return float(nearest.min()), float(nearest.mean())


def load_params(json_paths: Iterable[str]) -> np.ndarray:
    """recon_params[i][0] of every file, as diverse_grasp/diversity.py:30-41 reads them."""
    rows = []
    for p in json_paths:
        with open(p) as f:
            data = json.load(f)
        rows += [g[0] for g in data["recon_params"]]
    return np.asarray(rows)


KMEANS_INITS = ("spaced", "farthest")


def kmeans_init(n_objects: int, n_rows: int, k: int, how: str = "spaced", params=None, device=None):
    """Starting rows for ``ops.segment_kmeans``: int64 [n_objects, k] positions inside each segment of ``n_rows`` rows.
    ``"spaced"``: position floor(j * n_rows / k) for j = 0 .. k-1, the same for every segment (needs no data).
    ``"farthest"``: the first k picks of the greedy farthest-point order from row 0 (``ops.segment_diverse`` over the identity pool;
    needs ``params``, the device tensor [n_objects * n_rows, D]), which only works while n_rows is within that kernel's cap."""
    import torch
    from . import ops
    O, M, k = int(n_objects), int(n_rows), int(k)
    if O < 0 or not 1 <= k <= M:
        raise RuntimeError(f"kmeans_init: need n_objects >= 0 and 1 <= k <= n_rows (got n_objects={O} n_rows={M} k={k})")
    if how not in KMEANS_INITS:
        raise RuntimeError(f"kmeans_init: how must be one of {KMEANS_INITS} (got {how!r})")
    if device is None and params is not None:
        device = params.device
    if how == "spaced":
        pos = torch.tensor([j * M // k for j in range(k)], dtype=torch.int64)
        return pos.unsqueeze(0).repeat(O, 1).to(device if device is not None else "cpu")
    if M > ops.SEGMENT_DIVERSE_MAX_D:
        raise RuntimeError(f"kmeans_init: \"farthest\" needs n_rows <= {ops.SEGMENT_DIVERSE_MAX_D} (got {M}); use \"spaced\"")
    if params is None:
        raise RuntimeError("kmeans_init: \"farthest\" needs params, the rows to start from")
    pool = torch.arange(M, dtype=torch.int64, device=params.device).unsqueeze(0).repeat(O, 1)
    return ops.segment_diverse(params, pool, O, M, k)[1].to(torch.int64)


def kmeans_statistics(counts, dist) -> Tuple[float, float, int]:
    """(entropy, mean_dist, n_valid) of ONE segment from its cluster counts [k] and its rows' squared distances [M] (NaN for the
    rows that took no part), in numpy float64 on the host -- the same numbers whatever else shared the launch.  entropy = -sum p ln p
    over the counts > 0 with p = count / n_valid, which is ``scipy.stats.entropy(counts)``; mean_dist = the mean of sqrt(dist) over the
    valid rows.  n_valid = 0: (nan, nan, 0)."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    d = np.asarray(dist, dtype=np.float64).reshape(-1)
    n = int(c.sum())
    if n <= 0:
        return float("nan"), float("nan"), 0
    p = c[c > 0] / float(n)
    took_part = ~np.isnan(d)
    mean = float(np.sqrt(d[took_part]).sum() / n) if int(took_part.sum()) == n else float("nan")   # a valid row at a NaN distance
    return float(-(p * np.log(p)).sum()), mean, n


def segment_statistics(clusters: int, counts, dist, iters) -> List[Dict[str, object]]:
    """One dict per segment from the host copies of ``ops.segment_kmeans``'s counts [O,k], dist [O*M] and iters_used [O]."""
    counts = np.asarray(counts)
    O = counts.shape[0]
    dist = np.asarray(dist).reshape(O, -1) if O else np.zeros((0, 0))
    out = []
    for o in range(O):
        ent, mean, n = kmeans_statistics(counts[o], dist[o])
        out.append({"clusters": int(clusters), "entropy": ent, "mean_dist": mean, "iters": int(iters[o]),
                    "counts": [int(v) for v in counts[o]], "n_valid": n})
    return out


def device_diversity(params, n_objects: int, n_rows: int, cls_num: int = 20, iters: int = 100,
                     init: Union[str, object] = "spaced") -> List[Dict[str, object]]:
    """The diversity statistic of each of ``n_objects`` segments of ``n_rows`` parameter rows on the device: params fp32
    [n_objects * n_rows, D <= 64] (a CUDA/HIP tensor), one ``ops.segment_kmeans`` launch, ONE device-to-host copy of counts, dist and
    the iteration counts, the two floats on the host in float64 (kmeans_statistics).  ``init``: "spaced", "farthest" (kmeans_init) or
    an int64 tensor [n_objects, cls_num] of starting rows.  Returns one dict per segment: clusters, entropy, mean_dist, counts, iters,
    n_valid.  A segment's figures do not depend on which other segments share the call.

    This is ONE deterministic Lloyd run, reproducible to the bit.  scipy's protocol (``diversity`` above, the reference's) keeps the
    best of 20 random starts, so its figures differ slightly and vary with the seed: use ``diversity`` for numbers to set beside
    the paper's, this one to compare runs.  Vertex space (D = 2334) is out of scope."""
    import torch
    from . import ops
    O, M, k = int(n_objects), int(n_rows), int(cls_num)
    if isinstance(init, str):
        if not isinstance(params, torch.Tensor):
            raise RuntimeError("device_diversity: params must be a tensor")
        init = kmeans_init(O, M, k, init, params=params)
    elif not isinstance(init, torch.Tensor) or init.dim() != 2 or init.shape[1] != k:
        raise RuntimeError(f"device_diversity: init must be \"spaced\", \"farthest\" or an int64 tensor [n_objects, {k}]")
    _, counts, _, dist, used = ops.segment_kmeans(params, init, O, M, iters)
    pieces = [counts.reshape(-1), used, dist.view(torch.int32)]
    host = torch.cat(pieces).cpu().numpy()                          # ONE device-to-host copy
    return segment_statistics(k, host[:O * k].reshape(O, k), host[O * k + O:].view(np.float32), host[O * k:O * k + O])
