"""Float64 restatement of the beam search over the prior (include/dvq.h: dvq_pixelcnn_beam), on tests/pixelcnn_ref.forward.

Plain torch, shares no code with the product.  Definition: positions 0 .. 8 in raster order; one live beam of score 0 before position
0; candidate (b, k) = score_b + log_softmax(logits_b)[k]; the min(W, live * n_in) largest survive, ties to the lower flat index
b * n_in + k; survivors in rank order (score descending, flat index ascending); rows beyond the live count hold -1 / -inf; a NaN
among a segment's candidates kills the segment (live = 0).
"""
from __future__ import annotations

from typing import Optional

import torch

import pixelcnn_ref as P

Tensor = torch.Tensor


def candidates(prev: Tensor, logits: Tensor, dtype=torch.float64) -> Tensor:
    """prev [live] scores, logits [live, n_in] -> candidate scores [live, n_in] in ``dtype`` (one addition on the log-softmax)."""
    return prev.to(dtype)[:, None] + torch.log_softmax(logits.to(dtype), dim=1)


def select(cand: Tensor, W: int) -> Tensor:
    """Flat indices of the min(W, numel) largest candidates in rank order: descending, ties to the lower flat index (-0 == +0)."""
    flat = cand.reshape(-1)
    order = torch.argsort(-flat, stable=True)
    return order[: min(W, flat.numel())]


def band_check(cand64: Tensor, survivors: Tensor, W: int, band: float, what: str = "") -> None:
    """The band rule: every survivor's float64 score >= the W-th best - band; every candidate above the W-th best + band survives."""
    flat = cand64.reshape(-1)
    n = min(W, flat.numel())
    assert survivors.numel() == n, f"{what}: {survivors.numel()} survivors, {n} expected"
    assert survivors.unique().numel() == n, f"{what}: a candidate survives twice"
    kth = torch.sort(flat, descending=True).values[n - 1]
    low = flat[survivors] < kth - band
    assert not bool(low.any()), f"{what}: survivors {survivors[low].tolist()} lie more than {band} below the {n}-th best"
    must = (flat > kth + band).nonzero().reshape(-1)
    kept = torch.zeros(flat.numel(), dtype=torch.bool)
    kept[survivors] = True
    assert bool(kept[must].all()), f"{what}: candidates {must[~kept[must]].tolist()} above the {n}-th best + {band} were dropped"


def search(logits_of, n_in: int, W: int, dtype=torch.float64):
    """One segment.  ``logits_of(prefixes [live, p] int64, p) -> [live, n_in]``.  Returns (codes [W, 9] int64, score [W] ``dtype``,
    n_live, trace) with trace = lists over the positions of (parent, token, score, cand) of that position."""
    prefixes = torch.zeros(1, 0, dtype=torch.int64)
    score = torch.zeros(1, dtype=dtype)
    trace = []
    for p in range(9):
        if prefixes.shape[0] == 0:
            break
        cand = candidates(score, logits_of(prefixes, p), dtype)
        if bool(torch.isnan(cand).any()):
            prefixes, score = torch.zeros(0, 9, dtype=torch.int64), torch.zeros(0, dtype=dtype)
            break
        idx = select(cand, W)
        parent, token = idx // n_in, idx % n_in
        score = cand.reshape(-1)[idx]
        prefixes = torch.cat([prefixes[parent], token[:, None]], dim=1)
        trace.append((parent, token, score, cand))
    live = prefixes.shape[0]
    codes = torch.full((W, 9), -1, dtype=torch.int64)
    out = torch.full((W,), float("-inf"), dtype=dtype)
    codes[:live], out[:live] = prefixes, score
    return codes, out, live, trace


def beam(sd, label: Tensor, W: int):
    """The restatement on a state_dict: label [S] -> (codes [S, W, 9], score [S, W] float64, n_live [S])."""
    n_in = sd["embedding.weight"].shape[0]
    codes, score, live = [], [], []
    for lab in label.tolist():
        def logits_of(prefixes, p):
            x = torch.zeros(prefixes.shape[0], 9, dtype=torch.int64)
            x[:, :p] = prefixes
            lab_rows = torch.full((prefixes.shape[0],), lab, dtype=torch.int64)
            out = []
            for r0 in range(0, x.shape[0], 2048):            # bounded memory: the head is 2 048 wide
                out.append(P.forward(sd, x[r0:r0 + 2048].view(-1, 3, 3), lab_rows[r0:r0 + 2048])[:, :, p // 3, p % 3])
            return torch.cat(out)
        c, s, n, _ = search(logits_of, n_in, W)
        codes.append(c), score.append(s), live.append(n)
    return torch.stack(codes), torch.stack(score), torch.tensor(live, dtype=torch.int32)


def enumerate_all(sd, lab: int, n_in: int):
    """Every grid of an ``n_in``-token prior under label ``lab``: (codes [n_in^9, 9], score [n_in^9] float64, the nine
    log-probabilities summed left to right)."""
    n = n_in ** 9
    idx = torch.arange(n)
    codes = torch.stack([(idx // n_in ** (8 - p)) % n_in for p in range(9)], dim=1)
    score = torch.zeros(n, dtype=torch.float64)
    for r0 in range(0, n, 2048):
        x = codes[r0:r0 + 2048]
        lp = torch.log_softmax(P.forward(sd, x.view(-1, 3, 3), torch.full((x.shape[0],), lab, dtype=torch.int64)), dim=1)
        lp = lp.reshape(x.shape[0], n_in, 9).gather(1, x[:, None, :])[:, 0]            # [rows, 9]
        acc = torch.zeros(x.shape[0], dtype=torch.float64)
        for p in range(9):
            acc = acc + lp[:, p]
        score[r0:r0 + 2048] = acc
    return codes, score


def duplicate_of(codes: Tensor, n_live: Tensor, slots) -> Tensor:
    """codes [S, W, 9]: per beam the rank of the FIRST better beam with the same codes at ``slots`` (flat grid positions), or -1."""
    S, W = codes.shape[:2]
    out = torch.full((S, W), -1, dtype=torch.int64)
    for s in range(S):
        seen = {}
        for r in range(int(n_live[s])):
            key = tuple(codes[s, r, list(slots)].tolist())
            if key in seen:
                out[s, r] = seen[key]
            else:
                seen[key] = r
    return out


def left_to_right_sum(lm: Tensor) -> Tensor:
    """[..., 9] -> the sum in position order in lm's own dtype (the device adds one float32 term per position)."""
    acc = lm[..., 0].clone()
    for p in range(1, lm.shape[-1]):
        acc = acc + lm[..., p]
    return acc
