"""Float64 restatement of the controlled prior draw (include/dvq.h: dvq_pixelcnn_sample_ctl), one grid position
of a batch at a time, in torch so that it runs where its inputs live.  Only the scaling s = l / T is done in float32, because the
definition says so (it fixes the kept set); everything after it is evaluated in ``dtype``.

    s      = l / T                                      (fp32)
    S      = the top_k largest s, ties towards the lowest index (all tokens when top_k is 0 or >= n)
    p      = softmax of s over S
    code   = argmax_{k in S} p_k / q_k, lowest k on ties; or the given code where given >= 0
    logp_model = l[code] - logsumexp_k l[k]
    logp_draw  = s[code] - logsumexp_{k in S} s[k]      (-inf for a given code outside S)
    a row with a NaN logit: code -1 where drawn, both log-probabilities NaN
"""
from types import SimpleNamespace

import torch


def kept_set(s32: torch.Tensor, top_k: int) -> torch.Tensor:
    """[B,n] bool: the top_k largest entries of each row, ties towards the lowest index (exactly top_k per row)."""
    n = s32.shape[1]
    if not 0 < top_k < n:
        return torch.ones_like(s32, dtype=torch.bool)
    thr = torch.topk(s32, top_k, dim=1).values[:, -1:]              # the top_k-th largest value
    above, eq = s32 > thr, s32 == thr
    need = top_k - above.sum(dim=1, keepdim=True)
    return above | (eq & (torch.cumsum(eq.to(torch.int64), dim=1) <= need))


def draw(logits: torch.Tensor, q: torch.Tensor, temperature: float = 1.0, top_k: int = 0, given=None, dtype=torch.float64):
    """logits [B,n] fp32, q [B,n] Exp(1) noise, given [B] int64 (negative: draw) or None ->
    code [B] int64, kept [B,n] bool, logp_model / logp_draw [B] ``dtype``, gap [B]: (best - second best) / best race score."""
    l32 = logits.to(torch.float32)
    # a one-element TENSOR divisor: a Python scalar may be turned into a multiplication by its reciprocal
    s32 = l32 / torch.tensor([temperature], dtype=torch.float32, device=l32.device)
    B, n = s32.shape
    nan_row = torch.isnan(l32).any(dim=1)
    s32 = torch.where(nan_row[:, None], torch.zeros_like(s32), s32)     # keeps the helpers below defined; overwritten at the end
    kept = kept_set(s32, top_k)
    s, l, qd = s32.to(dtype), torch.where(nan_row[:, None], torch.zeros_like(l32), l32).to(dtype), q.to(dtype)
    ninf = torch.full_like(s, float("-inf"))
    mx = torch.where(kept, s, ninf).max(dim=1, keepdim=True).values
    e = torch.where(kept, torch.exp(s - mx), torch.zeros_like(s))
    Z = e.sum(dim=1, keepdim=True)
    score = torch.where(kept, (e / Z) / qd, ninf)
    code = torch.argmax(score, dim=1)                                   # the first of equal maxima
    if n > 1:
        top2 = torch.topk(score, 2, dim=1).values
        gap = (top2[:, 0] - top2[:, 1]) / top2[:, 0]
    else:
        gap = torch.full((B,), float("inf"), dtype=dtype, device=s.device)
    drawn = torch.ones(B, dtype=torch.bool, device=s.device)
    if given is not None:
        drawn = given < 0
        code = torch.where(drawn, code, given)
    c = code[:, None]
    lse_l = torch.logsumexp(l, dim=1)
    logp_model = l.gather(1, c)[:, 0] - lse_l
    logp_draw = torch.where(kept.gather(1, c)[:, 0], s.gather(1, c)[:, 0] - (mx[:, 0] + torch.log(Z[:, 0])),
                            torch.full_like(lse_l, float("-inf")))
    nan = torch.full_like(lse_l, float("nan"))
    return SimpleNamespace(code=torch.where(nan_row & drawn, torch.full_like(code, -1), code), kept=kept,
                           logp_model=torch.where(nan_row, nan, logp_model), logp_draw=torch.where(nan_row, nan, logp_draw),
                           gap=gap, drawn=drawn)
