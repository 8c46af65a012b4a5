"""Float64 reference of the gated PixelCNN prior and the weight families of tests/test_pixelcnn_fp64.py.

Plain torch in float64, functional over a ``state_dict``; shares no code with the oracle (oracle/dvq_oracle.py) or with the product's
packer.  Geometry and masks follow the reference's network/pixelcnn/models.py:30-88,161-174: layer 0 has k = 5 and mask A (last kernel
row of ``vert_stack`` and last kernel column of ``horiz_stack`` zero, on a copy), the layers after it k = 3; ``vert_to_horiz`` acts on
the pre-gate ``h_vert``; the residual applies for layers >= 1 only; the head is conv, ReLU, conv.  Every convolution is written as a
sum of one matrix product per kernel tap over a zero-padded channels-last grid, so nothing here goes through ``F.conv2d``.  Rows of the
batch are independent: a subset of rows is evaluated by passing ``x[rows]``, ``label[rows]``.

There is no condition scale for this network (a forward-propagated one reaches 1e37 at 15 layers): the tests take their tolerance from
the fp32 oracle's own distance to this reference.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from dvqvae_amd import synth

Tensor = torch.Tensor
SEED = 1234                      # the goldens' seed (tests/conftest.py)
N_HIDDEN = 2048
# (n_in, dim, n_layers, n_classes) -> seed of the weights; the first and the last are the goldens' networks at the goldens' seeds
SIZES = {(32, 64, 3, 16): SEED + 1, (100, 64, 2, 8): SEED + 3, (64, 128, 4, 8): SEED + 4, (512, 512, 15, 128): SEED + 2}
FULL = (512, 512, 15, 128)
FAMILIES = ("base", "hot", "dead", "grow", "gauge", "gauge_far")
DEAD_FRACTION = 0.06
DEAD_HEAD_ZERO, DEAD_HEAD_BIAS = 3, 5        # family "dead": output_conv.2 rows that are always zero, without / with a live bias
GROW = 4.0
FAR_SHIFT = 8                    # family "gauge_far": the residual exponents of "gauge" plus this, 2 .. 18


# ----------------------------------------------------------------------------------------------------------------- weights
def n_layers(sd) -> int:
    n = 0
    while f"layers.{n}.vert_stack.weight" in sd:
        n += 1
    return n


def template(size: Tuple[int, int, int, int]) -> Dict[str, Tensor]:
    """Zero tensors shaped like ``GatedPixelCNN(*size).state_dict()``."""
    n_in, dim, L, n_cls = size
    shapes = {"embedding.weight": (n_in, dim)}
    for i in range(L):
        k = 5 if i == 0 else 3
        p = f"layers.{i}."
        shapes[p + "class_cond_embedding.weight"] = (n_cls, 2 * dim)
        shapes[p + "vert_stack.weight"] = (2 * dim, dim, k // 2 + 1, k)
        shapes[p + "vert_stack.bias"] = (2 * dim,)
        shapes[p + "vert_to_horiz.weight"] = (2 * dim, 2 * dim, 1, 1)
        shapes[p + "vert_to_horiz.bias"] = (2 * dim,)
        shapes[p + "horiz_stack.weight"] = (2 * dim, dim, 1, k // 2 + 1)
        shapes[p + "horiz_stack.bias"] = (2 * dim,)
        shapes[p + "horiz_resid.weight"] = (dim, dim, 1, 1)
        shapes[p + "horiz_resid.bias"] = (dim,)
    shapes["output_conv.0.weight"] = (N_HIDDEN, dim, 1, 1)
    shapes["output_conv.0.bias"] = (N_HIDDEN,)
    shapes["output_conv.2.weight"] = (n_in, N_HIDDEN, 1, 1)
    shapes["output_conv.2.bias"] = (n_in,)
    return {k: torch.zeros(v) for k, v in shapes.items()}


def _pow2(shape, seed, name, lo: int, hi: int) -> Tensor:
    """2^k, k integer and uniform in lo .. hi, float32 (exact)."""
    k = torch.floor(synth.synthetic_uniform(shape, seed, name, float(lo), float(hi + 1))).clamp(lo, hi)
    return (2.0 ** k.double()).float()


def _rows(t: Tensor, s: Tensor) -> Tensor:
    return t * s.reshape((-1,) + (1,) * (t.dim() - 1))


def _cols(t: Tensor, s: Tensor) -> Tensor:
    return t * s.reshape((1, -1) + (1,) * (t.dim() - 2))


def weights(family: str, size: Tuple[int, int, int, int]) -> Dict[str, Tensor]:
    """The state_dict of a family (module docstring of tests/test_pixelcnn_fp64.py) at one of SIZES."""
    assert family in FAMILIES, family
    seed = SIZES[size]
    n_in, dim, L, _ = size
    sd = synth.synthetic_state_dict(template(size), seed)
    tag = "pcnn64/"
    if family == "hot":
        for k in sd:
            if k.endswith("class_cond_embedding.weight"):
                sd[k] = synth.synthetic_normal(sd[k].shape, seed, tag + k + ".hot", 3.0)
            elif k.endswith(".bias"):
                sd[k] = synth.synthetic_normal(sd[k].shape, seed, tag + k + ".hot", 1.0)
            elif k.split(".")[-2] in ("vert_stack", "horiz_stack", "vert_to_horiz"):
                sd[k] = sd[k] * 4.0
    if family == "dead":
        for k in [k for k in sd if k.endswith(".weight")]:
            u = synth.synthetic_uniform((sd[k].shape[0],), seed, tag + k + ".dead", 0.0, 1.0)
            if k == "output_conv.2.weight":
                u[DEAD_HEAD_ZERO], u[DEAD_HEAD_BIAS] = 0.0, 0.75 * DEAD_FRACTION
            sd[k][u < DEAD_FRACTION] = 0.0
            b = k[: -len("weight")] + "bias"
            if b in sd:
                sd[b][u < DEAD_FRACTION / 2] = 0.0
    if family == "grow":
        for i in range(L):
            sd[f"layers.{i}.horiz_resid.weight"] = sd[f"layers.{i}.horiz_resid.weight"] * GROW
    if family in ("gauge", "gauge_far"):
        shift = FAR_SHIFT if family == "gauge_far" else 0
        s = _pow2((dim,), seed, tag + "gauge.stream", -6, 10) * 2.0 ** shift           # residual stream, per channel
        for i in range(L):
            p = f"layers.{i}.horiz_resid."
            sd[p + "weight"], sd[p + "bias"] = _rows(sd[p + "weight"], s), sd[p + "bias"] * s
            if i >= 1:
                sd[f"layers.{i}.horiz_stack.weight"] = _cols(sd[f"layers.{i}.horiz_stack.weight"], 1.0 / s)
        sd["output_conv.0.weight"] = _cols(sd["output_conv.0.weight"], 1.0 / s)
        h = _pow2((N_HIDDEN,), seed, tag + "gauge.head", -10, 10)                       # head, per hidden unit (ReLU is homogeneous)
        sd["output_conv.0.weight"], sd["output_conv.0.bias"] = _rows(sd["output_conv.0.weight"], h), sd["output_conv.0.bias"] * h
        sd["output_conv.2.weight"] = _cols(sd["output_conv.2.weight"], 1.0 / h)
        e = _pow2((dim,), seed, tag + "gauge.token", -8, 8)                             # token embedding, per channel
        sd["embedding.weight"] = _cols(sd["embedding.weight"], e)
        for stack in ("vert_stack", "horiz_stack"):
            sd[f"layers.0.{stack}.weight"] = _cols(sd[f"layers.0.{stack}.weight"], 1.0 / e)
    return sd


def dead_head_rows(sd) -> Tuple[Tensor, Tensor]:
    """Family "dead": (logits whose output_conv.2 row and bias are zero, logits whose row is zero under a live bias)."""
    zero = (sd["output_conv.2.weight"].reshape(sd["output_conv.2.weight"].shape[0], -1) == 0).all(dim=1)
    live = sd["output_conv.2.bias"] != 0
    return (zero & ~live).nonzero().reshape(-1), (zero & live).nonzero().reshape(-1)


# --------------------------------------------------------------------------------------------------------------- reference
def _taps(h: Tensor, W: Tensor, top: int, left: int) -> Tensor:
    """Cross-correlation of a channels-last grid h [B, H, W, C] with W [O, C, kh, kw]: out[i, j] = sum_ab W[:, :, a, b] h[i + a - top,
    j + b - left], zero outside the grid."""
    B, H, Wd, C = h.shape
    O, _, kh, kw = W.shape
    hp = torch.zeros(B, H + kh - 1, Wd + kw - 1, C, dtype=h.dtype, device=h.device)
    hp[:, top:top + H, left:left + Wd] = h
    out = torch.zeros(B * H * Wd, O, dtype=h.dtype, device=h.device)
    for a in range(kh):
        for b in range(kw):
            out = out + hp[:, a:a + H, b:b + Wd].reshape(-1, C) @ W[:, :, a, b].t()
    return out.reshape(B, H, Wd, O)


def _gated(t: Tensor) -> Tensor:
    n = t.shape[-1] // 2
    return torch.tanh(t[..., :n]) * torch.sigmoid(t[..., n:])


def forward(sd, x: Tensor, label: Tensor, probe: Optional[dict] = None) -> Tensor:
    """GatedPixelCNN.forward: x [B, 3, 3] int64, label [B] -> logits [B, n_in, 3, 3] float64, on x's device.  ``probe``: a dict that
    receives ``stream``, the largest magnitude the residual stream x_h reaches after any layer."""
    dev = x.device
    g = lambda k: sd[k].to(dev).double()
    xv = xh = g("embedding.weight")[x]                      # [B, H, W, dim]
    stream = 0.0
    for i in range(n_layers(sd)):
        p = f"layers.{i}."
        Wv, Wh = g(p + "vert_stack.weight").clone(), g(p + "horiz_stack.weight").clone()
        if i == 0:                                          # mask A
            Wv[:, :, -1] = 0.0
            Wh[:, :, :, -1] = 0.0
        half = Wv.shape[3] // 2
        cls = g(p + "class_cond_embedding.weight")[label.to(dev)][:, None, None, :]
        # vert_stack: kernel (half + 1, k), padding (half, half), output cropped to the first H rows
        hv = _taps(xv, Wv, half, half) + g(p + "vert_stack.bias")
        # horiz_stack: kernel (1, half + 1), padding (0, half), output cropped to the first W columns
        hh = _taps(xh, Wh, 0, half) + g(p + "horiz_stack.bias")
        W1 = g(p + "vert_to_horiz.weight")
        v2h = hv @ W1.reshape(W1.shape[0], -1).t() + g(p + "vert_to_horiz.bias")
        out = _gated(v2h + hh + cls)
        Wr = g(p + "horiz_resid.weight")
        new = out @ Wr.reshape(Wr.shape[0], -1).t() + g(p + "horiz_resid.bias")
        xv, xh = _gated(hv + cls), (new + xh if i >= 1 else new)
        stream = max(stream, float(xh.abs().max()))
    if probe is not None:
        probe["stream"] = stream
    W0, W2 = g("output_conv.0.weight"), g("output_conv.2.weight")
    hid = torch.relu(xh @ W0.reshape(W0.shape[0], -1).t() + g("output_conv.0.bias"))
    return (hid @ W2.reshape(W2.shape[0], -1).t() + g("output_conv.2.bias")).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ inputs
def codes_and_labels(size, B: int) -> Tuple[Tensor, Tensor]:
    """Random codes [B, 3, 3] and labels [B] of a case."""
    g = torch.Generator().manual_seed(1000 * size[0] + B)
    return torch.randint(0, size[0], (B, 3, 3), generator=g), torch.randint(0, size[3], (B,), generator=g)


def rows_of(size, B: int, limit: int = 40, keep: int = 32) -> Tensor:
    """The rows on which a case is compared: all of them, except at the full size beyond ``limit`` rows, where it is about ``keep``:
    both ends of every 128-row block and rows spread evenly between."""
    if size != FULL or B <= limit:
        return torch.arange(B)
    ends = {r for b0 in range(0, B, 128) for r in (b0, min(b0 + 127, B - 1))}
    spread = {int(r) for r in torch.linspace(1, B - 2, keep - len(ends)).round().tolist()}
    return torch.tensor(sorted(ends | spread))


def race(logits: Tensor, q: Tensor) -> Tensor:
    """The exponential race behind a multinomial draw: argmax(logit - log q) is a draw from softmax(logit) for q ~ Exp(1)."""
    return logits.double() - torch.log(q.double())
