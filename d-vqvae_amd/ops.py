"""Tensor-level wrappers over the C ABI (include/dvq.h).

PyTorch is used for device memory and streams only: every op validates its tensors (device, dtype,
contiguity -> RuntimeError, the reference's error convention), allocates outputs/scratch through the
torch caching allocator and enqueues the HIP work on torch's *current* stream.  No host sync inside.
"""
from __future__ import annotations

import contextlib
import math
import threading
import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check

Tensor = torch.Tensor


def _require_gpu(*ts: Tensor) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("dvq ops need tensors on a HIP device (there is no CPU fallback); got " + str(t.device))
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {t.device} vs {dev}")
    return dev


def _f32(t: Tensor, name: str) -> Tensor:
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    return t


def _i64(t: Tensor, name: str) -> Tensor:
    if t.dtype != torch.int64:
        raise RuntimeError(f"{name}: expected int64, got {t.dtype}")
    return t


def _rows(t: Tensor, name: str) -> Tuple[int, int]:
    """(pointer, row stride) of a 2-D fp32 view whose rows are contiguous."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError(f"{name}: expected a 2-D tensor with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _tensors(what: str, names: str, *xs) -> None:
    """Every ``x`` must be a tensor; ``names`` holds their names, separated by blanks, for the refusal."""
    for i, x in enumerate(xs):
        if not isinstance(x, Tensor):
            raise RuntimeError(f"{what}: {names.split()[i]} must be a tensor")


def _int32_tables(what: str, names: str, *xs: Tensor) -> None:
    for i, x in enumerate(xs):
        if x.dtype != torch.int32 or not x.is_contiguous():
            raise RuntimeError(f"{what}: {names.split()[i]} must be contiguous int32")


def _positive(what: str, name: str, x) -> float:
    x = float(x)
    if not 0.0 < x < math.inf:
        raise RuntimeError(f"{what}: {name} must be finite and positive (got {x})")
    return x


def _non_negative(what: str, name: str, x) -> float:
    x = float(x)
    if not 0.0 <= x < math.inf:
        raise RuntimeError(f"{what}: {name} must be finite and >= 0 (got {x})")
    return x


def _obj_of_row(what: str, x: Tensor, B: int) -> None:
    if _i64(x, "obj_of_row").shape != (B,) or not x.is_contiguous():
        raise RuntimeError(f"{what}: `obj_of_row` must be a contiguous int64 [B] tensor")


_F, _I, _L = torch.float32, torch.int32, torch.int64


def _outputs(rows: int, dev: torch.device, *spec):
    """One uninitialised [rows, *trailing] tensor per ``(dtype, *trailing)`` of ``spec``; ``None`` (an optional output that was not
    asked for) stays ``None``, which ``_ptr`` hands to the library as a null pointer."""
    return tuple(None if s is None else torch.empty(rows, *s[1:], dtype=s[0], device=dev) for s in spec)


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


_ws: Dict[Tuple[int, int, str], Tensor] = {}
_WS_MAX = 16        # (device, stream) scratch buffers kept; the least recently used one goes when a 17th stream shows up


def workspace(nbytes: int, dev: torch.device, tag: str = "main") -> Tensor:
    """Grow-only scratch per (device, current stream): reuse is ordered by the stream the ops are enqueued on, so two
    streams driving the library concurrently never share a buffer.  At most ``_WS_MAX`` buffers are kept (LRU; an evicted
    buffer stays alive until the work already enqueued on it has run: the caching allocator frees by stream order)."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, int(torch.cuda.current_stream(idx).cuda_stream), tag)
    buf = _ws.pop(key, None)
    if buf is None or buf.numel() < nbytes:
        buf = None
        buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
    _ws[key] = buf                                           # (re)inserted last = most recently used
    while len(_ws) > _WS_MAX:
        _ws.pop(next(iter(_ws)))
    return buf


def release_workspaces() -> None:
    _ws.clear()


def new_err_flag(dev: torch.device) -> Tensor:
    return torch.zeros(1, dtype=torch.int32, device=dev)


@contextlib.contextmanager
def _err_flag(err: Optional[Tensor], dev: torch.device, message):
    """``with _err_flag(err, dev, message) as flag:`` around a launch that reports through an int32 flag.  ``flag`` is the caller's
    ``err`` -- then the caller reads it and nothing synchronises here -- or a fresh one, read once after the block: a non-zero value
    raises ``RuntimeError(message)``; a wrapper whose bits mean different things passes a function of the value for ``message``."""
    flag = new_err_flag(dev) if err is None else err
    yield flag
    if err is None:
        bad = int(flag.item())
        if bad:
            raise RuntimeError(message(bad) if callable(message) else message)


# ------------------------------------------------------------------------------------------ fp16 range
# The default GEMM arithmetic carries activations as two fp16 pieces: a value beyond fp16's range (|x| >= 65 520) turns its output
# ROW into NaN -- never a silently wrong number (csrc/gemm_f16x2.hip).  Every entry point that multiplies on those images looks at
# its result once (one host synchronisation) and runs the call again on the six-product bf16 images, which have fp32's range, when
# it holds a non-finite value; inputs that are themselves NaN / Inf come out non-finite there too, as in the reference.
# GenNet.gen makes ONE such check for the whole path and switches the per-op checks off around its inner calls.
_range_state = threading.local()                            # per host thread: one thread's gen() must not switch another's checks off


class no_range_check(contextlib.ContextDecorator):
    """``with ops.no_range_check(): ...`` (or ``@ops.no_range_check()`` on a function) -- the caller checks the final result itself
    (GenNet.gen: one synchronisation per call)."""

    def __enter__(self):
        _range_state.off = getattr(_range_state, "off", 0) + 1
        return self

    def __exit__(self, *exc):
        _range_state.off -= 1
        return False


def _out_of_range(kind, *outs: Tensor) -> bool:
    """True when a result of the fp16-image arithmetic holds a non-finite value and the per-op check is on (synchronises)."""
    if getattr(_range_state, "off", 0) or kind != _lib.PLANES_F16X2:
        return False
    return not all(bool(torch.isfinite(o).all()) for o in outs if o is not None)


# ------------------------------------------------------------------------------------------ dense
def _planes_args(pl, w: Tensor, what: str):
    """(kind, planes pointer, plane stride, scale pointer, scale tensor) of a weight image handed to an op: a packing.Planes
    or, as before, the bare int16 [3,N,K] tensor of packing.split_bf16x3."""
    from . import packing
    if isinstance(pl, Tensor):
        pl = packing.Planes(_lib.PLANES_BF16X3, pl)
    n_pl = 2 if pl.kind == _lib.PLANES_F16X2 else 3
    t = pl.planes
    if t.dtype != torch.int16 or tuple(t.shape) != (n_pl,) + tuple(w.shape) or not t.is_contiguous() or not w.is_contiguous():
        raise RuntimeError(f"{what}: planes must be the contiguous int16 [{n_pl},N,K] image of a contiguous weight")
    if pl.kind == _lib.PLANES_F16X2 and (pl.scale is None or pl.scale.numel() != w.shape[0] or pl.scale.dtype != torch.float32):
        raise RuntimeError(f"{what}: fp16 planes need their [N] row scales")
    return pl.kind, t.data_ptr(), w.numel(), (pl.scale.data_ptr() if pl.scale is not None else None), pl.scale


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, relu: bool = False,
           out: Optional[Tensor] = None, planes=None) -> Tensor:
    """y = act(x @ weight^T + bias) (dvq_linear).  ``planes`` = packing.split_planes(weight): the pre-split weight image;
    without it the image is built on the spot (two small launches), so both forms give the same bits."""
    return linear_multi([(x, weight)], bias, relu, out, planes=[planes] if planes is not None else None)


def linear_multi(pairs: Sequence[Tuple[Tensor, Tensor]], bias: Optional[Tensor] = None, relu: bool = False,
                 out: Optional[Tensor] = None, planes: Optional[Sequence] = None) -> Tensor:
    """y = act(sum_s x_s @ w_s^T + bias).  fp16 images of one call must come from ONE packing.split_f16x2 group (shared row
    scales); ``planes=None`` builds that group here when the default (fp16) arithmetic is selected."""
    from . import packing
    lib = _lib.load()
    dev = _require_gpu(*[t for p in pairs for t in p], bias, out)
    M = pairs[0][0].shape[0]
    N = pairs[0][1].shape[0]
    if planes is None and packing.gemm_kind() == _lib.PLANES_F16X2 and all(w.is_contiguous() and w.dtype == torch.float32 for _, w in pairs):
        planes = packing.split_f16x2([w for _, w in pairs])
    srcs = (_lib.GemmSrc * len(pairs))()
    scale0 = None
    for i, (x, w) in enumerate(pairs):
        _f32(x, "x"), _f32(w, "weight")
        if x.shape[0] != M or w.shape[0] != N or x.shape[1] != w.shape[1]:
            raise RuntimeError(f"linear: shape mismatch x{tuple(x.shape)} w{tuple(w.shape)}")
        px, ldx = _rows(x, "x")
        pw, ldw = _rows(w, "weight")
        kind, wp, wps, sp = 0, None, 0, None
        if planes is not None:
            kind, wp, wps, sp, st = _planes_args(planes[i], w, "linear")
            if i == 0:
                scale0 = st
            elif kind == _lib.PLANES_F16X2 and st is not scale0:
                raise RuntimeError("linear_multi: the fp16 images of one call must share their row scales (packing.split_f16x2 of the group)")
        srcs[i] = _lib.GemmSrc(px, pw, ldx, ldw, x.shape[1], kind, wp, wps, sp)
    if bias is not None:
        _f32(bias, "bias")
        if bias.numel() != N or not bias.is_contiguous():
            raise RuntimeError("linear: bias must be a contiguous [N] tensor")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=dev)
    po, ldo = _rows(_f32(out, "out"), "out")
    if out.shape[0] != M or out.shape[1] != N:
        raise RuntimeError("linear: bad output shape")
    with torch.cuda.device(dev):
        check(lib.dvq_linear(srcs, len(pairs), M, N, bias.data_ptr() if bias is not None else None,
                             1 if relu else 0, po, ldo, _stream(dev)), "dvq_linear")
    if planes is not None and _out_of_range(srcs[0].wp_kind, out):
        with no_range_check():                               # once more on the six-product images (fp32's range)
            return linear_multi(pairs, bias, relu, out, planes=[packing.split_planes(w.contiguous(), _lib.PLANES_BF16X3) for _, w in pairs])
    return out


def mlp3(x: Tensor, layers, out: Optional[Tensor] = None) -> Tensor:
    """Linear + ReLU, Linear + ReLU, Linear (dvq_mlp3: Decoder / Encoder of network/DVQVAE.py).
    ``layers`` = three (weight [n_out, k_in], bias or None, planes (packing.split_planes) or None) tuples."""
    lib = _lib.load()
    dev = _require_gpu(x, out, *[t for l in layers for t in l[:2]])
    if len(layers) != 3:
        raise RuntimeError("mlp3: exactly three layers")
    px, ldx = _rows(_f32(x, "x"), "x")
    M = x.shape[0]
    arr = (_lib.MlpLayer * 3)()
    k = x.shape[1]
    for i, (w, b, pl) in enumerate(layers):
        _f32(w, "weight")
        if not w.is_contiguous() or w.shape[1] != k or (b is not None and (b.numel() != w.shape[0] or not b.is_contiguous())):
            raise RuntimeError(f"mlp3: layer {i} has weight {tuple(w.shape)} for {k} inputs")
        kind, wp, sp = 0, None, None
        if pl is not None:
            kind, wp, _, sp, _ = _planes_args(pl, w, "mlp3")
        arr[i] = _lib.MlpLayer(w.data_ptr(), b.data_ptr() if b is not None else None, wp, w.shape[0], w.shape[1], sp, kind, 0)
        k = w.shape[0]
    if out is None:
        out = torch.empty(M, k, dtype=torch.float32, device=dev)
    po, ldo = _rows(_f32(out, "out"), "out")
    if tuple(out.shape) != (M, k):
        raise RuntimeError("mlp3: bad output shape")
    nws = lib.dvq_mlp3_workspace_bytes(M, layers[0][0].shape[0], layers[1][0].shape[0])
    ws = workspace(nws, dev, tag="mlp3")
    with torch.cuda.device(dev):
        check(lib.dvq_mlp3(px, ldx, M, arr, po, ldo, ws.data_ptr(), ws.numel(), _stream(dev)), "dvq_mlp3")
    if any(l[2] is not None and not isinstance(l[2], Tensor) and l[2].kind == _lib.PLANES_F16X2 for l in layers) and _out_of_range(_lib.PLANES_F16X2, out):
        from . import packing
        with no_range_check():                               # once more on the six-product images (fp32's range)
            return mlp3(x, [(w, b, packing.split_planes(w, _lib.PLANES_BF16X3)) for w, b, _ in layers], out=out)
    return out


# ------------------------------------------------------------------------------------------ VQ
def vq_fast_supported(K: int, D: int) -> bool:
    return bool(_lib.load().dvq_vq_fast_supported(K, D))


def vq_pack(E: Tensor) -> Tensor:
    """Packed image of a codebook for the fast path (fp16 image of -2 sE E, canonical |e_k|^2, max |e_k|, measured rounding error).
    Build it once per codebook state and pass it to ``vq_argmin(..., packed=)``; it is NOT cached here because a
    raw pointer cannot tell a recycled allocation from the same codebook."""
    lib = _lib.load()
    _require_gpu(E)
    K, D = E.shape
    nbytes = lib.dvq_vq_pack_bytes(K, D)
    if nbytes == 0:
        raise RuntimeError(f"vq_pack: no fast path for K={K}, D={D}")
    if not E.is_contiguous():
        raise RuntimeError("vq_pack: codebook must be contiguous")
    packed = torch.empty(nbytes, dtype=torch.uint8, device=E.device)
    with torch.cuda.device(E.device):
        check(lib.dvq_vq_pack(_f32(E, "E").data_ptr(), K, D, packed.data_ptr(), nbytes, _stream(E.device)), "dvq_vq_pack")
    return packed


def vq_argmin(z: Tensor, E: Tensor, return_dist: bool = False, fast: Optional[bool] = None,
              packed: Optional[Tensor] = None, slow_rows: Optional[Tensor] = None):
    """idx[m] = argmin_k (|z_m|^2 + |E_k|^2) - 2 z_m.E_k in the canonical fp32 order -> int64 [M].
    K<=512 (a multiple of 32)/D=256 on dense rows takes the fast kernel (fp16-MFMA filter + exact refine in one launch; same indices, bit for bit); everything else
    (and ``return_dist``) the exact fp32-MFMA kernel.  ``fast`` forces the choice; ``packed`` = vq_pack(E) skips the
    per-call codebook packing (three tiny kernels); ``slow_rows`` (int64 [1] on the device, accumulated, never reset)
    counts the rows the fast kernel could not decide from their candidate lists (see dvq.h)."""
    lib = _lib.load()
    dev = _require_gpu(z, E)
    _f32(z, "z"), _f32(E, "E")
    if not E.is_contiguous():
        raise RuntimeError("vq_argmin: codebook must be contiguous")
    pz, ldz = _rows(z, "z")
    M, D = z.shape
    K = E.shape[0]
    if E.shape[1] != D:
        raise RuntimeError(f"vq_argmin: z has D={D}, codebook has D={E.shape[1]}")
    idx = torch.empty(M, dtype=torch.int64, device=dev)
    can_fast = bool(lib.dvq_vq_fast_supported(K, D)) and not return_dist and (M <= 1 or ldz == D) and pz % 16 == 0
    if fast is None:
        fast = can_fast
    elif fast and not can_fast:
        raise RuntimeError(f"vq_argmin: fast path unavailable for K={K}, D={D}, dense={ldz == D}, return_dist={return_dist}")
    if fast and M > 0:
        if packed is None:
            packed = vq_pack(E)
        nws = lib.dvq_vq_fast_workspace_bytes(M, K, D)
        ws = workspace(nws, dev)
        with torch.cuda.device(dev):
            check(lib.dvq_vq_argmin_fast(pz, E.data_ptr(), packed.data_ptr(), M, K, D, idx.data_ptr(),
                                         _i64(slow_rows, "slow_rows").data_ptr() if slow_rows is not None else None,
                                         ws.data_ptr(), ws.numel(), _stream(dev)), "dvq_vq_argmin_fast")
        return idx
    dmin = torch.empty(M, dtype=torch.float32, device=dev) if return_dist else None
    nws = lib.dvq_vq_argmin_workspace_bytes(M, K)
    ws = workspace(nws, dev)
    with torch.cuda.device(dev):
        check(lib.dvq_vq_argmin(pz, ldz, E.data_ptr(), M, K, D, idx.data_ptr(), dmin.data_ptr() if return_dist else None,
                                ws.data_ptr(), ws.numel(), _stream(dev)), "dvq_vq_argmin")
    return (idx, dmin) if return_dist else idx


def vq_lookup(E: Tensor, idx: Tensor, out: Optional[Tensor] = None, err: Optional[Tensor] = None) -> Tensor:
    """out[m] = E[idx[m]] (row gather == one-hot @ E).  ``idx`` may be a strided 1-D view.
    Out-of-range indices raise RuntimeError unless an ``err`` flag tensor is supplied (then the caller checks it)."""
    lib = _lib.load()
    dev = _require_gpu(E, idx, out, err)
    _f32(E, "E"), _i64(idx, "idx")
    if idx.dim() != 1 or not E.is_contiguous():
        raise RuntimeError("vq_lookup: idx must be 1-D and the codebook contiguous")
    M, (K, D) = idx.shape[0], E.shape
    if out is None:
        out = torch.empty(M, D, dtype=torch.float32, device=dev)
    po, ldo = _rows(_f32(out, "out"), "out")
    with _err_flag(err, dev, f"index out of bounds for codebook with {K} rows") as flag, torch.cuda.device(dev):
        check(lib.dvq_vq_lookup(E.data_ptr(), idx.data_ptr(), idx.stride(0) if M > 1 else 1, M, K, D, po, ldo,
                                flag.data_ptr(), _stream(dev)), "dvq_vq_lookup")
    return out


# ------------------------------------------------------------------------------------------ sampling noise
def exp1_noise(rows: int, cols: int, seed: int, row0: int = 0, stream_id: int = 0, device=None, out: Optional[Tensor] = None,
               perm: Optional[Tensor] = None) -> Tensor:
    """[rows, cols] Exp(1) variates from the device Philox generator, keyed by (seed, stream_id, GLOBAL row row0 + r, column):
    a shard of a batch (row0 = its first row) draws exactly the rows the whole batch would draw (dvq_exp1_noise).
    ``perm`` (int64 [rows] on the device): row r of the result holds the draws of global row row0 + perm[r]."""
    lib = _lib.load()
    if cols % 4 != 0:                                     # the generator writes 16-byte quads: draw a padded row, keep the columns asked for
        if device is None and out is not None:
            device = out.device
        wide = exp1_noise(rows, (cols + 3) // 4 * 4, seed, row0, stream_id, device=device, perm=perm)
        if out is None:
            return wide[:, :cols].contiguous()
        out.copy_(wide[:, :cols])
        return out
    if out is None:
        if device is None:
            raise RuntimeError("exp1_noise: pass `device` or `out`")
        out = torch.empty(rows, cols, dtype=torch.float32, device=device)
    dev = _require_gpu(out)
    if tuple(out.shape) != (rows, cols) or not out.is_contiguous() or out.dtype != torch.float32:
        raise RuntimeError("exp1_noise: `out` must be a contiguous float32 [rows, cols] tensor")
    if perm is not None and (perm.dtype != torch.int64 or perm.numel() != rows or not perm.is_contiguous() or perm.device != out.device):
        raise RuntimeError("exp1_noise: `perm` must be a contiguous int64 [rows] tensor on the output's device")
    with torch.cuda.device(dev):
        check(lib.dvq_exp1_noise_rows(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF, int(row0),
                                      perm.data_ptr() if perm is not None else None, rows, cols, out.data_ptr(), _stream(dev)), "dvq_exp1_noise")
    return out


def exp1_noise_keyed(stream_ids: Tensor, row_ids: Tensor, cols: int, seed: int, out: Optional[Tensor] = None,
                     err: Optional[Tensor] = None) -> Tensor:
    """[rows, cols] Exp(1) variates with one key per row: row r holds exactly the draws of
    ``exp1_noise(1, cols, seed, row0=row_ids[r], stream_id=stream_ids[r])`` (dvq_exp1_noise_keyed), so a call that mixes the
    grasps of many objects draws what the per-object calls draw.  ``stream_ids`` / ``row_ids``: contiguous int64 [rows] on the
    device.  A stream id outside [0, 2^32) or a negative row id raises RuntimeError unless an ``err`` flag tensor is supplied
    (then the caller checks it; the row is NaN)."""
    lib = _lib.load()
    dev = _require_gpu(stream_ids, row_ids, out, err)
    _i64(stream_ids, "stream_ids"), _i64(row_ids, "row_ids")
    if stream_ids.dim() != 1 or row_ids.shape != stream_ids.shape or not stream_ids.is_contiguous() or not row_ids.is_contiguous():
        raise RuntimeError("exp1_noise_keyed: `stream_ids` and `row_ids` must be contiguous int64 [rows] tensors of one length")
    rows = stream_ids.shape[0]
    if cols % 4 != 0:                                     # the generator writes 16-byte quads: draw a padded row, keep the columns asked for
        wide = exp1_noise_keyed(stream_ids, row_ids, (cols + 3) // 4 * 4, seed, err=err)
        if out is None:
            return wide[:, :cols].contiguous()
        out.copy_(wide[:, :cols])
        return out
    if out is None:
        out = torch.empty(rows, cols, dtype=torch.float32, device=dev)
    if tuple(out.shape) != (rows, cols) or not out.is_contiguous() or out.dtype != torch.float32:
        raise RuntimeError("exp1_noise_keyed: `out` must be a contiguous float32 [rows, cols] tensor")
    with _err_flag(err, dev, "exp1_noise_keyed: stream id outside [0, 2^32) or negative row id") as flag, torch.cuda.device(dev):
        check(lib.dvq_exp1_noise_keyed(int(seed) & 0xFFFFFFFFFFFFFFFF, stream_ids.data_ptr(), row_ids.data_ptr(), rows, cols,
                                       out.data_ptr(), flag.data_ptr(), _stream(dev)), "dvq_exp1_noise_keyed")
    return out


def default_noise_key():
    """(seed, first global row) of noise drawn without an explicit key: the seed follows torch.manual_seed (initial_seed of
    the default generator), and every rank of a process group draws rows of its own (rank * 2^40 + b), so that ranks calling
    gen(obj) on different objects without naming seed / row0 do not all draw the same noise."""
    import torch.distributed as td
    rank = td.get_rank() if td.is_available() and td.is_initialized() else 0
    return int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF, rank << 40


def probe_f16_subnormal(device) -> Tuple[float, float]:
    """(fp16 MFMA product with a subnormal input, its exact value): equal when the matrix core keeps fp16 subnormals."""
    lib = _lib.load()
    out = torch.zeros(2, dtype=torch.float32, device=device)
    dev = _require_gpu(out)
    with torch.cuda.device(dev):
        check(lib.dvq_probe_f16_subnormal(out.data_ptr(), _stream(dev)), "dvq_probe_f16_subnormal")
    a, b = out.cpu().tolist()
    return a, b


# ------------------------------------------------------------------------------------------ PointNet
def pointnet_encode(packed, pc: Tensor, out: Optional[Tensor] = None, want_trans: bool = True):
    """packed: packing.PackedPointNet.  pc [B,C,N] -> (feat [B,1024] (or written into ``out``), trans [B,3,3])."""
    lib = _lib.load()
    dev = _require_gpu(pc, out)
    _f32(pc, "pc")
    if pc.dim() != 3 or not pc.is_contiguous() or pc.shape[1] != packed.C:
        raise RuntimeError(f"pointnet_encode: expected a contiguous [B,{packed.C},N] tensor, got {tuple(pc.shape)}")
    packed.to(dev)
    B, _, N = pc.shape
    if out is None:
        out = torch.empty(B, 1024, dtype=torch.float32, device=dev)
    po, ldo = _rows(_f32(out, "out"), "out")
    if out.shape != (B, 1024):
        raise RuntimeError("pointnet_encode: bad output shape")
    trans = torch.empty(B, 3, 3, dtype=torch.float32, device=dev) if want_trans else None
    nws = lib.dvq_pointnet_workspace_bytes(B, N)
    ws = workspace(nws, dev)
    with torch.cuda.device(dev):
        check(lib.dvq_pointnet_encode(C.byref(packed.cstruct), pc.data_ptr(), B, N, po, ldo,
                                      trans.data_ptr() if want_trans else None, ws.data_ptr(), ws.numel(), _stream(dev)),
              "dvq_pointnet_encode")
    return out, trans


def pointnet_fault_counters(reset: bool = False) -> Tuple[int, int]:
    """(suspect tile records, channels outside their records' interval) the filtered PointNet trunk has counted on the current device
    since the last reset -- its run-time consistency checks (dvq_pointnet_fault_counters).  Both are re-evaluated in full when they
    happen, so the features stay right; anything but (0, 0) means the filter's bookkeeping failed and should be reported."""
    lib = _lib.load()
    out = (C.c_uint64 * 2)()
    check(lib.dvq_pointnet_fault_counters(out, 1 if reset else 0), "dvq_pointnet_fault_counters")
    return int(out[0]), int(out[1])


# ------------------------------------------------------------------------------------------ PixelCNN
def pixelcnn_sample(packed, label: Tensor, noise: Optional[Tensor], return_logits: bool = False, err: Optional[Tensor] = None,
                    _retry: bool = False, temperature: float = 1.0, top_k: int = 0, given: Optional[Tensor] = None,
                    return_logp: bool = False):
    """label [B] int64, noise [B,9,n_in] Exp(1) -> codes [B,3,3] int64 (+ logits [B,9,n_in]) (+ logp_model, logp_draw [B,9]).
    With a caller-supplied ``err`` flag nothing synchronises here: a draw from all-NaN logits (fp16 range, bit 2 of the flag) leaves
    -1 at its position of ``codes`` and the caller deals with those rows (GenNet.gen regenerates them on the bf16x3 images).
    Controls on the draw (include/dvq.h: dvq_pixelcnn_sample_ctl): ``temperature`` T > 0 divides the logits, ``top_k`` > 0 keeps
    the top_k largest (ties towards the lowest index), ``given`` int64 [B,9] / [B,3,3] fixes the positions whose entry is >= 0
    and draws the negative ones (``noise`` may be None when nothing is drawn), ``return_logp`` appends the log-probability of
    every position's code under the untempered prior (logp_model) and under the distribution drawn from (logp_draw).  With all
    four at their defaults this is the call to dvq_pixelcnn_sample it always was."""
    _i64(label, "label")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or not temperature > 0:
        raise RuntimeError(f"pixelcnn_sample: temperature must be a finite number > 0, got {temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise RuntimeError(f"pixelcnn_sample: top_k must be an integer >= 0 (0: off), got {top_k!r}")
    B = label.shape[0]
    if label.dim() != 1 or not label.is_contiguous():
        raise RuntimeError("pixelcnn_sample: label must be a contiguous [B] tensor")
    if given is not None:
        if (not torch.is_tensor(given) or given.dtype != torch.int64 or tuple(given.shape) not in ((B, 9), (B, 3, 3))
                or not given.is_contiguous() or given.device != label.device):
            raise RuntimeError("pixelcnn_sample: given must be a contiguous int64 [B,9] or [B,3,3] tensor on label's device")
    controlled = float(temperature) != 1.0 or top_k != 0 or given is not None or return_logp
    if noise is None:
        if given is None:
            raise RuntimeError("pixelcnn_sample: noise may be omitted only when given codes are passed")
    else:
        _f32(noise, "noise")
    lib = _lib.load()
    dev = _require_gpu(label, noise, given, err)
    if noise is not None and (tuple(noise.shape) != (B, 9, packed.n_in) or not noise.is_contiguous()):
        raise RuntimeError(f"pixelcnn_sample: noise must be contiguous [B,9,{packed.n_in}], got {tuple(noise.shape)}")
    packed.to(dev)
    codes = torch.empty(B, 3, 3, dtype=torch.int64, device=dev)
    logits = torch.empty(B, 9, packed.n_in, dtype=torch.float32, device=dev) if return_logits else None
    logp = torch.empty(2, B, 9, dtype=torch.float32, device=dev) if return_logp else None
    own_err = err is None
    if own_err:
        err = new_err_flag(dev)
    nws = lib.dvq_pixelcnn_workspace_bytes(C.byref(packed.cstruct), B)
    ws = workspace(nws, dev)
    with torch.cuda.device(dev):
        if not controlled:
            check(lib.dvq_pixelcnn_sample(C.byref(packed.cstruct), label.data_ptr(), noise.data_ptr(), B, codes.data_ptr(),
                                          logits.data_ptr() if return_logits else None, err.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _stream(dev)), "dvq_pixelcnn_sample")
        else:
            ctl = _lib.PixelcnnCtl(float(temperature), int(min(top_k, 2 ** 31 - 1)), given.data_ptr() if given is not None else None,
                                   logp[0].data_ptr() if return_logp else None, logp[1].data_ptr() if return_logp else None)
            check(lib.dvq_pixelcnn_sample_ctl(C.byref(packed.cstruct), label.data_ptr(), noise.data_ptr() if noise is not None else None,
                                              B, C.byref(ctl), codes.data_ptr(), logits.data_ptr() if return_logits else None,
                                              err.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "dvq_pixelcnn_sample_ctl")
    if own_err:
        e = int(err.item())
        if e & 1:
            raise RuntimeError(f"label or given code out of range for the prior's {packed.n_classes} classes / {packed.n_in} tokens"
                               if controlled else f"label out of range for the prior's {packed.n_classes} classes")
        # a given code is never -1 and raises no bit 2: NaN logits at its position show in what the call returns for it alone
        nan_given = given is not None and not _retry and _out_of_range(packed.kind, logp[0] if return_logp else None, logits)
        if ((e & 4) or nan_given) and packed.kind == _lib.PLANES_F16X2 and not _retry:
            # non-finite logits under the fp16 weight images: an activation left fp16's range (or the input is not finite): once
            # more on the six-product bf16 split, which has fp32's range; the images return to the default kind at the next use
            from . import packing
            with packing.gemm_kind_as(_lib.PLANES_BF16X3):
                return pixelcnn_sample(packed, label, noise, return_logits=return_logits, _retry=True, temperature=temperature,
                                       top_k=top_k, given=given, return_logp=return_logp)
    out = (codes,) + ((logits,) if return_logits else ()) + ((logp[0], logp[1]) if return_logp else ())
    return out if len(out) > 1 else codes


PIXELCNN_BEAM_MAX_W = 1024          # csrc/pixelcnn.hip: BEAM_MAX_W (a segment's survivors are ordered in LDS)


def pixelcnn_beam(packed, label: Tensor, width: int, trace: bool = False, err: Optional[Tensor] = None):
    """Beam search over the prior (include/dvq.h: dvq_pixelcnn_beam): label [S] int64 -> (codes [S,W,3,3] int64, score [S,W] f32,
    n_live [S] int32), the ``width`` likeliest distinct code grids of every label in rank order; rows beyond n_live hold -1 / -inf.
    ``trace=True`` appends a dict of the per-position selections: parent, token [9,S,W] int32, score [9,S,W] f32, live [9,S] int32,
    logits [9,S,W,n_in] f32.  No noise, no temperature: the result is a function of the weights and the labels.
    fp16 weight images only: the search has no bf16 fallback.  With a caller-supplied ``err`` flag nothing synchronises here;
    otherwise a label out of range and a segment whose logits held a NaN (n_live = 0) raise."""
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= PIXELCNN_BEAM_MAX_W:
        raise RuntimeError(f"pixelcnn_beam: width must be an integer in 1 .. {PIXELCNN_BEAM_MAX_W}, got {width!r}")
    if not torch.is_tensor(label):
        raise RuntimeError("pixelcnn_beam: label must be a tensor")
    _i64(label, "label")
    if label.dim() != 1 or not label.is_contiguous():
        raise RuntimeError("pixelcnn_beam: label must be a contiguous [S] tensor")
    dev = _require_gpu(label, err)
    from . import packing
    if packing.gemm_kind() != _lib.PLANES_F16X2:
        raise RuntimeError("pixelcnn_beam: the search runs on the fp16 weight images only (it follows a beam's ancestry through the "
                           "row index of the fp16-plane GEMMs); there is no bf16 beam")
    lib = _lib.load()
    packed.to(dev)
    S, W, n_in = label.shape[0], width, packed.n_in
    codes = torch.empty(S, W, 3, 3, dtype=torch.int64, device=dev)
    score = torch.empty(S, W, dtype=torch.float32, device=dev)
    n_live = torch.empty(S, dtype=torch.int32, device=dev)
    tr, ctr = None, None
    if trace:
        tr = dict(parent=torch.empty(9, S, W, dtype=torch.int32, device=dev), token=torch.empty(9, S, W, dtype=torch.int32, device=dev),
                  score=torch.empty(9, S, W, dtype=torch.float32, device=dev), live=torch.empty(9, S, dtype=torch.int32, device=dev),
                  logits=torch.empty(9, S, W, n_in, dtype=torch.float32, device=dev))
        ctr = _lib.PixelcnnBeamTrace(*(tr[k].data_ptr() for k in ("parent", "token", "score", "live", "logits")))
    own_err = err is None
    if own_err:
        err = new_err_flag(dev)
    if S > 0:
        nws = lib.dvq_pixelcnn_beam_workspace_bytes(C.byref(packed.cstruct), S, W)
        ws = workspace(nws, dev)
        with torch.cuda.device(dev):
            check(lib.dvq_pixelcnn_beam(C.byref(packed.cstruct), label.data_ptr(), S, W, codes.data_ptr(), score.data_ptr(),
                                        n_live.data_ptr(), C.byref(ctr) if ctr is not None else None, err.data_ptr(), ws.data_ptr(),
                                        ws.numel(), _stream(dev)), "dvq_pixelcnn_beam")
    if own_err:
        e = int(err.item())
        if e & 1:
            raise RuntimeError(f"label out of range for the prior's {packed.n_classes} classes")
        if e & 4:
            bad = (n_live == 0).nonzero().reshape(-1).tolist()
            raise RuntimeError(f"pixelcnn_beam: NaN logits in the search of segments {bad} (an activation beyond fp16's range); "
                               "there is no bf16 beam")
    return (codes, score, n_live) + ((tr,) if trace else ())


def pixelcnn_forward(packed, x: Tensor, label: Tensor) -> Tensor:
    """x [B,3,3] int64 tokens, label [B] -> logits [B,n_in,3,3] (GatedPixelCNN.forward)."""
    lib = _lib.load()
    dev = _require_gpu(x, label)
    _i64(x, "x"), _i64(label, "label")
    packed.to(dev)
    B = x.shape[0]
    if tuple(x.shape[1:]) != (3, 3):
        raise RuntimeError("pixelcnn_forward: only the 3x3 latent grid of the grasp path is supported")
    x = x.contiguous()
    label = label.contiguous()
    logits = torch.empty(B, 9, packed.n_in, dtype=torch.float32, device=dev)
    err = new_err_flag(dev)
    nws = lib.dvq_pixelcnn_workspace_bytes(C.byref(packed.cstruct), B)
    ws = workspace(nws, dev)
    with torch.cuda.device(dev):
        check(lib.dvq_pixelcnn_forward(C.byref(packed.cstruct), x.data_ptr(), label.data_ptr(), B, logits.data_ptr(),
                                       err.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "dvq_pixelcnn_forward")
    if int(err.item()) & 1:
        raise RuntimeError("index out of range in self (token or class label)")
    if _out_of_range(packed.kind, logits):
        from . import packing
        with no_range_check(), packing.gemm_kind_as(_lib.PLANES_BF16X3):     # once more on the six-product images (fp32's range)
            return pixelcnn_forward(packed, x, label)
    return logits.view(B, 3, 3, packed.n_in).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------ MANO
def mano_forward(packed, betas: Tensor, hand_pose: Tensor, global_orient: Optional[Tensor] = None,
                 transl: Optional[Tensor] = None, channel_major: bool = False, want_joints: bool = False):
    """-> verts [B,778,3] (or [B,3,778] when channel_major), optional joints [B,16,3]."""
    lib = _lib.load()
    dev = _require_gpu(betas, hand_pose, global_orient, transl)
    packed.to(dev)
    B = betas.shape[0]
    pb, ldb = _rows(_f32(betas, "betas"), "betas")
    pp, ldp = _rows(_f32(hand_pose, "hand_pose"), "hand_pose")
    if betas.shape[1] != 10 or hand_pose.shape[1] != 45 or hand_pose.shape[0] != B:
        raise RuntimeError("mano_forward: expected betas [B,10] and hand_pose [B,45]")
    for name, t in (("global_orient", global_orient), ("transl", transl)):
        if t is not None and tuple(t.shape) != (B, 3):
            raise RuntimeError(f"mano_forward: expected {name} [B,3], got {tuple(t.shape)}")
    pg = ldg = pt = ldt = 0
    if global_orient is not None:
        pg, ldg = _rows(_f32(global_orient, "global_orient"), "global_orient")
    if transl is not None:
        pt, ldt = _rows(_f32(transl, "transl"), "transl")
    verts = torch.empty((B, 3, 778) if channel_major else (B, 778, 3), dtype=torch.float32, device=dev)
    joints = torch.empty(B, 16, 3, dtype=torch.float32, device=dev) if want_joints else None
    if B == 0:                                              # empty tensors have null data pointers, which the ABI refuses
        return (verts, joints) if want_joints else verts
    nws = lib.dvq_mano_workspace_bytes(B)
    ws = workspace(nws, dev)
    with torch.cuda.device(dev):
        check(lib.dvq_mano_forward(C.byref(packed.cstruct), pb, ldb, pp, ldp, pg or None, ldg, pt or None, ldt, B,
                                   verts.data_ptr(), 1 if channel_major else 0,
                                   joints.data_ptr() if want_joints else None, ws.data_ptr(), ws.numel(), _stream(dev)),
              "dvq_mano_forward")
    if _out_of_range(getattr(packed, "kind", None), verts, joints):
        from . import packing
        with no_range_check(), packing.gemm_kind_as(_lib.PLANES_BF16X3):     # the blendshape GEMM once more on the six-product images
            return mano_forward(packed, betas, hand_pose, global_orient, transl, channel_major, want_joints)
    return (verts, joints) if want_joints else verts


def mano_backward(packed, betas: Tensor, hand_pose: Tensor, global_orient: Optional[Tensor] = None,
                  transl: Optional[Tensor] = None, grad_verts: Optional[Tensor] = None, grad_joints: Optional[Tensor] = None,
                  channel_major: bool = False, needs: Sequence[bool] = (True, True, True, True)):
    """Vector-Jacobian product of ``mano_forward`` (dvq_mano_backward): the forward call's inputs, ``grad_verts`` [B,778,3] (or
    [B,3,778] when channel_major) and / or ``grad_joints`` [B,16,3] -> (grad_betas [B,10], grad_hand_pose [B,45], grad_global_orient
    [B,3], grad_transl [B,3]); an entry of ``needs`` that is false gives ``None`` in its place.  The forward state is recomputed."""
    lib = _lib.load()
    dev = _require_gpu(betas, hand_pose, global_orient, transl, grad_verts, grad_joints)
    packed.to(dev)
    B = betas.shape[0]
    pb, ldb = _rows(_f32(betas, "betas"), "betas")
    pp, ldp = _rows(_f32(hand_pose, "hand_pose"), "hand_pose")
    if betas.shape[1] != 10 or hand_pose.shape[1] != 45 or hand_pose.shape[0] != B:
        raise RuntimeError("mano_backward: expected betas [B,10] and hand_pose [B,45]")
    for name, t in (("global_orient", global_orient), ("transl", transl)):
        if t is not None and tuple(t.shape) != (B, 3):
            raise RuntimeError(f"mano_backward: expected {name} [B,3], got {tuple(t.shape)}")
    pg = ldg = pt = ldt = 0
    if global_orient is not None:
        pg, ldg = _rows(_f32(global_orient, "global_orient"), "global_orient")
    if transl is not None:
        pt, ldt = _rows(_f32(transl, "transl"), "transl")
    if grad_verts is None and grad_joints is None:
        raise RuntimeError("mano_backward: grad_verts and grad_joints are both None")
    vshape = (B, 3, 778) if channel_major else (B, 778, 3)
    for name, t, shape in (("grad_verts", grad_verts, vshape), ("grad_joints", grad_joints, (B, 16, 3))):
        if t is not None and tuple(_f32(t, name).shape) != shape:
            raise RuntimeError(f"mano_backward: expected {name} {list(shape)}, got {tuple(t.shape)}")
    if len(needs) != 4:
        raise RuntimeError("mano_backward: needs = (betas, hand_pose, global_orient, transl)")
    grad_verts = None if grad_verts is None else grad_verts.contiguous()
    grad_joints = None if grad_joints is None else grad_joints.contiguous()
    outs = [torch.empty(B, n, dtype=torch.float32, device=dev) if need else None for n, need in zip((10, 45, 3, 3), needs)]
    if B == 0:                                              # empty tensors have null data pointers, which the ABI refuses
        return tuple(outs)
    ptr = lambda t: None if t is None else t.data_ptr()
    nws = lib.dvq_mano_backward_workspace_bytes(B)
    ws = workspace(nws, dev)
    with torch.cuda.device(dev):
        check(lib.dvq_mano_backward(C.byref(packed.cstruct), packed.tensors["blend_wt"].data_ptr(), pb, ldb, pp, ldp, pg or None, ldg,
                                    pt or None, ldt, B, ptr(grad_verts), 1 if channel_major else 0, ptr(grad_joints),
                                    *[ptr(o) for o in outs], ws.data_ptr(), ws.numel(), _stream(dev)), "dvq_mano_backward")
    if _out_of_range(getattr(packed, "kind", None), *outs):
        from . import packing
        with no_range_check(), packing.gemm_kind_as(_lib.PLANES_BF16X3):     # the recomputed blendshapes once more on the six-product images
            return mano_backward(packed, betas, hand_pose, global_orient, transl, grad_verts, grad_joints, channel_major, needs)
    return tuple(outs)


# ------------------------------------------------------------------------------------------ data movement
def copy_cols(src: Tensor, out: Tensor) -> Tensor:
    lib = _lib.load()
    dev = _require_gpu(src, out)
    ps, lds = _rows(_f32(src, "src"), "src")
    po, ldo = _rows(_f32(out, "out"), "out")
    if src.shape != out.shape:
        raise RuntimeError("copy_cols: shape mismatch")
    with torch.cuda.device(dev):
        check(lib.dvq_copy_cols(ps, lds, src.shape[0], src.shape[1], po, ldo, _stream(dev)), "dvq_copy_cols")
    return out


def assemble61(recon: Tensor, recon_pos: Tensor) -> Tensor:
    lib = _lib.load()
    dev = _require_gpu(recon, recon_pos)
    B = recon.shape[0]
    if tuple(recon.shape) != (B, 55) or tuple(recon_pos.shape) != (B, 6) or not recon.is_contiguous() or not recon_pos.is_contiguous():
        raise RuntimeError("assemble61: expected contiguous recon [B,55] and recon_pos [B,6]")
    out = torch.empty(B, 61, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dvq_assemble61(_f32(recon, "recon").data_ptr(), _f32(recon_pos, "recon_pos").data_ptr(), B,
                                 out.data_ptr(), _stream(dev)), "dvq_assemble61")
    return out


def transform_cloud(pc: Tensor, R: Tensor, t: Optional[Tensor] = None) -> Tensor:
    """pc [C,N] (one object, broadcast) or [B,C,N]; R [B,3,3]; t [3] -> [B,C,N] with xyz' = R xyz + t."""
    lib = _lib.load()
    dev = _require_gpu(pc, R, t)
    _f32(pc, "pc"), _f32(R, "R")
    B = R.shape[0]
    if not pc.is_contiguous() or not R.is_contiguous() or tuple(R.shape[1:]) != (3, 3):
        raise RuntimeError("transform_cloud: expected contiguous pc and R [B,3,3]")
    if pc.dim() == 2:
        Cc, N = pc.shape
        bstride = 0
    else:
        if pc.shape[0] != B:
            raise RuntimeError("transform_cloud: batch mismatch")
        _, Cc, N = pc.shape
        bstride = Cc * N
    out = torch.empty(B, Cc, N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.dvq_transform_cloud(pc.data_ptr(), bstride, R.data_ptr(), t.data_ptr() if t is not None else None, B, Cc,
                                      N, out.data_ptr(), _stream(dev)), "dvq_transform_cloud")
    return out


def transform_clouds(pc: Tensor, obj_of_row: Tensor, R: Tensor, t: Optional[Tensor] = None, err: Optional[Tensor] = None) -> Tensor:
    """pc [O,C,N] (one cloud per object); obj_of_row int64 [B]; R [B,3,3]; t [3] -> [B,C,N] with row b = R[b] xyz(pc[obj_of_row[b]]) + t,
    the bits ``transform_cloud(pc[obj_of_row[b]], R[b:b+1], t)`` gives (dvq_transform_clouds); no per-grasp copy of the clouds.
    An index outside [0, O) raises RuntimeError unless an ``err`` flag tensor is supplied (then the caller checks it; the row is
    left unwritten)."""
    lib = _lib.load()
    dev = _require_gpu(pc, obj_of_row, R, t, err)
    _f32(pc, "pc"), _f32(R, "R")
    if t is not None and (_f32(t, "t").numel() != 3 or not t.is_contiguous()):
        raise RuntimeError("transform_clouds: expected contiguous t [3]")
    B = R.shape[0]
    if pc.dim() != 3 or not pc.is_contiguous() or not R.is_contiguous() or tuple(R.shape[1:]) != (3, 3):
        raise RuntimeError("transform_clouds: expected contiguous pc [O,C,N] and R [B,3,3]")
    _obj_of_row("transform_clouds", obj_of_row, B)
    O, Cc, N = pc.shape
    out = torch.empty(B, Cc, N, dtype=torch.float32, device=dev)
    with _err_flag(err, dev, f"transform_clouds: object index out of bounds for {O} clouds") as flag, torch.cuda.device(dev):
        check(lib.dvq_transform_clouds(pc.data_ptr(), obj_of_row.data_ptr(), O, R.data_ptr(), _ptr(t), B, Cc, N, out.data_ptr(),
                                       flag.data_ptr(), _stream(dev)), "dvq_transform_clouds")
    return out


# ---------------------------------------------------------------------------------------- contact / penetration proxies
def _points(x: Tensor, name: str):
    """[B,N,3]-shaped view (any strides: a permuted [B,C,N] cloud is read in place) -> (ptr, batch, point, coord strides)."""
    if x.dim() != 3 or x.shape[2] != 3:
        raise RuntimeError(f"{name}: expected [B,N,3] (got {tuple(x.shape)})")
    _f32(x, name)
    return (x.data_ptr(),) + x.stride()


def nn_points(src: Tensor, trg: Tensor):
    """Nearest target point per source point (utils_loss.get_NN): src [B,N1,3], trg [B,N2,3] -> (dist2 [B,N1] f32,
    idx [B,N1] int64).  d = fma(dz,dz, fma(dy,dy, dx*dx)); first minimum; NaN first."""
    lib = _lib.load()
    dev = _require_gpu(src, trg)
    ps, sb, sp, sc = _points(src, "src")
    pt, tb, tp, tc = _points(trg, "trg")
    B, N1, N2 = src.shape[0], src.shape[1], trg.shape[1]
    if trg.shape[0] != B:
        raise RuntimeError("nn_points: batch mismatch")
    dist = torch.empty(B, N1, dtype=torch.float32, device=dev)
    idx = torch.empty(B, N1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.dvq_nn_points(ps, sb, sp, sc, pt, tb, tp, tc, B, N1, N2, dist.data_ptr(), idx.data_ptr(), _stream(dev)),
              "dvq_nn_points")
    return dist, idx


def vertex_normals(verts: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor) -> Tensor:
    """Area-weighted unit vertex normals of B meshes with shared topology: verts [B,V,3]; faces [F,3], vf_off [V+1],
    vf_face [3F] int32 on the device (``contact.face_csr``)."""
    lib = _lib.load()
    dev = _require_gpu(verts, faces, vf_off, vf_face)
    _f32(verts, "verts")
    _int32_tables("vertex_normals", "faces vf_off vf_face", faces, vf_off, vf_face)
    if verts.dim() != 3 or verts.shape[2] != 3 or not verts.is_contiguous():
        raise RuntimeError("vertex_normals: verts must be contiguous [B,V,3]")
    B, V = verts.shape[0], verts.shape[1]
    if vf_off.numel() != V + 1 or vf_face.numel() != faces.numel():
        raise RuntimeError("vertex_normals: CSR does not match the mesh")
    out = torch.empty_like(verts)
    with torch.cuda.device(dev):
        check(lib.dvq_vertex_normals(verts.data_ptr(), B, V, faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(),
                                     out.data_ptr(), _stream(dev)), "dvq_vertex_normals")
    return out


def interior(normals: Tensor, hand: Tensor, obj: Tensor, nn_idx: Tensor) -> Tensor:
    """utils_loss.get_interior: bool [B,N], True where the object point lies behind its nearest hand vertex's surface."""
    lib = _lib.load()
    dev = _require_gpu(normals, hand, obj, nn_idx)
    _f32(normals, "normals"), _f32(hand, "hand"), _i64(nn_idx, "nn_idx")
    po, ob, op, oc = _points(obj, "obj")
    B, N, V = obj.shape[0], obj.shape[1], hand.shape[1]
    if not (normals.is_contiguous() and hand.is_contiguous() and nn_idx.is_contiguous()):
        raise RuntimeError("interior: normals, hand, nn_idx must be contiguous")
    if tuple(normals.shape) != tuple(hand.shape) or tuple(nn_idx.shape) != (B, N) or hand.shape[0] != B:
        raise RuntimeError("interior: shape mismatch")
    out = torch.empty(B, N, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.dvq_interior(normals.data_ptr(), hand.data_ptr(), V, po, ob, op, oc, nn_idx.data_ptr(), B, N,
                               out.data_ptr(), _stream(dev)), "dvq_interior")
    return out.bool()


GRASP_SCORES_MAX_V = 2048          # csrc/grasp_scan.h: GRASP_MAX_V (the hand and its normals sit in LDS)
SEGMENT_TOPK_MAX_M = 4096          # csrc/contact.hip: TOPK_MAX_M


def _hand_cloud_args(what: str, hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor):
    """The arguments ``grasp_scores``, ``grasp_wrench`` and ``grasp_refine`` share -- hand [B,V,3] contiguous, the topology of
    ``contact.face_csr``, obj [B,N,3] with any strides -- checked before any device use -> (obj's pointer and its three strides,
    B, V, N)."""
    _tensors(what, "hand obj faces vf_off vf_face", hand, obj, faces, vf_off, vf_face)
    _int32_tables(what, "faces vf_off vf_face", faces, vf_off, vf_face)
    po, ob, op, oc, B, V, N = _hand_cloud(what, hand, obj)
    _csr(what, faces, vf_off, vf_face, V)
    return po, ob, op, oc, B, V, N


def _hand(what: str, hand: Tensor, N: Optional[int] = None) -> Tuple[int, int]:
    """hand fp32 [B,V,3], contiguous, 1 <= V <= GRASP_SCORES_MAX_V -> (B, V).  A wrapper that scans a cloud passes its point count
    ``N``, which must be >= 1 and shares the bound's message."""
    _f32(hand, "hand")
    shape = hand.shape
    if len(shape) != 3 or shape[2] != 3 or not hand.is_contiguous():
        raise RuntimeError(f"{what}: hand must be contiguous [B,V,3]")
    B, V = shape[0], shape[1]
    if N is None:
        if not 1 <= V <= GRASP_SCORES_MAX_V:
            raise RuntimeError(f"{what}: need 1 <= V <= {GRASP_SCORES_MAX_V} (got V={V})")
    elif N < 1 or not 1 <= V <= GRASP_SCORES_MAX_V:
        raise RuntimeError(f"{what}: need N >= 1 and 1 <= V <= {GRASP_SCORES_MAX_V} (got N={N} V={V})")
    return B, V


def _hand_cloud(what: str, hand: Tensor, obj: Tensor):
    """``_hand`` against a cloud obj [B,N,3] with any strides -> (obj's pointer and its three strides, B, V, N)."""
    po, ob, op, oc = _points(obj, "obj")
    rows, N, _ = obj.shape
    B, V = _hand(what, hand, N)
    if rows != B:
        raise RuntimeError(f"{what}: batch mismatch")
    return po, ob, op, oc, B, V, N


def _csr(what: str, faces: Tensor, vf_off: Tensor, vf_face: Tensor, V: int) -> None:
    shape = faces.shape
    if len(shape) != 2 or shape[1] != 3 or vf_off.numel() != V + 1 or vf_face.numel() != 3 * shape[0]:
        raise RuntimeError(f"{what}: CSR does not match the mesh")


def _labels(what: str, V: int, names: str, *xs: Tensor) -> None:
    """Per-vertex tables (``part_of_vertex``, ``source_of_vertex``): contiguous int32 [V]."""
    for i, x in enumerate(xs):
        if x.dtype != torch.int32 or not x.is_contiguous() or x.shape != (V,):
            raise RuntimeError(f"{what}: {names.split()[i]} must be contiguous int32 [{V}] (got {x.dtype} {tuple(x.shape)})")


def _frame(what: str, R: Optional[Tensor], t: Optional[Tensor], B: int) -> None:
    """The object frame ``transform_clouds`` got: R [B,3,3] and t [3], fp32 and contiguous, or None for objects in place (the launch
    passes ``_ptr(R)``, ``_ptr(t)``)."""
    if R is None and t is not None:
        raise RuntimeError(f"{what}: t without R")
    if R is not None and (not isinstance(R, Tensor) or tuple(_f32(R, "R").shape) != (B, 3, 3) or not R.is_contiguous()):
        raise RuntimeError(f"{what}: expected contiguous R [B,3,3]")
    if t is not None and (not isinstance(t, Tensor) or _f32(t, "t").numel() != 3 or not t.is_contiguous()):
        raise RuntimeError(f"{what}: expected contiguous t [3]")


def grasp_scores(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor, contact_threshold: float = 0.02 ** 2):
    """Per-grasp ``(penetration [B] f32, n_interior [B] i32, n_contact [B] i32)`` in one fused kernel (dvq_grasp_scores): hand
    [B,V,3] contiguous, the topology of ``contact.face_csr`` on the device, obj [B,N,3] with any strides.  Per point the bits of
    ``vertex_normals`` / ``nn_points`` / ``interior``; the sums in the fixed order include/dvq.h documents."""
    po, ob, op, oc, B, V, N = _hand_cloud_args("grasp_scores", hand, faces, vf_off, vf_face, obj)
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face)
    lib = _lib.load()
    outs = _outputs(B, dev, (_F,), (_I,), (_I,))                                       # penetration, n_interior, n_contact
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_scores(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, po, ob, op, oc, B, N,
                                   float(contact_threshold), *map(_ptr, outs), _stream(dev)), "dvq_grasp_scores")
    return outs


GRASP_WRENCH_SUMS = 27             # csrc/grasp_wrench.hip: GW_SUMS (the wrench's 6 sums, then the upper triangle of sum w w^T)


def grasp_wrench(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor, inv_length: float,
                 contact_threshold: float = 0.02 ** 2):
    """The contact-wrench sums of every grasp in one fused kernel (dvq_grasp_wrench; the definition is in include/dvq.h):
    ``(penetration [B] f32, n_interior [B] i32, n_contact [B] i32, centre [B,3] f32, sums [B,27] f32, key [B] f32)``.  The first
    three are the bits of ``grasp_scores``; ``inv_length`` is the reciprocal of the length that scales torques to forces.
    Arguments as ``grasp_scores`` (obj [B,N,3] with any strides, read in place)."""
    po, ob, op, oc, B, V, N = _hand_cloud_args("grasp_wrench", hand, faces, vf_off, vf_face, obj)
    inv_length = _positive("grasp_wrench", "inv_length", inv_length)
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face)
    lib = _lib.load()
    outs = _outputs(B, dev, (_F,), (_I,), (_I,), (_F, 3), (_F, GRASP_WRENCH_SUMS), (_F,))   # penetration .. n_contact, centre, sums, key
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_wrench(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, po, ob, op, oc, B, N,
                                   float(contact_threshold), inv_length, *map(_ptr, outs), _stream(dev)), "dvq_grasp_wrench")
    return outs


GRASP_CLOSURE_MAX_DIRS = 1024      # include/dvq.h: DVQ_GRASP_CLOSURE_MAX_DIRS (a thread of the workgroup owns at most four directions)


def grasp_closure(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor, inv_length: float, mu: float, dirs: Tensor,
                  contact_threshold: float = 0.02 ** 2, want_support: bool = False):
    """Force-closure quality with friction in one fused kernel (dvq_grasp_closure; the definition is in include/dvq.h):
    ``(quality [B] f32, worst_dir [B] i32, status [B] i32, n_contact [B] i32, centre [B,3] f32, support)`` -- per grasp the smallest
    value over ``dirs`` [D,6] (fp32, contiguous, on the device, 1 <= D <= GRASP_CLOSURE_MAX_DIRS) of the support function of the
    contacts' friction cones at coefficient ``mu`` (finite, >= 0), the lowest direction that attains it, 0 / 1 (no contact) / 2 (a
    coordinate is not finite), the contact count of ``grasp_scores`` and the centre of ``grasp_wrench``; with ``want_support`` the
    whole [B,D] support table as well (None otherwise).  Arguments as ``grasp_wrench`` (obj [B,N,3] with any strides, read in place)."""
    po, ob, op, oc, B, V, N = _hand_cloud_args("grasp_closure", hand, faces, vf_off, vf_face, obj)
    inv_length = _positive("grasp_closure", "inv_length", inv_length)
    mu = _non_negative("grasp_closure", "mu", mu)
    _tensors("grasp_closure", "dirs", dirs)
    if _f32(dirs, "dirs").dim() != 2 or dirs.shape[1] != 6 or not dirs.is_contiguous() or not 1 <= dirs.shape[0] <= GRASP_CLOSURE_MAX_DIRS:
        raise RuntimeError(f"grasp_closure: dirs must be contiguous [D,6] with 1 <= D <= {GRASP_CLOSURE_MAX_DIRS} (got {tuple(dirs.shape)})")
    D = dirs.shape[0]
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face, dirs)
    lib = _lib.load()
    # quality, worst_dir, status, n_contact, centre, support
    outs = _outputs(B, dev, (_F,), (_I,), (_I,), (_I,), (_F, 3), (_F, D) if want_support else None)
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_closure(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, po, ob, op, oc, B, N,
                                    float(contact_threshold), inv_length, mu, dirs.data_ptr(), D, *map(_ptr, outs), _stream(dev)),
              "dvq_grasp_closure")
    return outs


GRASP_PARTS_TILE = 2048            # csrc/grasp_parts.hip: GP_TILE (the cloud's points per LDS tile)
GRASP_PARTS_MAX_P = 32             # GP_MAX_P


def grasp_parts(hand: Tensor, part_of_vertex: Tensor, n_parts: int, obj: Tensor, contact_threshold: float, want_verts: bool = False):
    """Contact from the hand's side in one fused kernel (dvq_grasp_parts; the definition is in include/dvq.h): hand [B,V,3]
    contiguous, ``part_of_vertex`` int32 [V] on the device (a label outside [0, n_parts) is "no part"), obj [B,N,3] with any strides
    (read in place), ``contact_threshold`` a squared distance.  Returns ``(part_min [B,P] f32, part_count [B,P] i32, mask [B,W] i32,
    status [B] i32, vert_dist, vert_idx)``: per part the smallest squared distance from one of its vertices to the cloud and the
    number of its vertices closer than the threshold, a bit per vertex (W = (V + 31) // 32), status 1 for a row with a non-finite
    coordinate (NaN / -1 / 0 there), and with ``want_verts`` the bits of ``nn_points(hand, obj)`` as f32 [B,V] and int32 [B,V]
    (None otherwise)."""
    _tensors("grasp_parts", "hand part_of_vertex obj", hand, part_of_vertex, obj)
    po, ob, op, oc, B, V, N = _hand_cloud("grasp_parts", hand, obj)
    n_parts = int(n_parts)
    if not 1 <= n_parts <= GRASP_PARTS_MAX_P:
        raise RuntimeError(f"grasp_parts: need 1 <= n_parts <= {GRASP_PARTS_MAX_P} (got {n_parts})")
    _labels("grasp_parts", V, "part_of_vertex", part_of_vertex)
    contact_threshold = float(contact_threshold)
    if math.isnan(contact_threshold):
        raise RuntimeError("grasp_parts: contact_threshold is NaN")
    dev = _require_gpu(hand, obj, part_of_vertex)
    lib = _lib.load()
    # part_min, part_count, mask, status, vert_dist, vert_idx
    outs = _outputs(B, dev, (_F, n_parts), (_I, n_parts), (_I, (V + 31) // 32), (_I,), *(((_F, V), (_I, V)) if want_verts else (None, None)))
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_parts(hand.data_ptr(), part_of_vertex.data_ptr(), V, n_parts, po, ob, op, oc, B, N, contact_threshold,
                                  *map(_ptr, outs), _stream(dev)), "dvq_grasp_parts")
    return outs


GRASP_SELF_MAX_P = 32               # csrc/grasp_self.hip: GSELF_MAX_P (one bit per part)


def _pair_words(what: str, pairs, n_parts: int):
    """``pairs`` (a sequence of ints or an integer array) of ``grasp_self`` / ``contact.SelfTable`` -> (its ``n_parts`` words as ints,
    the first index whose word names a part outside [0, n_parts) or its own part -- the caller words that refusal -- or None)."""
    words = [int(w) for w in (pairs.tolist() if hasattr(pairs, "tolist") else pairs)]
    if len(words) != n_parts:
        raise RuntimeError(f"{what}: pairs must hold {n_parts} words, one per part (got {len(words)})")
    top = 1 << n_parts
    for a, w in enumerate(words):
        if not 0 <= w < top or (w >> a) & 1:
            return words, a
    return words, None


def grasp_self(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, part_of_vertex: Tensor, source_of_vertex: Tensor,
               n_parts: int, pairs, reach2: float, margin: float):
    """Self-collision of hands in one fused kernel (dvq_grasp_self; the definition is in include/dvq.h): hand [B,V,3] contiguous,
    the topology of ``contact.face_csr`` on the device, ``part_of_vertex`` and ``source_of_vertex`` int32 [V] on the device (a label
    outside [0, n_parts) is "no part"; a vertex with source 0 never counts, it remains a target), ``pairs``: ``n_parts`` words on
    the HOST (a sequence of ints or an integer array), bit b of ``pairs[a]`` = part a's vertices are tested against part b's;
    ``reach2`` a squared distance, ``margin`` a distance.  Returns ``(pen_count [B,P] i32, pen_depth [B,P] f32, gap_min [B,P] f32,
    pair_bits [B,P] i32, mask [B,W] i32, status [B] i32)``: per part the number of penetrating vertices, the largest depth (+0.0
    without one), the smallest squared distance of a source vertex to its targets (+inf without one) and the parts hit, a bit per
    vertex (W = (V + 31) // 32), status 1 for a row with a non-finite coordinate (-1 / NaN / NaN / 0 / 0 there)."""
    what = "grasp_self"
    _tensors(what, "hand faces vf_off vf_face part_of_vertex source_of_vertex", hand, faces, vf_off, vf_face, part_of_vertex, source_of_vertex)
    _int32_tables(what, "faces vf_off vf_face", faces, vf_off, vf_face)
    B, V = _hand(what, hand)
    _csr(what, faces, vf_off, vf_face, V)
    n_parts = int(n_parts)
    if not 1 <= n_parts <= GRASP_SELF_MAX_P:
        raise RuntimeError(f"grasp_self: need 1 <= n_parts <= {GRASP_SELF_MAX_P} (got {n_parts})")
    _labels(what, V, "part_of_vertex source_of_vertex", part_of_vertex, source_of_vertex)
    words, a = _pair_words(what, pairs, n_parts)
    if a is not None:
        raise RuntimeError(f"grasp_self: pairs[{a}] tests part {a} against itself" if 0 <= words[a] < 1 << n_parts else
                           f"grasp_self: pairs[{a}] = {words[a]:#x} names a part at or above n_parts = {n_parts} (or is negative)")
    reach2, margin = _positive(what, "reach2", reach2), _non_negative(what, "margin", margin)
    dev = _require_gpu(hand, faces, vf_off, vf_face, part_of_vertex, source_of_vertex)
    lib = _lib.load()
    # pen_count, pen_depth, gap_min, pair_bits, mask, status
    outs = _outputs(B, dev, (_I, n_parts), (_F, n_parts), (_F, n_parts), (_I, n_parts), (_I, (V + 31) // 32), (_I,))
    host_pairs = (C.c_uint32 * n_parts)(*words)                # read by the library before the call returns
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_self(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, part_of_vertex.data_ptr(),
                                 source_of_vertex.data_ptr(), n_parts, C.addressof(host_pairs), B, reach2, margin,
                                 *map(_ptr, outs), _stream(dev)), "dvq_grasp_self")
    return outs


GRASP_TTT_MAX_N = 16384             # include/dvq.h: DVQ_GRASP_TTT_MAX_N (one word per object point sits in LDS)


def grasp_ttt(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor, targets: Optional[Tensor] = None,
              w_pen: Optional[Tensor] = None, w_con: Optional[Tensor] = None, mean_contact: bool = False, want_grad: bool = False,
              contact_threshold: float = 0.02 ** 2):
    """The two terms of the reference's test-time loss and their gradient with respect to the hand in one fused kernel
    (dvq_grasp_ttt; the definition is in include/dvq.h): arguments as ``grasp_scores``; ``targets`` int32 [V] on the device (nonzero =
    the vertex is a contact target) or None for every vertex; ``w_pen`` / ``w_con`` fp32 [B] on the device or None (= 1): the
    weights of the two terms in the gradient; ``mean_contact``: the contact weight is divided by max(n_contact, 1).  Returns
    ``(penetration [B] f32, contact_sum [B] f32, n_interior [B] i32, n_contact [B] i32, grad_hand [B,V,3] f32 or None)``; without
    ``want_grad`` the gradient phase does not run.  A row with a non-finite coordinate has a NaN contact sum and a NaN gradient."""
    po, ob, op, oc, B, V, N = _hand_cloud_args("grasp_ttt", hand, faces, vf_off, vf_face, obj)
    if N > GRASP_TTT_MAX_N:
        raise RuntimeError(f"grasp_ttt: need N <= {GRASP_TTT_MAX_N} (got N={N})")
    if targets is not None and (not isinstance(targets, Tensor) or targets.dtype != torch.int32 or not targets.is_contiguous()
                                or tuple(targets.shape) != (V,)):
        raise RuntimeError(f"grasp_ttt: targets must be a contiguous int32 tensor [{V}] or None")
    for t, n in ((w_pen, "w_pen"), (w_con, "w_con")):
        if t is not None and (not isinstance(t, Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B,)):
            raise RuntimeError(f"grasp_ttt: {n} must be a contiguous float32 tensor [{B}] or None")
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face, targets, w_pen, w_con)
    lib = _lib.load()
    # penetration, contact_sum, n_interior, n_contact, grad_hand
    outs = _outputs(B, dev, (_F,), (_F,), (_I,), (_I,), (_F, V, 3) if want_grad else None)
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_ttt(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, po, ob, op, oc, B, N,
                                float(contact_threshold), _ptr(targets), _ptr(w_pen), _ptr(w_con), 1 if mean_contact else 0,
                                *map(_ptr, outs), _stream(dev)), "dvq_grasp_ttt")
    return outs


GRASP_VOLUME_MAX_F = 8192         # csrc/grasp_volume.hip: GV_MAX_F
GRASP_VOLUME_MAX_LOOPS = 64        # GV_MAX_L
GRASP_VOLUME_MAX_PLANES = 8192     # GV_MAX_P: per object
GRASP_VOLUME_MAX_CELLS = 1024      # GV_MAX_CELLS: per axis of a hand's box; beyond it the grasp reports status 2


def grasp_volume(hand: Tensor, faces: Tensor, loop_off: Tensor, loop_vert: Tensor, planes: Tensor, plane_off: Tensor,
                 obj_of_row: Tensor, R: Optional[Tensor] = None, t: Optional[Tensor] = None, res: float = 0.001,
                 err: Optional[Tensor] = None):
    """The voxels shared by the sealed hand mesh and the object's convex hull, and the deepest hand vertex inside the hull, in one
    fused kernel (dvq_grasp_volume; the definition is in include/dvq.h): ``(count [B] i32, depth [B] f32, status [B] i32)``.
    hand [B,V,3] contiguous; faces [F,3] int32 with indices below V + L, loop_off [L+1] and loop_vert int32 (``contact.seal_faces``);
    planes [P,4] f32 rows (n, d) with n.x <= d inside, plane_off int32 [O+1] (``contact.pack_planes``); obj_of_row int64 [B]; R [B,3,3]
    and t [3] as ``transform_clouds`` got them, or None for objects in place; ``res``: the lattice spacing.  An object index outside
    [0, O) raises RuntimeError unless an ``err`` flag tensor is supplied (then the caller checks it: bit 0; bit 1 = an index of the
    topology or a plane range out of bounds)."""
    what = "grasp_volume"
    _tensors(what, "hand faces loop_off loop_vert planes plane_off obj_of_row", hand, faces, loop_off, loop_vert, planes, plane_off, obj_of_row)
    _f32(planes, "planes")
    _int32_tables(what, "faces loop_off loop_vert plane_off", faces, loop_off, loop_vert, plane_off)
    B, V = _hand(what, hand)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] > GRASP_VOLUME_MAX_F:
        raise RuntimeError(f"grasp_volume: faces must be [F,3] with F <= {GRASP_VOLUME_MAX_F} (got {tuple(faces.shape)})")
    if loop_off.dim() != 1 or not 1 <= loop_off.numel() <= GRASP_VOLUME_MAX_LOOPS + 1 or loop_vert.dim() != 1:
        raise RuntimeError(f"grasp_volume: loop_off must be [L+1] with L <= {GRASP_VOLUME_MAX_LOOPS} and loop_vert 1-D")
    if planes.dim() != 2 or planes.shape[1] != 4 or not planes.is_contiguous() or planes.shape[0] >= 2 ** 31:
        raise RuntimeError("grasp_volume: planes must be contiguous [P,4]")
    if plane_off.dim() != 1 or plane_off.numel() < 1:
        raise RuntimeError("grasp_volume: plane_off must be [O+1]")
    _obj_of_row(what, obj_of_row, B)
    _frame(what, R, t, B)
    res = _positive(what, "res", res)
    dev = _require_gpu(hand, faces, loop_off, loop_vert, planes, plane_off, obj_of_row, R, t, err)
    lib = _lib.load()
    outs = _outputs(B, dev, (_I,), (_F,), (_I,))                                       # count, depth, status
    message = lambda bad: (f"grasp_volume: object index out of bounds for {plane_off.numel() - 1} objects" if bad & 1 else
                           "grasp_volume: an index of the topology or a plane range is out of bounds")
    with _err_flag(err, dev, message) as flag, torch.cuda.device(dev):
        check(lib.dvq_grasp_volume(hand.data_ptr(), V, faces.data_ptr(), faces.shape[0], loop_off.data_ptr(), loop_vert.data_ptr(),
                                   loop_off.numel() - 1, loop_vert.numel(), planes.data_ptr(), planes.shape[0], plane_off.data_ptr(),
                                   plane_off.numel() - 1, obj_of_row.data_ptr(), _ptr(R), _ptr(t), B, res, *map(_ptr, outs), flag.data_ptr(),
                                   _stream(dev)), "dvq_grasp_volume")
    return outs


GRASP_MESH_MAX_FACES = 262144      # include/dvq.h: DVQ_GRASP_MESH_MAX_FACES, per object
GRASP_MESH_TILE = 256              # csrc/grasp_mesh.hip: GM_TILE (the faces per LDS tile)


def _mesh_tables(what: str, mesh_verts: Tensor, vert_off: Tensor, mesh_faces: Tensor, face_off: Tensor) -> int:
    """The shapes of the four CSR tables of ``contact.ObjectMeshes`` (their dtypes are checked before) -> O."""
    if mesh_verts.dim() != 2 or mesh_verts.shape[1] != 3 or not mesh_verts.is_contiguous() or mesh_verts.shape[0] >= 2 ** 31:
        raise RuntimeError(f"{what}: mesh_verts must be contiguous [n,3]")
    if mesh_faces.dim() != 2 or mesh_faces.shape[1] != 3 or mesh_faces.shape[0] >= 2 ** 31:
        raise RuntimeError(f"{what}: mesh_faces must be contiguous [m,3]")
    if vert_off.dim() != 1 or vert_off.numel() < 1 or face_off.dim() != 1 or face_off.numel() != vert_off.numel():
        raise RuntimeError(f"{what}: vert_off and face_off must both be [O+1]")
    return vert_off.numel() - 1


def grasp_mesh(hand: Tensor, mesh_verts: Tensor, vert_off: Tensor, mesh_faces: Tensor, face_off: Tensor, obj_of_row: Tensor,
               R: Optional[Tensor] = None, t: Optional[Tensor] = None, want_verts: bool = False, err: Optional[Tensor] = None):
    """The hand vertices inside each row's object MESH (parity along +z, watertight at edges and vertices) and the largest distance
    of one of them to the surface, in one fused kernel (dvq_grasp_mesh; the definition is in include/dvq.h): ``(n_inside [B] i32,
    depth [B] f32, deep_vertex [B] i32, deep_face [B] i32, inside_mask [B,W] i32, status [B] i32, vert_d2, vert_face)``.
    hand [B,V,3] contiguous; mesh_verts [n,3] f32 and vert_off int32 [O+1], mesh_faces [m,3] int32 (indices local to the object's
    vertices) and face_off int32 [O+1] (``contact.ObjectMeshes``); obj_of_row int64 [B]; R [B,3,3] and t [3] as ``transform_clouds``
    got them, or None for objects in place.  With ``want_verts`` every inside vertex's squared distance and nearest face as f32 /
    int32 [B,V] (+inf / -1 outside; None otherwise).  An object index outside [0, O) raises RuntimeError unless an ``err`` flag tensor
    is supplied (then the caller checks it: bit 0; bit 1 = a face index or an object's range out of bounds)."""
    what = "grasp_mesh"
    _tensors(what, "hand mesh_verts vert_off mesh_faces face_off obj_of_row", hand, mesh_verts, vert_off, mesh_faces, face_off, obj_of_row)
    _f32(mesh_verts, "mesh_verts")
    _int32_tables(what, "vert_off mesh_faces face_off", vert_off, mesh_faces, face_off)
    B, V = _hand(what, hand)
    _mesh_tables(what, mesh_verts, vert_off, mesh_faces, face_off)
    _obj_of_row(what, obj_of_row, B)
    _frame(what, R, t, B)
    dev = _require_gpu(hand, mesh_verts, vert_off, mesh_faces, face_off, obj_of_row, R, t, err)
    lib = _lib.load()
    # n_inside, depth, deep_vertex, deep_face, mask, status, vert_d2, vert_face
    outs = _outputs(B, dev, (_I,), (_F,), (_I,), (_I,), (_I, (V + 31) // 32), (_I,), *(((_F, V), (_I, V)) if want_verts else (None, None)))
    message = lambda bad: (f"grasp_mesh: object index out of bounds for {vert_off.numel() - 1} objects" if bad & 1 else
                           "grasp_mesh: a face index or an object's vertex / face range is out of bounds")
    with _err_flag(err, dev, message) as flag, torch.cuda.device(dev):
        check(lib.dvq_grasp_mesh(hand.data_ptr(), V, mesh_verts.data_ptr(), mesh_verts.shape[0], vert_off.data_ptr(),
                                 mesh_faces.data_ptr(), mesh_faces.shape[0], face_off.data_ptr(), vert_off.numel() - 1,
                                 obj_of_row.data_ptr(), _ptr(R), _ptr(t), B, *map(_ptr, outs), flag.data_ptr(), _stream(dev)),
              "dvq_grasp_mesh")
    return outs


GRASP_MESH_VOLUME_LIST = 2048      # csrc/grasp_mesh_volume.hip: GMV_LIST (the culled faces a grasp keeps in LDS; more: every tile walks all)


def grasp_mesh_volume(hand: Tensor, faces: Tensor, loop_off: Tensor, loop_vert: Tensor, mesh_verts: Tensor, vert_off: Tensor,
                      mesh_faces: Tensor, face_off: Tensor, obj_of_row: Tensor, R: Optional[Tensor] = None, t: Optional[Tensor] = None,
                      res: float = 0.001, err: Optional[Tensor] = None):
    """The voxels shared by the sealed hand mesh and each row's object MESH (not its hull: hollows and holes are seen) in one fused
    kernel (dvq_grasp_mesh_volume; the definition is in include/dvq.h): ``(count [B] i32, status [B] i32)``; no depth -- the depth
    against the mesh is ``grasp_mesh``'s.  hand, faces, loop_off, loop_vert, R, t and ``res`` as ``grasp_volume`` takes them; mesh_verts,
    vert_off, mesh_faces, face_off as ``grasp_mesh`` takes them (``contact.ObjectMeshes``); obj_of_row int64 [B].  An object index
    outside [0, O) raises RuntimeError unless an ``err`` flag tensor is supplied (then the caller checks it: bit 0; bit 1 = an index of
    the topology, a face index or an object's vertex / face range out of bounds)."""
    what = "grasp_mesh_volume"
    _tensors(what, "hand faces loop_off loop_vert mesh_verts vert_off mesh_faces face_off obj_of_row", hand, faces, loop_off, loop_vert,
             mesh_verts, vert_off, mesh_faces, face_off, obj_of_row)
    _f32(mesh_verts, "mesh_verts")
    _int32_tables(what, "faces loop_off loop_vert vert_off mesh_faces face_off", faces, loop_off, loop_vert, vert_off, mesh_faces, face_off)
    B, V = _hand(what, hand)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] > GRASP_VOLUME_MAX_F:
        raise RuntimeError(f"grasp_mesh_volume: faces must be [F,3] with F <= {GRASP_VOLUME_MAX_F} (got {tuple(faces.shape)})")
    if loop_off.dim() != 1 or not 1 <= loop_off.numel() <= GRASP_VOLUME_MAX_LOOPS + 1 or loop_vert.dim() != 1:
        raise RuntimeError(f"grasp_mesh_volume: loop_off must be [L+1] with L <= {GRASP_VOLUME_MAX_LOOPS} and loop_vert 1-D")
    _mesh_tables(what, mesh_verts, vert_off, mesh_faces, face_off)
    _obj_of_row(what, obj_of_row, B)
    _frame(what, R, t, B)
    res = _positive(what, "res", res)
    dev = _require_gpu(hand, faces, loop_off, loop_vert, mesh_verts, vert_off, mesh_faces, face_off, obj_of_row, R, t, err)
    lib = _lib.load()
    outs = _outputs(B, dev, (_I,), (_I,))                                              # count, status
    message = lambda bad: (f"grasp_mesh_volume: object index out of bounds for {vert_off.numel() - 1} objects" if bad & 1 else
                           "grasp_mesh_volume: an index of the topology, a face index or an object's vertex / face range is out of bounds")
    with _err_flag(err, dev, message) as flag, torch.cuda.device(dev):
        check(lib.dvq_grasp_mesh_volume(hand.data_ptr(), V, faces.data_ptr(), faces.shape[0], loop_off.data_ptr(), loop_vert.data_ptr(),
                                        loop_off.numel() - 1, loop_vert.numel(), mesh_verts.data_ptr(), mesh_verts.shape[0],
                                        vert_off.data_ptr(), mesh_faces.data_ptr(), mesh_faces.shape[0], face_off.data_ptr(),
                                        vert_off.numel() - 1, obj_of_row.data_ptr(), _ptr(R), _ptr(t), B, res, *map(_ptr, outs),
                                        flag.data_ptr(), _stream(dev)), "dvq_grasp_mesh_volume")
    return outs


GRASP_REFINE_MAX_STEPS = 64        # csrc/grasp_refine.hip: GR_MAX_STEPS
GRASP_FINGERS_MAX_P = 5            # csrc/grasp_refine.hip: GR_MAX_P


def _refine_steps(what: str, steps) -> int:
    steps = int(steps)
    if not 0 <= steps <= GRASP_REFINE_MAX_STEPS:
        raise RuntimeError(f"{what}: need 0 <= steps <= {GRASP_REFINE_MAX_STEPS} (got {steps})")
    return steps


def _refine_factors(what: str, **factors):
    """The step factors as floats, in the order given; each must be finite and >= 0 (a NaN compares false)."""
    names, vals = list(factors), [float(v) for v in factors.values()]
    if not all(0.0 <= v < float("inf") for v in vals):
        raise RuntimeError(f"{what}: {', '.join(names[:-1])} and {names[-1]} must be finite and >= 0 (got {', '.join(map(str, vals))})")
    return vals


def _refine_rows(what: str, name: str, x, shape, shown=None) -> None:
    """``pivot`` / ``knuckle``: an fp32 tensor of exactly ``shape`` = [B,...], contiguous."""
    if not isinstance(x, Tensor):
        raise RuntimeError(f"{what}: {name} must be a tensor")
    _f32(x, name)
    if tuple(x.shape) != shape or not x.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be contiguous {shown or list(shape)} (got {tuple(x.shape)})")


_REFINE_SCORES = ((_F,), (_I,), (_I,))                   # penetration, n_interior, n_contact of an iterate
_REFINE_BEST = ((_I,),) + _REFINE_SCORES                  # iter, then the scores of the iterate kept: the tail of every level's outputs


def grasp_refine(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor, steps: int, push: float = 1.0,
                 pull: float = 0.25, min_contact: int = 1, contact_threshold: float = 0.02 ** 2):
    """Translation push-out in one fused kernel (dvq_grasp_refine; the definition is in include/dvq.h): at most ``steps`` steps of
    descent on the scores of ``grasp_scores`` with respect to the hand's translation.  Returns ``(offset [B,3] f32, iter [B] i32,
    penetration [B] f32, n_interior [B] i32, n_contact [B] i32)`` of each grasp's best iterate -- add ``offset`` to the hand's
    translation.  Arguments as ``grasp_scores`` (obj [B,N,3] with any strides, read in place)."""
    what = "grasp_refine"
    po, ob, op, oc, B, V, N = _hand_cloud_args(what, hand, faces, vf_off, vf_face, obj)
    steps, min_contact = _refine_steps(what, steps), int(min_contact)
    push, pull = _refine_factors(what, push=push, pull=pull)
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face)
    lib = _lib.load()
    outs = _outputs(B, dev, (_F, 3), *_REFINE_BEST)                                    # offset, iter, penetration, n_interior, n_contact
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_refine(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, po, ob, op, oc, B, N,
                                   float(contact_threshold), steps, push, pull, min_contact, *(t.data_ptr() for t in outs),
                                   _stream(dev)), "dvq_grasp_refine")
    return outs


def grasp_refine_rigid(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor, pivot: Tensor, steps: int,
                       push: float = 1.0, pull: float = 0.25, spin: float = 1.0, min_contact: int = 1,
                       contact_threshold: float = 0.02 ** 2):
    """Rigid push-out in one fused kernel (dvq_grasp_refine_rigid; the definition is in include/dvq.h): ``grasp_refine`` whose state
    is a translation and a unit quaternion about ``pivot`` [B,3] (fp32, contiguous: the wrist of every hand).  Returns ``(offset
    [B,3] f32, quat [B,4] f32 (w, x, y, z), iter [B] i32, penetration [B] f32, n_interior [B] i32, n_contact [B] i32)`` of each
    grasp's best iterate: the refined hand is ``R(quat) (v - pivot) + pivot + offset``.  ``spin = 0`` gives ``grasp_refine``'s bits
    and the identity quaternion.  Other arguments as ``grasp_refine``."""
    what = "grasp_refine_rigid"
    po, ob, op, oc, B, V, N = _hand_cloud_args(what, hand, faces, vf_off, vf_face, obj)
    _refine_rows(what, "pivot", pivot, (B, 3), f"[B,3] = [{B},3]")
    steps, min_contact = _refine_steps(what, steps), int(min_contact)
    push, pull, spin = _refine_factors(what, push=push, pull=pull, spin=spin)
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face, pivot)
    lib = _lib.load()
    outs = _outputs(B, dev, (_F, 3), (_F, 4), *_REFINE_BEST)                           # offset, quat, iter, penetration, n_interior, n_contact
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_refine_rigid(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, po, ob, op, oc, B,
                                         N, pivot.data_ptr(), float(contact_threshold), steps, push, pull, spin, min_contact,
                                         *(t.data_ptr() for t in outs), _stream(dev)), "dvq_grasp_refine_rigid")
    return outs


def grasp_refine_fingers(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, vert_part: Tensor, vert_w: Tensor, n_fingers: int,
                         obj: Tensor, pivot: Tensor, knuckle: Tensor, steps: int, push: float = 1.0, pull: float = 0.25,
                         spin: float = 1.0, curl: float = 1.0, max_curl: float = 0.35, min_contact: int = 1,
                         contact_threshold: float = 0.02 ** 2):
    """Articulated push-out in one fused kernel (dvq_grasp_refine_fingers; the definition is in include/dvq.h): ``grasp_refine_rigid``
    whose state also holds one unit quaternion per finger, a turn of the finger about its knuckle.  ``vert_part`` int32 [V] (-1, or the
    vertex's finger in [0, n_fingers); checked here, on the host, when it lives there -- a device tensor is the caller's word, and the
    kernel treats a label outside the range as -1), ``vert_w`` f32 [V] (the blend weight in [0, 1]), ``knuckle`` [B,P,3] (fp32,
    contiguous: every finger's pivot), ``max_curl`` (radians, 0 < max_curl <= pi: no finger turns further from the hand as given).
    Returns ``(offset [B,3], quat [B,4], finger_quat [B,P,4], iter [B], penetration [B], n_interior [B], n_contact [B],
    penetration0 [B], n_interior0 [B], n_contact0 [B])``: the best iterate as ``grasp_refine_rigid`` reports it, its finger
    quaternions (w, x, y, z) and the three scores of iterate 0, which are ``grasp_scores`` of the input.  ``curl = 0`` gives
    ``grasp_refine_rigid``'s bits and identity finger quaternions."""
    what = "grasp_refine_fingers"
    po, ob, op, oc, B, V, N = _hand_cloud_args(what, hand, faces, vf_off, vf_face, obj)
    P = int(n_fingers)
    if not 1 <= P <= GRASP_FINGERS_MAX_P:
        raise RuntimeError(f"grasp_refine_fingers: need 1 <= n_fingers <= {GRASP_FINGERS_MAX_P} (got {P})")
    for name, x, dt in (("vert_part", vert_part, torch.int32), ("vert_w", vert_w, torch.float32)):
        if not isinstance(x, Tensor) or x.dtype != dt or tuple(x.shape) != (V,) or not x.is_contiguous():
            raise RuntimeError(f"grasp_refine_fingers: {name} must be a contiguous {dt} tensor [V] = [{V}]")
    if vert_part.device.type == "cpu" and V and (int(vert_part.min()) < -1 or int(vert_part.max()) >= P):
        raise RuntimeError(f"grasp_refine_fingers: vert_part must lie in [-1, {P}) (got {int(vert_part.min())} .. {int(vert_part.max())})")
    if vert_w.device.type == "cpu" and V and not bool(((vert_w >= 0) & (vert_w <= 1)).all()):
        raise RuntimeError("grasp_refine_fingers: vert_w must lie in [0, 1]")
    _refine_rows(what, "pivot", pivot, (B, 3))
    _refine_rows(what, "knuckle", knuckle, (B, P, 3))
    steps, min_contact, max_curl = _refine_steps(what, steps), int(min_contact), float(max_curl)
    push, pull, spin, curl = _refine_factors(what, push=push, pull=pull, spin=spin, curl=curl)
    if not 0.0 < max_curl <= math.pi:
        raise RuntimeError(f"grasp_refine_fingers: need 0 < max_curl <= pi (got {max_curl})")
    min_w = math.cos(0.5 * max_curl)                                                   # float64; rounded once, to fp32, by the call
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face, vert_part, vert_w, pivot, knuckle)
    lib = _lib.load()
    # offset, quat, finger_quat, iter, penetration, n_interior, n_contact, then iterate 0's penetration0, n_interior0, n_contact0
    outs = _outputs(B, dev, (_F, 3), (_F, 4), (_F, P, 4), *_REFINE_BEST, *_REFINE_SCORES)
    with torch.cuda.device(dev):
        check(lib.dvq_grasp_refine_fingers(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, vert_part.data_ptr(),
                                           vert_w.data_ptr(), P, po, ob, op, oc, B, N, pivot.data_ptr(), knuckle.data_ptr(),
                                           float(contact_threshold), steps, push, pull, spin, curl, min_w, min_contact,
                                           *(t.data_ptr() for t in outs), _stream(dev)), "dvq_grasp_refine_fingers")
    return outs


def segment_topk(cls: Tensor, key: Tensor, n_objects: int, n_candidates: int, keep: int) -> Tensor:
    """cls int32 [O*M], key f32 [O*M] (candidate c of object o at o * M + c) -> int64 [O,keep]: each object's ``keep`` best
    candidate indices, best first, by (cls, key, index) with NaN keys last in their class and -0.0 == +0.0 (dvq_segment_topk)."""
    if not isinstance(cls, Tensor) or not isinstance(key, Tensor):
        raise RuntimeError("segment_topk: cls and key must be tensors")
    O, M, keep = int(n_objects), int(n_candidates), int(keep)
    if cls.dtype != torch.int32:
        raise RuntimeError(f"segment_topk: cls: expected int32, got {cls.dtype}")
    _f32(key, "key")
    if O < 0 or not 1 <= keep <= M <= SEGMENT_TOPK_MAX_M:
        raise RuntimeError(f"segment_topk: need O >= 0 and 1 <= keep <= M <= {SEGMENT_TOPK_MAX_M} (got O={O} M={M} keep={keep})")
    if cls.dim() != 1 or key.dim() != 1 or cls.numel() != O * M or key.numel() != O * M or not cls.is_contiguous() or not key.is_contiguous():
        raise RuntimeError(f"segment_topk: cls and key must be contiguous [O*M] = [{O * M}] (got {tuple(cls.shape)}, {tuple(key.shape)})")
    dev = _require_gpu(cls, key)
    lib = _lib.load()
    sel = torch.empty(O, keep, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.dvq_segment_topk(cls.data_ptr(), key.data_ptr(), O, M, keep, sel.data_ptr(), _stream(dev)), "dvq_segment_topk")
    return sel


SEGMENT_DIVERSE_MAX_D = 4096       # csrc/diverse.hip: DIV_MAX (M, P and D)
SEGMENT_DIVERSE_LDS_FLOATS = 40960  # csrc/diverse.hip: DIV_LDS_FLOATS, the 160 KiB one workgroup may hold


def segment_diverse_lds_resident(pool: int, n_features: int) -> bool:
    """True when ``segment_diverse`` keeps the pooled rows in LDS (csrc/diverse.hip: 32 floats of header, one float of state per
    pool position rounded up to four, the rows at the odd stride D | 1), False when it streams them from global memory every step.
    The two paths give the same bits."""
    P, D = int(pool), int(n_features)
    return 32 + ((P + 3) & ~3) + P * (D | 1) <= SEGMENT_DIVERSE_LDS_FLOATS


def _segment_feat(what: str, feat: Tensor, rows: int, max_d: int, d_note: str = "") -> Tuple[int, int]:
    """The feature matrix of the segment kernels: [rows, D] with 1 <= D <= ``max_d``, ``stride(1) == 1`` and rows that do not
    overlap -> (row stride, D)."""
    shape, stride = feat.shape, feat.stride()
    if len(shape) != 2 or shape[0] != rows:
        raise RuntimeError(f"{what}: feat must be [O*M, D] = [{rows}, D] (got {tuple(shape)})")
    D = int(shape[1])
    if not 1 <= D <= max_d:
        raise RuntimeError(f"{what}: need 1 <= D <= {max_d} (got D={D}{d_note})")
    if D > 1 and stride[1] != 1:
        raise RuntimeError(f"{what}: feat rows must be contiguous (stride(1) == 1, got strides {stride})")
    ld = int(stride[0]) if rows > 1 else max(int(stride[0]), D)
    if ld < D:
        raise RuntimeError(f"{what}: feat rows overlap (stride(0) = {ld} < D = {D})")
    return ld, D


def _caller_err(what: str, err) -> None:
    if err is not None and (not isinstance(err, Tensor) or err.dtype != torch.int32 or err.numel() != 1):
        raise RuntimeError(f"{what}: err must be an int32 tensor of one element (ops.new_err_flag)")


def segment_diverse(feat: Tensor, pool: Tensor, n_objects: int, n_candidates: int, keep: int, err: Optional[Tensor] = None):
    """Greedy farthest-point order inside each object's quality pool (dvq_segment_diverse; the definition is in include/dvq.h).
    feat fp32 [O*M, D] with ``stride(1) == 1`` and any ``stride(0) >= D`` (a column slice or ``vertices.view(B, -1)`` is read in
    place); pool int64 [O,P] contiguous: distinct candidate indices in rank order (``segment_topk(..., keep=P)``) -> ``(sel int64,
    rank int32, gap f32)``, each [O,keep]: candidate index, pool position and squared distance to the nearest earlier pick (-1 for
    pick 0 and for rows that are not finite).  A pool entry outside [0, M) raises RuntimeError unless an ``err`` flag tensor is
    supplied (then the caller checks it; that object's outputs are -1)."""
    if not isinstance(feat, Tensor) or not isinstance(pool, Tensor):
        raise RuntimeError("segment_diverse: feat and pool must be tensors")
    O, M, keep = int(n_objects), int(n_candidates), int(keep)
    _f32(feat, "segment_diverse: feat"), _i64(pool, "segment_diverse: pool")
    if pool.dim() != 2 or pool.shape[0] != O or not pool.is_contiguous():
        raise RuntimeError(f"segment_diverse: pool must be a contiguous int64 [O,P] with O={O} (got {tuple(pool.shape)})")
    P = int(pool.shape[1])
    if O < 0 or not 1 <= keep <= P <= M <= SEGMENT_DIVERSE_MAX_D:
        raise RuntimeError(f"segment_diverse: need O >= 0 and 1 <= keep <= P <= M <= {SEGMENT_DIVERSE_MAX_D} (got O={O} M={M} P={P} keep={keep})")
    ld, D = _segment_feat("segment_diverse", feat, O * M, SEGMENT_DIVERSE_MAX_D)
    _caller_err("segment_diverse", err)
    dev = _require_gpu(feat, pool, err)
    lib = _lib.load()
    outs = _outputs(O, dev, (_L, keep), (_I, keep), (_F, keep))                        # sel, rank, gap
    with _err_flag(err, dev, f"segment_diverse: pool entry out of bounds for {M} candidates") as flag, torch.cuda.device(dev):
        check(lib.dvq_segment_diverse(feat.data_ptr(), ld, D, pool.data_ptr(), O, M, P, keep, *map(_ptr, outs), flag.data_ptr(),
                                      _stream(dev)), "dvq_segment_diverse")
    return outs


SEGMENT_KMEANS_MAX_M = 262144      # csrc/kmeans.hip: KM_MAX_M
SEGMENT_KMEANS_MAX_K = 64          # csrc/kmeans.hip: KM_MAX_K
SEGMENT_KMEANS_MAX_D = 64          # csrc/kmeans.hip: KM_MAX_D


def segment_kmeans(feat: Tensor, init: Tensor, n_objects: int, n_rows: int, iters: int, err: Optional[Tensor] = None):
    """Lloyd's k-means inside each segment of ``n_rows`` rows (dvq_segment_kmeans; the definition is in include/dvq.h): ONE
    deterministic run from the starting rows ``init``, one workgroup per segment, one launch.  feat fp32 [O*M, D] with
    ``stride(1) == 1`` and any ``stride(0) >= D`` (a column slice is read in place), D <= 64 (vertex space is out of scope);
    init int64 [O,k] contiguous: distinct positions of valid rows inside each segment, k <= 64 -> ``(centres f32 [O,k,D], counts
    int32 [O,k], assign int32 [O*M], dist f32 [O*M], iters_used int32 [O])``; rows that are not finite get assign -1 and dist NaN.
    A bad ``init`` (out of range, a duplicate, a row that is not finite) raises RuntimeError unless an ``err`` flag tensor is
    supplied (then the caller checks it; that segment's outputs are -1 / NaN)."""
    if not isinstance(feat, Tensor) or not isinstance(init, Tensor):
        raise RuntimeError("segment_kmeans: feat and init must be tensors")
    O, M, iters = int(n_objects), int(n_rows), int(iters)
    _f32(feat, "segment_kmeans: feat"), _i64(init, "segment_kmeans: init")
    if init.dim() != 2 or init.shape[0] != O or not init.is_contiguous():
        raise RuntimeError(f"segment_kmeans: init must be a contiguous int64 [O,k] with O={O} (got {tuple(init.shape)})")
    k = int(init.shape[1])
    if O < 0 or iters < 0 or not 1 <= k <= SEGMENT_KMEANS_MAX_K or not k <= M <= SEGMENT_KMEANS_MAX_M:
        raise RuntimeError(f"segment_kmeans: need O >= 0, iters >= 0, 1 <= k <= {SEGMENT_KMEANS_MAX_K} and k <= M <= {SEGMENT_KMEANS_MAX_M} "
                           f"(got O={O} M={M} k={k} iters={iters})")
    ld, D = _segment_feat("segment_kmeans", feat, O * M, SEGMENT_KMEANS_MAX_D, "; vertex space is out of scope")
    _caller_err("segment_kmeans", err)
    dev = _require_gpu(feat, init, err)
    lib = _lib.load()
    centres, counts = _outputs(O, dev, (_F, k, D), (_I, k))
    assign, dist = _outputs(O * M, dev, (_I,), (_F,))
    used, = _outputs(O, dev, (_I,))
    message = f"segment_kmeans: init entry out of bounds for {M} rows, repeated, or the position of a row that is not finite"
    with _err_flag(err, dev, message) as flag, torch.cuda.device(dev):
        check(lib.dvq_segment_kmeans(feat.data_ptr(), ld, D, init.data_ptr(), O, M, k, iters, centres.data_ptr(), counts.data_ptr(),
                                     assign.data_ptr(), dist.data_ptr(), used.data_ptr(), flag.data_ptr(), _stream(dev)),
              "dvq_segment_kmeans")
    return centres, counts, assign, dist, used


SEGMENT_CONTACT_TILE = 1024        # csrc/segment_contact.hip: SC_TILE (the object points one workgroup holds still)
SEGMENT_CONTACT_MAX_K = 262144     # csrc/segment_contact.hip: SC_MAX_K (rows per segment)


def segment_contact(hand: Tensor, faces: Tensor, vf_off: Tensor, vf_face: Tensor, obj: Tensor, n_objects: int, n_rows: int,
                    rows: Optional[Tensor] = None, contact_threshold: float = 0.02 ** 2, err: Optional[Tensor] = None):
    """Contact from the object's side in one fused kernel (dvq_segment_contact; the definition is in include/dvq.h): per object point,
    over the ``n_rows`` = K grasps of each of the ``n_objects`` = O segments, ``(touch [O,N] i32, inside [O,N] i32, dmin [O,N] f32,
    near_sum [O,N] f32, n_valid [O] i32, row_status [O*K] i32)``: how many valid rows come closer than ``contact_threshold`` (a squared
    distance), how many have the point inside the hand, the smallest squared distance (+inf without a valid row), the summed distances
    of the touching rows in the fixed four-chain order, the valid rows, and 1 for a row with a non-finite coordinate.  hand, the
    topology and obj [B,N,3] (any strides, read in place) as ``grasp_scores`` takes them; segment o is the rows ``rows[o*K:(o+1)*K]``
    of them (int64 [O*K] contiguous on the device: a gather by index, nothing is copied), or with ``rows=None`` rows o*K .. o*K+K-1,
    and then B must be O*K.  Per row and point the bits of ``grasp_scores``.  An entry of ``rows`` outside [0, B) raises RuntimeError
    unless an ``err`` flag tensor is supplied (then the caller checks it; that segment's outputs are -1 / NaN)."""
    po, ob, op, oc, B, V, N = _hand_cloud_args("segment_contact", hand, faces, vf_off, vf_face, obj)
    O, K = int(n_objects), int(n_rows)
    if O < 0 or not 1 <= K <= SEGMENT_CONTACT_MAX_K:
        raise RuntimeError(f"segment_contact: need O >= 0 and 1 <= K <= {SEGMENT_CONTACT_MAX_K} (got O={O} K={K})")
    if rows is None:
        if B != O * K:
            raise RuntimeError(f"segment_contact: without rows the batch must hold O * K = {O * K} rows (got B={B})")
    elif not isinstance(rows, Tensor) or _i64(rows, "segment_contact: rows").shape != (O * K,) or not rows.is_contiguous():
        raise RuntimeError(f"segment_contact: rows must be a contiguous int64 [O*K] = [{O * K}] tensor")
    contact_threshold = _positive("segment_contact", "contact_threshold", contact_threshold)
    _caller_err("segment_contact", err)
    dev = _require_gpu(hand, obj, faces, vf_off, vf_face, rows, err)
    lib = _lib.load()
    maps = _outputs(O, dev, (_I, N), (_I, N), (_F, N), (_F, N), (_I,))                # touch, inside, dmin, near_sum, n_valid
    status, = _outputs(O * K, dev, (_I,))
    with _err_flag(err, dev, f"segment_contact: rows entry out of bounds for {B} rows") as flag, torch.cuda.device(dev):
        check(lib.dvq_segment_contact(hand.data_ptr(), faces.data_ptr(), vf_off.data_ptr(), vf_face.data_ptr(), V, po, ob, op, oc, B, N,
                                      _ptr(rows), O, K, contact_threshold, *map(_ptr, maps), status.data_ptr(), flag.data_ptr(),
                                      _stream(dev)), "dvq_segment_contact")
    return maps + (status,)


MESH_SAMPLE_MAX_S = 1 << 20        # include/dvq.h: DVQ_MESH_SAMPLE_MAX_S, samples per object and call
MESH_SAMPLE_CHUNK = 1024           # csrc/mesh_sample.hip: MS_T (the faces per chunk of the prefix sum)
CLOUD_FPS_MAX_P = 16384            # include/dvq.h: DVQ_CLOUD_FPS_MAX_P (the pool sits in the registers of one workgroup)


def mesh_sample(verts: Tensor, vert_off: Tensor, faces: Tensor, face_off: Tensor, n_samples: int, seed: int, stream_ids: Tensor,
                err: Optional[Tensor] = None):
    """Area-weighted random points on each object's triangle mesh (dvq_mesh_sample; the definition is in include/dvq.h): ``(points
    [O,S,3] f32, face [O,S] i32, status [O] i32, cdf [n_mf] int64)``.  verts [n,3] f32, vert_off int32 [O+1], faces [m,3] int32 (indices
    local to the object's vertices) and face_off int32 [O+1] (``contact.ObjectMeshes``); ``n_samples`` = S per object; stream_ids int64
    [O]: every object's GLOBAL index, which with ``seed`` and the sample index fixes a draw whatever shares the call.  ``face`` is the
    LOCAL face a point lies on; status 0 fine, 1 no face with area (points NaN, face -1), 4 a range out of bounds; ``cdf`` holds the
    inclusive sums of the integer face weights (the bits of the ABI's uint64).  A face index or an object's range out of bounds (bit 1)
    or a stream id outside [0, 2^32) (bit 0) raises RuntimeError unless an ``err`` flag tensor is supplied (then the caller checks it)."""
    what = "mesh_sample"
    _tensors(what, "verts vert_off faces face_off stream_ids", verts, vert_off, faces, face_off, stream_ids)
    _f32(verts, "mesh_sample: verts")
    _int32_tables(what, "vert_off faces face_off", vert_off, faces, face_off)
    O = _mesh_tables(what, verts, vert_off, faces, face_off)
    S = int(n_samples)
    if not 1 <= S <= MESH_SAMPLE_MAX_S:
        raise RuntimeError(f"mesh_sample: need 1 <= n_samples <= {MESH_SAMPLE_MAX_S} (got {S})")
    if _i64(stream_ids, "mesh_sample: stream_ids").shape != (O,) or not stream_ids.is_contiguous():
        raise RuntimeError(f"mesh_sample: stream_ids must be a contiguous int64 [O] = [{O}] tensor")
    _caller_err(what, err)
    dev = _require_gpu(verts, vert_off, faces, face_off, stream_ids, err)
    lib = _lib.load()
    points, face, status = _outputs(O, dev, (_F, S, 3), (_I, S), (_I,))
    cdf = torch.zeros(faces.shape[0], dtype=torch.int64, device=dev)       # (an object of status 4 leaves its words unwritten)
    message = lambda bad: ("mesh_sample: a stream id is outside [0, 2^32)" if bad & 1 else
                           "mesh_sample: a face index or an object's vertex / face range is out of bounds")
    with _err_flag(err, dev, message) as flag, torch.cuda.device(dev):
        check(lib.dvq_mesh_sample(verts.data_ptr(), verts.shape[0], vert_off.data_ptr(), faces.data_ptr(), faces.shape[0],
                                  face_off.data_ptr(), O, S, int(seed) & 0xFFFFFFFFFFFFFFFF, stream_ids.data_ptr(), cdf.data_ptr(), points.data_ptr(),
                                  face.data_ptr(), status.data_ptr(), flag.data_ptr(), _stream(dev)), "dvq_mesh_sample")
    return points, face, status, cdf


def cloud_fps(points: Tensor, keep: int):
    """Farthest-point subsampling of 3-D pools (dvq_cloud_fps; the definition is in include/dvq.h): points [O,P,3] f32 contiguous ->
    ``(sel [O,keep] i32, gap [O,keep] f32, status [O] i32)``: the pool positions in greedy k-centre order from position 0, each pick's
    squared distance to the nearest earlier pick (-1 for pick 0), and 1 for a pool with a non-finite coordinate (sel -1, gap -1)."""
    if not isinstance(points, Tensor):
        raise RuntimeError("cloud_fps: points must be a tensor")
    _f32(points, "cloud_fps: points")
    if points.dim() != 3 or points.shape[2] != 3 or not points.is_contiguous():
        raise RuntimeError(f"cloud_fps: points must be contiguous [O,P,3] (got {tuple(points.shape)})")
    O, P, keep = int(points.shape[0]), int(points.shape[1]), int(keep)
    if not 1 <= keep <= P <= CLOUD_FPS_MAX_P:
        raise RuntimeError(f"cloud_fps: need 1 <= keep <= P <= {CLOUD_FPS_MAX_P} (got P={P} keep={keep})")
    dev = _require_gpu(points)
    lib = _lib.load()
    outs = _outputs(O, dev, (_I, keep), (_F, keep), (_I,))                             # sel, gap, status
    with torch.cuda.device(dev):
        check(lib.dvq_cloud_fps(points.data_ptr(), O, P, keep, *map(_ptr, outs), _stream(dev)), "dvq_cloud_fps")
    return outs
