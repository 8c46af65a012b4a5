"""GenNet mirror (reference: network/gen_net.py:13-125): the batched grasp-generation graph.

Batched semantics = B independent B=1 reference calls (the reference's own ``gen`` only works for B=1:
per-sample label instead of ``idx6[:,0,0]`` of sample 0, row-gather lookup instead of ``view(1,dim)``)."""
import os

import torch
import torch.nn as nn

from .. import _lib, ops, packing
from .DVQVAE import Decoder, _codebooks
from .pixelcnn.models import GatedPixelCNN
from .pointnet_encoder import PointNetEncoder

CODE_SLOTS = ((0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2))     # grid position -> vqvae0..5 (gen_net.py:95-100)


def code_grid(part_codes, device=None):
    """Six hand-part codes per grasp [B,6] int64 (column k = vqvae{k}; from DVQVAE.forward's emb_idx [7B,1]:
    ``emb_idx.view(7, B)[1:].t()``) -> the prior's [B,3,3] grid with the codes at CODE_SLOTS and -1 in the context column
    (column 0, which gen() never decodes): as ``codes=`` of GenNet.gen the six parts are kept and the context is drawn; overwrite
    entries with -1 to resample those parts."""
    part_codes = torch.as_tensor(part_codes, dtype=torch.int64, device=device)
    if part_codes.dim() != 2 or part_codes.shape[1] != len(CODE_SLOTS):
        raise RuntimeError(f"code_grid: expected [B,{len(CODE_SLOTS)}] part codes, got {tuple(part_codes.shape)}")
    grid = torch.full((part_codes.shape[0], 3, 3), -1, dtype=torch.int64, device=part_codes.device)
    for k, (i, j) in enumerate(CODE_SLOTS):
        grid[:, i, j] = part_codes[:, k]
    return grid


class GenNet(nn.Module):
    def __init__(self, n_embeddings=128, prior_tokens=512, prior_dim=512, prior_layers=15, prior_classes=128):
        """Defaults are the reference's fixed sizes (gen_net.py:17-34).  ``n_embeddings`` = 512 builds the
        K=512 codebooks of the synthetic benchmark (prior emits 512 classes, checkpoint codebooks 128)."""
        super().__init__()
        self.obj_encoder_type = PointNetEncoder(global_feat=True, feature_transform=False, channel=4)
        self.obj_encoder_pos = PointNetEncoder(global_feat=True, feature_transform=False, channel=4)
        _codebooks(self, n_embeddings)
        self.decoder = Decoder(layer_sizes=[1024, 256, 55], latent_size=2560)
        self.num = 0
        self.rh_mano = None
        self.recon_encoder = PointNetEncoder(global_feat=True, feature_transform=False, channel=3)
        self.pos_decoder = Decoder(layer_sizes=[1024, 128, 6], latent_size=2048)
        self.GatedPixelCNN = GatedPixelCNN(prior_tokens, prior_dim, prior_layers, prior_classes)
        self.noise_seed = None       # key of the device Philox generator that replaces multinomial's draws (set_noise_seed);
        #                              None: torch.initial_seed(), i.e. torch.manual_seed governs the draws as it does the reference's
        self._noise_stream = 0       # one Philox stream per gen() call unless the caller names it
        self.sort_by_label = os.environ.get("DVQ_SORT_LABELS", "1") != "0"   # prior evaluated in label order (gather locality)
        self.range_fallbacks = 0     # gen() calls in which rows were generated again on the bf16 split (an activation left fp16's range)
        self.range_fallback_rows = 0 # ... and how many rows that was

    def set_noise_seed(self, seed, first_stream=0):
        """Seed of the prior's sampling noise; every gen() call without explicit ``noise`` / ``stream_id`` uses the next stream."""
        self.noise_seed = int(seed)
        self._noise_stream = int(first_stream)
        return self

    def set_rh_mano(self, Rh_mano):
        Rh_mano.eval()
        self.rh_mano = Rh_mano

    # ------------------------------------------------------------------------------------------
    def _hand_vertices(self, recon):
        """rh_mano(betas, global_orient=0, hand_pose, transl=0).vertices as [B,3,778] (gen_net.py:116-120)."""
        m = self.rh_mano
        if m is None:
            raise RuntimeError("GenNet.gen: call set_rh_mano(layer) first (gen_diverse_grasp_obman.py:361)")
        if hasattr(m, "vertices_channel_major"):
            return m.vertices_channel_major(recon[:, :10], recon[:, 10:55])
        zero = torch.zeros(recon.shape[0], 3, device=recon.device)
        v = m(betas=recon[:, :10], global_orient=zero, hand_pose=recon[:, 10:55], transl=zero).vertices
        return v.detach().permute(0, 2, 1).contiguous()

    def _decode(self, codes, feat_type, feat_pos_into, err):
        """codes [B,3,3] + object feature -> recon [B,55]; shared by gen and gen_byid."""
        B, dev = codes.shape[0], codes.device
        z_out = feat_type["z_out"]
        flat = codes.view(B, 9)
        for k, (i, j) in enumerate(CODE_SLOTS):
            E = getattr(self, f"vqvae{k}").vector_quantization.embedding.weight.detach()
            ops.vq_lookup(E, flat[:, i * 3 + j], out=z_out[:, 256 * k: 256 * (k + 1)], err=err)
        return self.decoder(z_out).view(B, 55)

    def _noise_key(self, seed, row0, stream_id):
        """(seed, first global row, stream) of the device Philox generator under gen()'s key rules."""
        if stream_id is None:
            stream_id = self._noise_stream
            self._noise_stream += 1
        dseed, drow = ops.default_noise_key()
        if seed is None:
            seed = dseed if self.noise_seed is None else self.noise_seed
        return seed, (drow if row0 is None else row0), stream_id

    def _draw_noise(self, B, dev, key, perm=None):
        """[B, 9, prior_tokens] Exp(1) variates; with ``perm``, row r holds the draws of row perm[r] of the keyed batch."""
        n_in = self.GatedPixelCNN.packed().n_in
        seed, row0, stream_id = key
        return ops.exp1_noise(B, 9 * n_in, seed, row0, stream_id, device=dev, perm=perm).view(B, 9, n_in)

    def _draw_noise_keyed(self, row_keys, seed, err, sel=None):
        """[B, 9, prior_tokens] Exp(1) variates of per-row keys (stream_ids, row_ids); with ``sel``, row r holds the draws of
        key sel[r].  Only the two [B] key arrays are gathered, never the noise."""
        n_in = self.GatedPixelCNN.packed().n_in
        sid, rid = row_keys
        if sel is not None:
            sid, rid = sid.index_select(0, sel), rid.index_select(0, sel)
        return ops.exp1_noise_keyed(sid, rid, 9 * n_in, seed, err=err).view(sid.shape[0], 9, n_in)

    def _gen_impl(self, obj, noise, key=None, rows=None, row_keys=None, ctl=None):
        """The device work of gen(): no host synchronisation inside (gen() checks the error flag once at the end).
        ``noise`` None: the prior's draws come from the device generator under ``key``, drawn directly in the order the prior
        is evaluated in (no gather of the [B, 9, tokens] tensor).  ``rows`` (int64 [B] on the device): ``obj`` holds rows
        ``rows`` of the keyed batch -- sample b draws the noise of row ``rows[b]`` (the per-row range fallback of gen()).
        ``row_keys`` (two int64 [B0] tensors on the device, ``key`` = the seed): per-row keys instead of one stream per call --
        sample b draws the noise of (seed, stream_ids[b], row_ids[b]), or of entry ``rows[b]`` of the two arrays under ``rows``.
        ``ctl`` = (temperature, top_k, given [B,9] or None): the controlled draw (ops.pixelcnn_sample) with the log-probabilities in
        ``aux``; ``given`` holds the rows of ``obj``.  None: the plain draw, the launches of every call before the controls."""
        if obj.dim() != 3:
            raise RuntimeError(f"gen: expected obj [B,4,N], got {tuple(obj.shape)}")
        B, dev = obj.shape[0], obj.device
        obj = obj.contiguous()
        z_out = torch.empty(B, 2560, device=dev, dtype=torch.float32)      # [emb0..5 | obj_type_feature] (:109)
        z_pos = torch.empty(B, 2048, device=dev, dtype=torch.float32)      # [hand_feat | obj_pos_feature]  (:121)
        self.obj_encoder_type(obj, out=z_out[:, 1536:])                    # :81 written in place
        self.obj_encoder_pos(obj, out=z_pos[:, 1024:])                     # :82
        feat_type = z_out[:, 1536:]
        idx6, _ = self.vqvae6.inference(feat_type)                         # :83 (obj_emb unused, as in the reference)
        label = idx6[:, 0].contiguous()                                    # per-sample label
        err = ops.new_err_flag(dev)
        pk = self.GatedPixelCNN.packed()
        logp = None

        def draw(lab, q, given):
            if ctl is None:
                return ops.pixelcnn_sample(pk, lab, q, err=err), None                      # :92
            c, lm, ld = ops.pixelcnn_sample(pk, lab, q, err=err, temperature=ctl[0], top_k=ctl[1], given=given, return_logp=True)
            return c, (lm, ld)
        given = None if ctl is None else ctl[2]
        # The gated GEMMs add the class-conditional row cls[label[m]] in their epilogue: with rows in arrival order every lane of a
        # store instruction gathers from a different 4 KB row of the table; sorted by label a 128-row tile holds one or two labels
        # and the gather is a broadcast again (measured: -10 % on the gated GEMMs at 65 536 grasps with 123 distinct object codes).
        # Rows are independent, so the order changes no result; the codes are scattered back.
        if B >= 512 and self.sort_by_label:
            order = torch.argsort(label, stable=True)
            if noise is not None:
                noise_s = noise.index_select(0, order)
            elif row_keys is not None:
                noise_s = self._draw_noise_keyed(row_keys, key, err, sel=order if rows is None else rows.index_select(0, order))
            else:
                noise_s = self._draw_noise(B, dev, key, perm=order if rows is None else rows[order].contiguous())
            codes_s, logp_s = draw(label[order].contiguous(), noise_s, None if given is None else given.index_select(0, order))
            codes = torch.empty_like(codes_s)
            codes[order] = codes_s
            if logp_s is not None:                                         # the log-probabilities travel with their rows
                logp = tuple(torch.empty_like(t) for t in logp_s)
                for dst, src in zip(logp, logp_s):
                    dst[order] = src
        else:
            if noise is None:
                noise = (self._draw_noise_keyed(row_keys, key, err, sel=rows) if row_keys is not None
                         else self._draw_noise(B, dev, key, perm=rows))
            codes, logp = draw(label, noise.contiguous(), given)
        # a position drawn from all-NaN logits carries -1 (bit 2 of err is set; gen() regenerates those rows): decode token 0 there
        recon = self._decode(codes.clamp_min(0), {"z_out": z_out}, None, err)   # :95-113
        verts = self._hand_vertices(recon)                                 # :116-118
        self.recon_encoder(verts, out=z_pos[:, :1024])                     # :120
        recon_pos = self.pos_decoder(z_pos).view(B, 6)                     # :122-123
        aux = dict(idx6=idx6, codes=codes, feat_type=feat_type, feat_pos=z_pos[:, 1024:], verts=verts, hand_feat=z_pos[:, :1024])
        if logp is not None:
            aux["logp_model"], aux["logp_draw"] = logp
        return recon, recon_pos, aux, err

    _RANGE_ERROR = ("GenNet.gen: code or label index out of range (prior classes vs codebook rows, "
                    "gen_net.py:20-34); build GenNet(n_embeddings=...) to match the prior")

    @torch.no_grad()
    def gen(self, obj, noise=None, return_aux=False, seed=None, row0=None, stream_id=None, check=True, row_keys=None,
            temperature=1.0, top_k=0, codes=None, log_prob=False):
        """obj [B,4,N] f32 on the GPU -> (recon [B,55], recon_pos [B,6]).
        ``noise`` [B,9,prior_tokens] ~ Exp(1) fixes the prior's draws (parity runs).  Without it the draws come from the
        device Philox generator keyed by (seed, stream_id, row0 + b): a batch sharded over ranks (``row0`` = first global
        row of the shard, same ``seed`` / ``stream_id``) generates exactly what the unsharded call generates.
        Defaults: seed = set_noise_seed's, else torch.initial_seed(); one stream per call; rows of this rank
        (ops.default_noise_key), so ranks that name nothing never share noise.
        ``row_keys`` = (stream_ids, row_ids), two int64 [B] tensors on the device: sample b draws the noise of
        (seed, stream_ids[b], row_ids[b]) -- a call that mixes the grasps of many objects (stream = object, row = grasp index)
        generates for each grasp the bits its own per-object call generates.  Excludes ``noise`` / ``row0`` / ``stream_id`` and
        leaves the per-call stream counter alone.
        ``check=False``: no host synchronisation at all -- the call returns as soon as the work is enqueued (a loop of B = 1 calls
        then overlaps the host side of call i + 1 with the device side of call i); the caller gives up the index-range error
        and the fp16-range fallback below, and gets ``aux["err"]`` (device int32: bit 0 range, bit 2 all-NaN logits) to check later.
        Controls on the prior's draw: ``temperature`` > 0 divides the logits (below 1: likelier, less diverse
        grasps), ``top_k`` > 0 draws from the top_k likeliest codes of each position, ``codes`` int64 [B,3,3] / [B,9] fixes the
        grid positions whose entry is >= 0 and draws the rest (code_grid builds one from six part codes).  With any of them, or
        ``log_prob=True``, ``aux`` gains ``logp_model`` and ``logp_draw`` [B,9]: each position's log-probability under the
        untempered prior and under the distribution it was drawn from; a grasp's prior log-likelihood is ``logp_model.sum(1)``.
        Keys, sharding, ``row_keys``, ``check=False`` and the range fallback work as without them; at the defaults the call runs
        the launches it always ran."""
        if obj.dim() != 3:
            raise RuntimeError(f"gen: expected obj [B,4,N], got {tuple(obj.shape)}")
        ctl = None
        if float(temperature) != 1.0 or top_k != 0 or codes is not None or log_prob:
            if codes is not None:
                if (not torch.is_tensor(codes) or codes.dtype != torch.int64 or codes.device != obj.device
                        or tuple(codes.shape) not in ((obj.shape[0], 9), (obj.shape[0], 3, 3))):
                    raise RuntimeError("gen: codes must be an int64 [B,3,3] or [B,9] tensor on obj's device")
                codes = codes.reshape(obj.shape[0], 9).contiguous()
            ctl = (temperature, top_k, codes)
        if row_keys is not None:
            if noise is not None or row0 is not None or stream_id is not None:
                raise RuntimeError("gen: row_keys names every row's noise key itself; it excludes noise / row0 / stream_id")
            sid, rid = row_keys
            for k, name in ((sid, "stream_ids"), (rid, "row_ids")):
                if (not torch.is_tensor(k) or k.dtype != torch.int64 or tuple(k.shape) != (obj.shape[0],) or k.device != obj.device
                        or not k.is_contiguous()):
                    raise RuntimeError(f"gen: row_keys {name} must be a contiguous int64 [B] tensor on obj's device")
            row_keys = (sid, rid)
            if seed is None:
                seed = ops.default_noise_key()[0] if self.noise_seed is None else self.noise_seed
            key = seed                                                     # the streams and rows come from row_keys
        else:
            key = self._noise_key(seed, row0, stream_id) if noise is None else None
        with ops.no_range_check():                                         # ONE check for the whole path, below
            recon, recon_pos, aux, err = self._gen_impl(obj, noise, key, row_keys=row_keys, ctl=ctl)
        aux["err"] = err
        if not check:
            return (recon, recon_pos, aux) if return_aux else (recon, recon_pos)
        # one host synchronisation per call: the index-range flag and "every parameter is finite"
        finite = torch.isfinite(recon).all() & torch.isfinite(recon_pos).all()
        if ctl is not None:                # a given code is never -1: NaN logits at its position show in its log-probability alone
            finite = finite & torch.isfinite(aux["logp_model"]).all()
        status = int((err + 2 * (~finite).to(torch.int32)).item())
        if status & 1:
            raise RuntimeError(self._RANGE_ERROR + ("" if row_keys is None else
                                                    "; or a row key outside the noise generator's counter (stream id in [0, 2^32), row id >= 0)"))
        if (status & 6) and packing.gemm_kind() == _lib.PLANES_F16X2:     # non-finite parameters, or a draw from all-NaN logits (bit 2)
            # The default GEMM arithmetic splits activations into fp16 pieces: a value beyond fp16's range (|x| >= 65 520) turns its
            # ROW into NaN -- never a silently wrong number (rows do not interact anywhere on the path).  Exactly those rows -- a
            # non-finite parameter, or a -1 where the sampler drew from all-NaN logits -- are generated again on the six-product bf16
            # split, which has fp32's range (csrc/gemm_f16x2.hip), under the same noise keys, and scattered back; every other row keeps
            # its bits.  NaN / Inf INPUTS come out non-finite there too, as in the reference.
            bad = ~(torch.isfinite(recon).all(dim=1) & torch.isfinite(recon_pos).all(dim=1)) | (aux["codes"].reshape(obj.shape[0], -1) < 0).any(dim=1)
            if ctl is not None:
                bad = bad | ~torch.isfinite(aux["logp_model"]).all(dim=1)
            rows = bad.nonzero().reshape(-1)
            self.range_fallbacks += 1
            self.range_fallback_rows += int(rows.numel())
            with ops.no_range_check(), packing.gemm_kind_as(_lib.PLANES_BF16X3):
                ctl2 = ctl if ctl is None or ctl[2] is None else (ctl[0], ctl[1], ctl[2].index_select(0, rows))
                r2, p2, aux2, err2 = self._gen_impl(obj.index_select(0, rows), None if noise is None else noise.index_select(0, rows), key, rows=rows,
                                                    row_keys=row_keys, ctl=ctl2)
                if int(err2.item()) & 1:
                    raise RuntimeError(self._RANGE_ERROR)
            recon[rows], recon_pos[rows] = r2, p2
            for k in ("idx6", "codes", "feat_type", "feat_pos", "verts", "hand_feat") + (() if ctl is None else ("logp_model", "logp_draw")):
                aux[k][rows] = aux2[k]
            aux["err"] = err2
            aux["fallback_rows"] = rows
        return (recon, recon_pos, aux) if return_aux else (recon, recon_pos)

    @staticmethod
    def beam_duplicates(codes, n_live):
        """codes [S,W,3,3] / [S,W,9] int64, n_live [S] -> int64 [S,W]: the rank of the first better beam of the same cloud with the
        same six CODE_SLOTS codes (the hand decodes from those alone: such a beam is the same grasp), or -1."""
        S, W = codes.shape[:2]
        six = codes.reshape(S, W, 9)[:, :, [i * 3 + j for i, j in CODE_SLOTS]]
        rank = torch.arange(W, device=codes.device)
        live = rank[None, :] < n_live[:, None].to(torch.int64)
        same = (six[:, :, None, :] == six[:, None, :, :]).all(dim=-1) & (rank[None, :] < rank[:, None])[None] & live[:, None, :] & live[:, :, None]
        first = torch.where(same, rank[None, None, :], torch.full_like(rank, W)[None, None, :]).min(dim=2).values
        return torch.where(first < W, first, torch.full_like(first, -1))

    @torch.no_grad()
    def gen_beam(self, obj, width, return_aux=False):
        """obj [S,4,N] f32 on the GPU -> (recon [S*W,55], recon_pos [S*W,6]): row s * W + r is the grasp decoded from the r-th
        likeliest code grid of cloud s under the prior (ops.pixelcnn_beam) -- no noise, nothing drawn.  Both object
        encoders and the object codebook run once per cloud; their features are repeated into the W rows, and the decode, MANO,
        recon_encoder and pos_decoder are gen()'s launches on S * W rows: the result equals
        ``gen(obj.repeat_interleave(W, 0), codes=aux["codes"])`` bit for bit.
        ``aux``: ``codes`` [S*W,3,3], ``log_prob`` [S*W] (the beam's score: its nine log-probabilities summed in float32),
        ``n_live`` [S] int32, ``duplicate_of`` [S,W] (beam_duplicates; beams are distinct on nine tokens, the hand uses six),
        ``idx6`` [S,1], ``verts`` [S*W,3,778].  Rows beyond a cloud's n_live (fewer than W grids exist) come out NaN.
        Rows whose parameters are not finite (fp16 range in the decoders) are generated again by ``gen(codes=...)``, which has the
        bf16 fallback; the SEARCH has none: a cloud whose logits held a NaN raises."""
        if obj.dim() != 3:
            raise RuntimeError(f"gen_beam: expected obj [S,4,N], got {tuple(obj.shape)}")
        if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= ops.PIXELCNN_BEAM_MAX_W:
            raise RuntimeError(f"gen_beam: width must be an integer in 1 .. {ops.PIXELCNN_BEAM_MAX_W}, got {width!r}")
        S, W, dev = obj.shape[0], width, obj.device
        B = S * W
        obj = obj.contiguous()
        with ops.no_range_check():
            z1 = torch.empty(S, 2560, device=dev, dtype=torch.float32)
            p1 = torch.empty(S, 2048, device=dev, dtype=torch.float32)
            self.obj_encoder_type(obj, out=z1[:, 1536:])
            self.obj_encoder_pos(obj, out=p1[:, 1024:])
            idx6, _ = self.vqvae6.inference(z1[:, 1536:])
            label = idx6[:, 0].contiguous()
            err = ops.new_err_flag(dev)
            codes, score, n_live = ops.pixelcnn_beam(self.GatedPixelCNN.packed(), label, W, err=err)
            z_out = torch.empty(B, 2560, device=dev, dtype=torch.float32)
            z_pos = torch.empty(B, 2048, device=dev, dtype=torch.float32)
            z_out.view(S, W, 2560)[:, :, 1536:] = z1[:, None, 1536:]
            z_pos.view(S, W, 2048)[:, :, 1024:] = p1[:, None, 1024:]
            codes = codes.view(B, 3, 3)
            recon = self._decode(codes.clamp_min(0), {"z_out": z_out}, None, err)
            verts = self._hand_vertices(recon)
            self.recon_encoder(verts, out=z_pos[:, :1024])
            recon_pos = self.pos_decoder(z_pos).view(B, 6)
        status = int(err.item())
        if status & 1:
            raise RuntimeError(self._RANGE_ERROR)
        if status & 4:
            raise RuntimeError(f"GenNet.gen_beam: NaN logits in the search of clouds {(n_live == 0).nonzero().reshape(-1).tolist()} "
                               "(an activation beyond fp16's range); the beam search has no bf16 fallback")
        live = (torch.arange(W, device=dev)[None, :] < n_live[:, None]).reshape(B)
        bad = live & ~(torch.isfinite(recon).all(dim=1) & torch.isfinite(recon_pos).all(dim=1))
        rows = bad.nonzero().reshape(-1)
        if rows.numel():
            self.range_fallbacks += 1
            self.range_fallback_rows += int(rows.numel())
            r2, p2, aux2 = self.gen(obj.index_select(0, rows // W), codes=codes.index_select(0, rows), return_aux=True)
            recon[rows], recon_pos[rows], verts[rows] = r2, p2, aux2["verts"]
        dead = ~live
        recon[dead], recon_pos[dead], verts[dead] = float("nan"), float("nan"), float("nan")
        if not return_aux:
            return recon, recon_pos
        aux = dict(codes=codes, log_prob=score.view(B), n_live=n_live, duplicate_of=self.beam_duplicates(codes.view(S, W, 9), n_live),
                   idx6=idx6, verts=verts, err=err)
        return recon, recon_pos, aux

    @torch.no_grad()
    def gen_byid(self, idx6, noise=None):
        """Debug variant (gen_net.py:41-75): samples codes for a given object code, then decodes an all-zero
        latent (as the reference does) and returns zero wrist parameters."""
        idx6 = idx6.reshape(-1).contiguous()
        B, dev = idx6.shape[0], idx6.device
        self.vqvae6.get_embbeding(idx6, 1024)                              # range check, value unused (:45)
        self.GatedPixelCNN.generate(None, idx6, shape=(3, 3), batch_size=B, noise=noise)
        recon = self.decoder(torch.zeros(B, 2560, device=dev)).view(B, 55)
        return recon, torch.zeros(B, 6, device=dev)

