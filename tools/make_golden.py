#!/usr/bin/env python3
"""Generate tests/golden/*.npz by IMPORTING the real reference from /root/reference.

Runs only in the build container (the reference does not exist on the GPU box and never travels).
Nothing from the reference is copied: the reference modules are imported, loaded with the
deterministic synthetic weights of ``dvqvae_amd.synth`` and executed on CPU; only inputs (when
small), seeds and outputs are written.  Shims applied to make the reference's CPU forward run at
all:

  (1) ``network.vqvae.quantizer.device = cpu``            (quantizer.py:7 hard-codes cuda)
  (2) ``Tensor.to('cuda') -> cpu``                         (gen_net.py:79-116 literals)
  (3) ``network.DVQVAE.f0hand = <83 thumb vertices>``      (DVQVAE.py:93 uses an undefined name)
  (4) prior restricted to the codebook range: ``output_conv.2.bias[128:] = -1e4``
  (5) stand-in MANO layer = oracle/mano_oracle.ManoOracle on the synthetic MANO-shaped model
  (6) ``Tensor.multinomial`` replaced by the exponential race ``argmax(p / q)`` with recorded q;
      the equivalence with the real ``multinomial(1)`` under a replayed generator is asserted first.

The one data file taken over from the reference is its MANO model, for the pickle readers' test (g9_mano_pkl: trimmed to
fit the size limit of a committed file).

Usage:  python tools/make_golden.py            (writes tests/golden/)
        python tools/make_golden.py mano       (only tests/golden/g9_mano_right.pkl.xz)
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import dvqvae_amd  # noqa: E402  (alias of d-vqvae_amd/)
from dvqvae_amd import synth  # noqa: E402
from oracle import mano_oracle  # noqa: E402

torch.set_num_threads(8)
OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)
SEED = 1234

# ---- shims -------------------------------------------------------------------------------------
import network.vqvae.quantizer as ref_quant  # noqa: E402

ref_quant.device = torch.device("cpu")                                   # (1)
_orig_to = torch.Tensor.to


def _to_cpu(self, *a, **k):                                              # (2)
    a = tuple("cpu" if (isinstance(x, str) and x.startswith("cuda")) else x for x in a)
    if isinstance(k.get("device"), str) and k["device"].startswith("cuda"):
        k["device"] = "cpu"
    return _orig_to(self, *a, **k)


torch.Tensor.to = _to_cpu

import network.DVQVAE as ref_dvq  # noqa: E402
from network.gen_net import GenNet as RefGenNet  # noqa: E402
from network.pointnet_encoder import PointNetEncoder as RefPointNet  # noqa: E402
from network.VQVAE import VQVAE as RefVQVAE  # noqa: E402
from network.pixelcnn.models import GatedPixelCNN as RefPixelCNN  # noqa: E402

THUMB = [240] + list(range(248, 254)) + [266, 267, 286, 287] + list(range(697, 769))
ref_dvq.f0hand = THUMB                                                   # (3)


class RaceSampler:
    """(6) deterministic stand-in for Tensor.multinomial(1): argmax(p / q) with recorded q."""

    def __init__(self):
        self.q = None
        self.pos = 0

    def arm(self, q):
        self.q, self.pos = q, 0

    def __call__(self, probs, num_samples, *a, **k):
        assert num_samples == 1
        q = self.q[:, self.pos]
        self.pos += 1
        return torch.argmax(probs / q, dim=-1, keepdim=True)


def check_multinomial_equivalence():
    p = torch.softmax(torch.randn(5, 512, generator=torch.Generator().manual_seed(3)), -1)
    torch.manual_seed(77)
    a = p.multinomial(1).squeeze(1)
    torch.manual_seed(77)
    q = torch.empty_like(p).exponential_(1)
    b = torch.argmax(p / q, dim=-1)
    assert torch.equal(a, b), "multinomial(1) != exponential race on this torch build"


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrs.items()})
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def load_synth(module, seed=SEED, prefix=""):
    sd = synth.synthetic_state_dict(module.state_dict(), seed)
    module.load_state_dict(sd, strict=True)
    module.eval()
    return sd


# ---- G1: PointNetEncoder -------------------------------------------------------------------------
def g1_pointnet():
    out = {}
    for C, N, B in [(4, 64, 4), (4, 1024, 1), (4, 1024, 4), (4, 3000, 1), (3, 778, 4), (3, 100, 2)]:
        net = RefPointNet(global_feat=True, feature_transform=False, channel=C)
        load_synth(net, SEED + C)
        x = synth.synthetic_clouds(B, N, seed=100 + N, channels=C)
        with torch.no_grad():
            feat, trans, _ = net(x)
        tag = f"C{C}_N{N}_B{B}"
        out[tag + "_feat"], out[tag + "_trans"] = feat, trans
        if N <= 100:
            out[tag + "_x"] = x
    save("g1_pointnet", **out)


# ---- G2/G3: VectorQuantizer / VQVAE ----------------------------------------------------------------
def g2_vq():
    out = {}
    for K, D in [(128, 256), (128, 1024), (512, 256)]:
        vq = RefVQVAE(128, 32, 2, K, D, 0.25, a=1)
        E = synth.synthetic_normal((K, D), SEED, f"vq/E/{K}/{D}")
        vq.vector_quantization.embedding.weight.data.copy_(E)
        vq.eval()
        for M in (1, 7, 4096):
            z = synth.synthetic_normal((M, D), SEED, f"vq/z/{K}/{D}/{M}")
            with torch.no_grad():
                idx, zq = vq.inference(z)
                d64 = ((z.double()[:, None, :] - E.double()[None]) ** 2).sum(-1) if M <= 7 else \
                    (z.double() ** 2).sum(1, keepdim=True) + (E.double() ** 2).sum(1) - 2 * z.double() @ E.double().t()
            top2 = torch.topk(d64, 2, dim=1, largest=False)[0]
            tag = f"K{K}_D{D}_M{M}"
            out[tag + "_idx"] = idx.squeeze(1).to(torch.int32)
            out[tag + "_gap"] = (top2[:, 1] - top2[:, 0]).float()
            out[tag + "_zq_rowsum"] = zq.double().sum(1).float()
            assert torch.equal(zq, E[idx.squeeze(1)])
        # reference-init regime (quantizer.py:27): E ~ U(+-1/K): tie-prone, gaps tiny
        Eu = synth.synthetic_uniform((K, D), SEED, f"vq/Eu/{K}/{D}", -1.0 / K, 1.0 / K)
        vq.vector_quantization.embedding.weight.data.copy_(Eu)
        z = synth.synthetic_normal((512, D), SEED, f"vq/zu/{K}/{D}")
        with torch.no_grad():
            idx, _ = vq.inference(z)
            d64 = (z.double() ** 2).sum(1, keepdim=True) + (Eu.double() ** 2).sum(1) - 2 * z.double() @ Eu.double().t()
        top2 = torch.topk(d64, 2, dim=1, largest=False)[0]
        out[f"K{K}_D{D}_uinit_idx"] = idx.squeeze(1).to(torch.int32)
        out[f"K{K}_D{D}_uinit_gap"] = (top2[:, 1] - top2[:, 0]).float()
    # crafted rows: duplicated codebook rows (exact tie -> lowest index), NaN row, Inf row
    K, D = 128, 256
    vq = RefVQVAE(128, 32, 2, K, D, 0.25, a=1)
    E = synth.synthetic_normal((K, D), SEED, "vq/E/crafted")
    E[77] = E[5]
    E[100] = E[5]
    z = synth.synthetic_normal((6, D), SEED, "vq/z/crafted")
    z[0] = E[5]                     # exact tie between rows 5, 77, 100 -> 5
    z[1] = E[77] * 1.0              # same
    z[2, 3] = float("nan")          # NaN row -> every distance NaN -> index 0
    z[3, 9] = float("inf")          # Inf row -> inf - inf = NaN everywhere -> index 0
    z[4] = 0.0
    vq.vector_quantization.embedding.weight.data.copy_(E)
    with torch.no_grad():
        idx, _ = vq.inference(z)
    out["crafted_idx"] = idx.squeeze(1).to(torch.int32)
    out["crafted_z"], out["crafted_E"] = z, E
    # G3: train-mode forward (loss, perplexity)
    vq.train()
    zt = synth.synthetic_normal((64, D), SEED, "vq/z/train")
    with torch.no_grad():
        loss, zq, perp = vq(zt)
    out["train_loss"], out["train_perplexity"], out["train_zq_rowsum"] = loss, perp, zq.double().sum(1).float()
    save("g2_vq", **out)


# ---- G4/G5: GatedPixelCNN ---------------------------------------------------------------------------
def g4_pixelcnn(sampler):
    out = {}
    # reduced net (weights regenerated from the seed in tests)
    small = RefPixelCNN(input_dim=32, dim=64, n_layers=3, n_classes=16)
    load_synth(small, SEED + 1)
    g = np.random.Generator(np.random.Philox(key=SEED))
    x = torch.from_numpy(g.integers(0, 32, size=(5, 3, 3)))
    lab = torch.from_numpy(g.integers(0, 16, size=(5,)))
    with torch.no_grad():
        out["small_logits"] = small(x, lab)
    out["small_x"], out["small_label"] = x, lab
    q = synth.exp1_noise(5, 9, 32, seed=5)
    sampler.arm(q)
    with torch.no_grad():
        out["small_codes"] = small.generate(None, lab, shape=(3, 3), batch_size=5)
    # full-size prior
    full = RefPixelCNN(512, 512, 15)
    load_synth(full, SEED + 2)
    x = torch.from_numpy(g.integers(0, 512, size=(2, 3, 3)))
    lab = torch.from_numpy(g.integers(0, 128, size=(2,)))
    with torch.no_grad():
        out["full_logits"] = full(x, lab)
    out["full_x"], out["full_label"] = x, lab
    codes = []
    labs = torch.tensor([0, 17, 64, 127])
    qf = synth.exp1_noise(4, 9, 512, seed=6)
    for b in range(4):                              # the reference's generate is called with B=1
        sampler.arm(qf[b:b + 1])
        with torch.no_grad():
            codes.append(full.generate(None, labs[b:b + 1], shape=(3, 3), batch_size=1))
    out["full_codes"], out["full_gen_label"] = torch.cat(codes), labs
    save("g4_pixelcnn", **out)


# ---- G6: Decoder ------------------------------------------------------------------------------------
def g6_decoder():
    out = {}
    for tag, sizes, lat in [("dec", [1024, 256, 55], 2560), ("pos", [1024, 128, 6], 2048)]:
        dec = ref_dvq.Decoder(layer_sizes=sizes, latent_size=lat)
        load_synth(dec, SEED + 3)
        z = synth.synthetic_normal((5, lat), SEED, f"dec/z/{tag}")
        with torch.no_grad():
            out[tag + "_y"] = dec(z)
    save("g6_decoder", **out)


# ---- G7: GenNet.gen end to end (config 1: 1 object x 8 grasps, reference called with B=1) -----------
class RefManoStandIn:
    """(5) quacks like the ``mano`` layer: .eval(), __call__(betas=, global_orient=, hand_pose=, transl=).vertices"""

    def __init__(self, oracle):
        self.oracle = oracle

    def eval(self):
        return self

    def __call__(self, betas, global_orient, hand_pose, transl):
        return types.SimpleNamespace(vertices=self.oracle(betas, hand_pose, global_orient, transl))


def gen_state_dict(net):
    """Synthetic GenNet weights with the object codebook made of the REFERENCE's object-type features of 128 seed clouds
    (synth.feature_codebook), so that idx6 differs from object to object; the codebook is stored in the fixture (fp16)."""
    sd = synth.synthetic_state_dict(net.state_dict(), SEED)
    sd["GatedPixelCNN.output_conv.2.bias"][128:] = -1e4                       # (4)
    net.load_state_dict(sd, strict=True)
    net.eval()
    with torch.no_grad():
        f, _, _ = net.obj_encoder_type(synth.seed_clouds(128, 1024))
    sd[synth.OBJECT_CODEBOOK] = synth.feature_codebook(f)
    net.load_state_dict(sd, strict=True)
    return sd


def g7_gen(sampler):
    net = RefGenNet()
    sd = gen_state_dict(net)
    mano = mano_oracle.ManoOracle(mano_oracle.synthetic_mano_arrays())
    net.set_rh_mano(RefManoStandIn(mano))
    n_obj, N = 8, 1024
    obj = synth.synthetic_clouds(n_obj, N, seed=42)
    q = synth.exp1_noise(n_obj, 9, 512, seed=43)
    rec, pos, codes, idx6s, feats = [], [], [], [], []
    for b in range(n_obj):
        sampler.arm(q[b:b + 1])
        captured = {}
        orig_gen = net.GatedPixelCNN.generate

        def spy(*a, _o=orig_gen, **k):
            r = _o(*a, **k)
            captured["codes"] = r.clone()
            return r

        net.GatedPixelCNN.generate = spy
        with torch.no_grad():
            r, p = net.gen(obj[b:b + 1])
            f, _, _ = net.obj_encoder_type(obj[b:b + 1])
            i6, _ = net.vqvae6.inference(f)
        net.GatedPixelCNN.generate = orig_gen
        rec.append(r); pos.append(p); codes.append(captured["codes"]); idx6s.append(i6); feats.append(f)
    feats = torch.cat(feats)
    E6 = sd[synth.OBJECT_CODEBOOK].double()
    d64 = ((feats.double()[:, None, :] - E6[None]) ** 2).sum(-1)
    top2 = torch.topk(d64, 2, dim=1, largest=False)[0]
    idx6 = torch.cat(idx6s).squeeze(1)
    gap = (top2[:, 1] - top2[:, 0]).float()
    print("g7 idx6", idx6.tolist(), "gaps", [f"{v:.2e}" for v in gap.tolist()])
    assert len(set(idx6[gap > G7_MARGIN].tolist())) >= 6, "fixture must bite: >= 6 distinct, well separated object codes"
    save("g7_gen", recon=torch.cat(rec), recon_pos=torch.cat(pos), codes=torch.cat(codes),
         idx6=idx6, idx6_gap=gap, idx6_margin=G7_MARGIN, E6_f16=sd[synth.OBJECT_CODEBOOK].half(),
         feat_type=feats, n_points=N, cloud_seed=42, noise_seed=43)


G8_MARGIN = 2e-4      # same for the seven codes of G8 (D = 256 / 1024 embeddings of magnitude ~1)
G7_MARGIN = 5e-4      # fp64 top-2 gap of the object code's squared distance above which fp32 paths must agree (noise ~2e-5)


def g7_gen_juice(sampler):
    """Re-run the juice case on the fp16-rounded cloud actually stored (keeps the fixture small and exact)."""
    net = RefGenNet()
    gen_state_dict(net)
    net.set_rh_mano(RefManoStandIn(mano_oracle.ManoOracle(mano_oracle.synthetic_mano_arrays())))
    pts = np.load(os.path.join(REF, "models/Object_models/juice_model/juice_modelresampled.npy"))
    diag = np.linalg.norm(pts.max(0) - pts.min(0))
    pc = np.concatenate([pts.T, np.full((1, pts.shape[0]), diag)], 0).astype(np.float16)[None]
    pc_t = torch.from_numpy(pc.astype(np.float32))
    q = synth.exp1_noise(8, 9, 512, seed=43)
    sampler.arm(q[:1])
    with torch.no_grad():
        r, p = net.gen(pc_t)
    save("g7_gen_juice", obj_f16=pc, recon=r, recon_pos=p)


# ---- G8: DVQVAE.forward eval --------------------------------------------------------------------------
def g8_dvqvae():
    """DVQVAE.forward eval.  The seven codebooks are the reference's own encoder outputs for 128 seed samples (hand-part
    embeddings / object-type features, fp16-rounded, stored in the fixture), so every sample gets its own codes."""
    net = ref_dvq.DVQVAE(obj_inchannel=4)
    sd = load_synth(net, SEED + 8)
    K = 128
    seed_obj = synth.seed_clouds(K, 512, seed=4180)
    seed_hand = synth.synthetic_normal((K, 3, 778), SEED, "dvq/seed_hand", 0.05)
    got = {}
    hooks = [m.register_forward_hook(lambda mod, a, out, k=k: got.__setitem__(k, out.detach())) for k, m in enumerate(net.handembnns)]
    hooks.append(net.obj_encoder_type.register_forward_hook(lambda mod, a, out: got.__setitem__(6, out[0].detach())))
    with torch.no_grad():
        for b0 in range(0, K, 16):
            net(seed_obj[b0:b0 + 16], seed_hand[b0:b0 + 16])
            for k in range(7):
                got.setdefault(("all", k), []).append(got[k])
    books = {}
    for k in range(7):
        E = synth.feature_codebook(torch.cat(got[("all", k)]))
        sd[f"vqvae{k}.vector_quantization.embedding.weight"] = E
        books[f"E{k}_f16"] = E.half()
    net.load_state_dict(sd, strict=True)
    net.eval()
    B = 3
    obj = synth.synthetic_clouds(B, 512, seed=80)
    hand = synth.synthetic_normal((B, 3, 778), SEED, "dvq/hand", 0.05)
    with torch.no_grad():
        emb_idx, obj_emb = net(obj, hand)
    for h in hooks:
        h.remove()
    rows = emb_idx.squeeze(1).view(7, B)
    gaps = []
    for k in (6, 0, 1, 2, 3, 4, 5):                                            # emb_idx order: idx6, idx0..5
        E = sd[f"vqvae{k}.vector_quantization.embedding.weight"].double()
        d64 = ((got[k].double()[:, None, :] - E[None]) ** 2).sum(-1)
        t2 = torch.topk(d64, 2, dim=1, largest=False)[0]
        gaps.append((t2[:, 1] - t2[:, 0]).float())
    gaps = torch.cat(gaps)
    print("g8 emb_idx", rows.tolist(), "min gap", float(gaps.min()))
    assert all(len(set(r.tolist())) == B for r in rows), "fixture must bite: pairwise-different codes across the samples"
    books["emb_gap"] = gaps
    books["emb_margin"] = G8_MARGIN
    save("g8_dvqvae", emb_idx=emb_idx.squeeze(1), obj_emb=obj_emb, **books)


def g0_state_dict_layout():
    """Every state_dict key with its shape and dtype, for the modules a checkpoint is loaded into (data, not source)."""
    import json
    out = {}
    for name, mod in (("GenNet", RefGenNet()), ("DVQVAE", ref_dvq.DVQVAE(obj_inchannel=4)),
                      ("GatedPixelCNN", RefPixelCNN(512, 512, 15, 128)), ("PointNetEncoder4", RefPointNet(channel=4)),
                      ("VQVAE", RefVQVAE(0, 0, 0, 128, 256, 0.25))):
        out[name] = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in mod.state_dict().items()]
    with open(os.path.join(ROOT, "tests", "golden", "g0_state_dict_layout.json"), "w") as f:
        json.dump(out, f)
    print("g0_state_dict_layout", {k: len(v) for k, v in out.items()})


def g9_mano_pkl():
    """models/mano/MANO_RIGHT.pkl as the MANO readers meet it (Python-2 pickle: chumpy Select/Ch, scipy csc_matrix, numpy arrays),
    byte for byte, except two payloads that keep it under the size limit: posedirs rounded to fp16 values (still float64; the
    readers' checks run at zero pose) and hands_coeffs, which neither reader reads, zeroed.  xz-compressed (data, not source)."""
    import lzma
    import pickletools
    raw = bytearray(open(os.path.join(REF, "models", "mano", "MANO_RIGHT.pkl"), "rb").read())
    key, seen = None, set()
    for op, arg, pos in pickletools.genops(bytes(raw)):
        if op.name == "SHORT_BINSTRING" and arg in ("posedirs", "hands_coeffs"):
            key = arg
        elif op.name == "BINSTRING" and key is not None and len(arg) > 1000:       # the key's array payload: 'T' + 4-byte length
            n = int.from_bytes(raw[pos + 1: pos + 5], "little")
            a = np.frombuffer(bytes(raw[pos + 5: pos + 5 + n]), "<f8")
            a = a.astype(np.float16).astype("<f8") if key == "posedirs" else np.zeros_like(a)
            raw[pos + 5: pos + 5 + n] = a.tobytes()
            seen.add(key)
            key = None
    assert seen == {"posedirs", "hands_coeffs"}, seen
    path = os.path.join(OUT, "g9_mano_right.pkl.xz")
    with open(path, "wb") as f:
        f.write(lzma.compress(bytes(raw), preset=9 | lzma.PRESET_EXTREME))
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "layout":
        g0_state_dict_layout()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "mano":
        g9_mano_pkl()
        return
    check_multinomial_equivalence()
    g0_state_dict_layout()
    sampler = RaceSampler()
    torch.Tensor.multinomial = lambda self, n, *a, **k: sampler(self, n, *a, **k)   # (6)
    g1_pointnet()
    g2_vq()
    g4_pixelcnn(sampler)
    g6_decoder()
    g7_gen(sampler)
    g7_gen_juice(sampler)
    g8_dvqvae()


if __name__ == "__main__":
    main()
