"""Prior-sampler microbench (GPU box): ms per ops.pixelcnn_sample call of the product's GatedPixelCNN (512 tokens, dim 512, 15 layers,
128 classes, synthetic weights) at B rows (default 16 384: one chunk of the benchmark step) -- gated, gated-from-state, residual and
bias launches of the tiled fp16-plane GEMM in the proportions of the step.  DVQ_TREE=<checkout> measures that checkout's library."""
import os, sys, torch
root = os.environ.get("DVQ_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import dvqvae_amd
from dvqvae_amd import ops, synth
from dvqvae_amd.network.pixelcnn.models import GatedPixelCNN
from util import load_synth
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
dev = "cuda:0"
net = GatedPixelCNN(512, 512, 15, 128); load_synth(net, 5); net = net.to(dev)
pk = net.packed()
lab = torch.randint(0, 128, (B,), generator=torch.Generator().manual_seed(1)).to(dev)
q = synth.exp1_noise(B, 9, 512, seed=2).to(dev)
for _ in range(3): codes = ops.pixelcnn_sample(pk, lab, q)
torch.cuda.synchronize(); e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10): codes = ops.pixelcnn_sample(pk, lab, q)
e1.record(); torch.cuda.synchronize()
import hashlib
print(f"prior sample B={B}: {e0.elapsed_time(e1) / 10:.2f} ms per call, codes sha {hashlib.sha256(codes.cpu().numpy().tobytes()).hexdigest()[:12]}", flush=True)
