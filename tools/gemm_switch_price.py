"""Price of a source switch in the tiled fp16-plane GEMM: one source of K = 1536 against three of 512 and six of 256 (same total K,
same FLOPs) at M = 16 384, N = 1 024 through ops.linear_multi.  DVQ_TREE=<checkout> measures that checkout's library."""
import os, sys, torch
sys.path.insert(0, os.environ.get("DVQ_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dvqvae_amd
from dvqvae_amd import ops, packing
dev = "cuda:0"
M, N = 16384, 1024
res = []
for ks in ((1536,), (512,) * 3, (256,) * 6, (192,) * 8):
    g = torch.Generator().manual_seed(3)
    xs = [(torch.randn(M, k, generator=g) * 0.1).to(dev) for k in ks]
    ws = [(torch.randn(N, k, generator=g) * 0.03).to(dev) for k in ks]
    b = torch.randn(N, generator=g).to(dev)
    pls = packing.split_f16x2(ws)
    out = torch.empty(M, N, device=dev)
    pairs = list(zip(xs, ws))
    for _ in range(5): ops.linear_multi(pairs, b, out=out, planes=pls)
    torch.cuda.synchronize(); e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50): ops.linear_multi(pairs, b, out=out, planes=pls)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 50
    res.append((ks, us))
    print(f"sources {len(ks)} x K={ks[0]}: {us:.1f} us per launch", flush=True)
base = res[0][1]
for ks, us in res[1:]:
    sw = (len(ks) - 1) * 2          # switches per workgroup, two rounds of workgroups per launch
    print(f"  {len(ks)} sources: +{us - base:.1f} us = {(us - base) / sw * 1e3:.0f} ns per switch and round")
