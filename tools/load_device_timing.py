"""One-off behind DESIGN §7b: a weighted RMAT graph (generate_rmat's stream, regenerated on the host by the oracle) loaded from device
tensors (Engine.load_coo with an int64 [2, E] edge_index: srw_load_coo_device) and from the same values on the host (srw_load_coo),
alternated, wall time around calls that end in a stream synchronise.  usage: load_device_timing.py [scale=22] [repeat=3]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
import oracle_py
from helpers import rmat_weights_np
pkg = _pkg.load()
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
rep = int(sys.argv[2]) if len(sys.argv) > 2 else 3
E = 16 << scale
s, d = oracle_py.rmat_edges(scale, E, seed=42)
w = rmat_weights_np(s, d, 42)
ei = torch.from_numpy(np.stack([s, d]).astype(np.int64)).to("cuda:0")
tw = torch.from_numpy(w).to("cuda:0")
torch.cuda.synchronize()
host, dev = pkg.Engine(0), pkg.Engine(0)
t = {"device": [], "host": [], "host+download": []}
for r in range(rep + 1):                           # (round 0 warms both paths up: code objects, the allocator)
    t0 = time.perf_counter(); dev.load_coo(ei, None, tw); a = time.perf_counter() - t0
    t0 = time.perf_counter(); host.load_coo(s, d, w); b = time.perf_counter() - t0
    t0 = time.perf_counter()
    h = ei.cpu().numpy().astype(np.int32); host.load_coo(h[0], h[1], tw.cpu().numpy())
    c = time.perf_counter() - t0
    print("round %d: device tensors %.1f ms | host arrays %.1f ms | tensors -> host -> int32 -> host load %.1f ms" % (r, a * 1e3, b * 1e3, c * 1e3), flush=True)
    if r:
        t["device"].append(a); t["host"].append(b); t["host+download"].append(c)
assert dev.stats() == host.stats()
print("RMAT-%d weighted, %d lines, stats %s: median of %d — %s" % (scale, E, dev.stats(), rep, ", ".join("%s %.1f ms" % (k, statistics.median(v) * 1e3) for k, v in t.items())))
