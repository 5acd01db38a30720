"""One-off behind DESIGN §7h: srw_sample_neighbors on an RMAT graph, fanouts [25, 10] and [15, 10, 5], with and without replacement,
next to the ceiling the first-order walk is held against — srw_probe_request_rate's dependent random 16-byte reads per second, taken on
the same handle in the same process.  A call is timed by a host clock around Engine.sample_neighbors (it ends in a synchronise; the
layers' torch allocations are inside the window, as they are for a user); samples = the elements of all layers; one warm-up call per
case (it also builds the first-order tables), then `repeat` calls with the cases alternated, median (min - max).  The fraction printed
is samples/s over reads/s: a sample with replacement costs one parent row read shared by f lanes plus ~1 record read.
usage: neighbors_timing.py [scale=22] [batch=65536] [repeat=10]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
pkg = _pkg.load()
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d      # noqa: E731
scale, B, rep = arg(1, 22), arg(2, 65536), arg(3, 10)

e = pkg.Engine(0)
e.generate_rmat(scale)
V = e.vertices()
nV, nE = e.stats()
rng = np.random.default_rng(1)
seeds = torch.as_tensor(V[rng.integers(0, len(V), B)].astype(np.int32)).cuda().contiguous()
print("%s  RMAT-%d undirected: %d vertices, %d entries, %d seeds, %d rounds after one warm-up" % (pkg.version(), scale, nV, nE, B, rep), flush=True)
reads_per_s, gib = e.probe_request_rate()
print("probe_request_rate: %.3g dependent random 16-byte reads/s over %.1f GiB" % (reads_per_s, gib), flush=True)

cases = [(fan, rp) for fan in ([25, 10], [15, 10, 5]) for rp in (True, False)]
sec = {i: [] for i in range(len(cases))}
n_samples = {}
for r in range(rep + 1):
    for i, (fan, rp) in enumerate(cases):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        layers = e.sample_neighbors(seeds, fan, seed=1, epoch=r, replace=rp)
        dt = time.perf_counter() - t0
        n_samples[i] = sum(int(x.numel()) for x in layers)
        del layers
        if r:
            sec[i].append(dt)
for i, (fan, rp) in enumerate(cases):
    med = statistics.median(sec[i])
    rate = n_samples[i] / med
    print("    fanouts %-12s %-20s median %.3f ms (min %.3f, max %.3f)  %d samples: %.3g samples/s = %.2f x the probe's reads/s"
          % (fan, "with replacement" if rp else "without replacement", med * 1e3, min(sec[i]) * 1e3, max(sec[i]) * 1e3, n_samples[i], rate,
             rate / reads_per_s), flush=True)
e.close()
