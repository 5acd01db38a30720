"""One-off behind DESIGN §7i: srw_importance_neighbors on an RMAT graph at restart = 0.5, shapes (R, L, T) = (10, 2, 3), (50, 4, 10) and
(200, 20, 50), 262 144 and 2 097 152 seeds drawn from the present vertices, next to the ceiling the first-order walk is held against —
srw_probe_request_rate's dependent random 16-byte reads per second, taken on the same handle in the same process.  A call is timed by a
host clock around Engine.importance_neighbors (it ends in a synchronise; the outputs' torch allocations are inside the window, as they
are for a user); steps = the steps actually taken, read from `total` under keep_seed (every visit is one step); one warm-up call per
case (the first also builds the first-order tables), then `repeat` calls with the cases alternated, median (min - max).  The fraction
printed is steps/s over reads/s: a step costs about one record read.  The share of a call spent in the selection comes from a run of
its own under a kernel trace (k_imp_topk against k_imp_walk in the statistics); `only` picks one case for that run.
usage: importance_timing.py [scale=24] [repeat=10] [only=-1]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
pkg = _pkg.load()
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d      # noqa: E731
scale, rep, only = arg(1, 24), arg(2, 10), arg(3, -1)

e = pkg.Engine(0)
e.generate_rmat(scale)
V = e.vertices()
nV, nE = e.stats()
rng = np.random.default_rng(1)
batches = {B: torch.as_tensor(V[rng.integers(0, len(V), B)].astype(np.int32)).cuda().contiguous() for B in (262144, 2097152)}
print("%s  RMAT-%d undirected: %d vertices, %d entries, %d rounds after one warm-up" % (pkg.version(), scale, nV, nE, rep), flush=True)
reads_per_s, gib = e.probe_request_rate()
print("probe_request_rate: %.3g dependent random 16-byte reads/s over %.1f GiB" % (reads_per_s, gib), flush=True)

cases = [(B, shape) for B in batches for shape in ((10, 2, 3), (50, 4, 10), (200, 20, 50))]
if only >= 0:
    cases = [cases[only]]
sec = {i: [] for i in range(len(cases))}
steps = {}
for r in range(rep + 1):
    for i, (B, (R, L, T)) in enumerate(cases):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, counts, total = e.importance_neighbors(batches[B], R, L, T, restart=0.5, seed=1, epoch=r, keep_seed=True, return_total=True)
        dt = time.perf_counter() - t0
        steps[i] = int(total.sum(dtype=torch.int64))
        del ids, counts, total
        if r:
            sec[i].append(dt)
for i, (B, shape) in enumerate(cases):
    med = statistics.median(sec[i])
    rate = steps[i] / med
    print("    %8d seeds  (R, L, T) = %-14s median %.3f ms (min %.3f, max %.3f)  %d steps: %.3g steps/s = %.2f x the probe's reads/s, %.3g seeds/s"
          % (B, shape, med * 1e3, min(sec[i]) * 1e3, max(sec[i]) * 1e3, steps[i], rate, rate / reads_per_s, B / med), flush=True)
e.close()
