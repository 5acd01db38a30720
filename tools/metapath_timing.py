"""One-off behind DESIGN §7g: the metapath walk next to the kernel it is shaped after, alternated on one graph in one process —
Engine.walk(p = 1, q = 1, force_general=True) (k_walk_general: one wave per walker, every neighbour a candidate, no type bytes) as the
yardstick, then Engine.walk_metapath with pattern [-1] (the same walk through the typed pick), and with types id mod 3 the patterns
[0, 1, 2] and [0, 1] from the sources of type 0.  Kernel time from the library's own events (stats.kernel_ms), walk-steps per second =
stats.n_steps / kernel time; one warm-up round, then `repeat` rounds, median (min - max).  set_vertex_types once more on its own: the
per-entry type bytes it lays out and the wall time of the call (it ends in a synchronise).
usage: metapath_timing.py [scale=20] [repeat=10] [walk_length=80]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
pkg = _pkg.load()
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d      # noqa: E731
scale, rep, WL = arg(1, 20), arg(2, 10), arg(3, 80)


def fmt(v, unit="ms", k=1.0):
    return "median %.3f %s (min %.3f, max %.3f)" % (statistics.median(v) * k, unit, min(v) * k, max(v) * k)


e = pkg.Engine(0)
e.generate_rmat(scale)
V = e.vertices()
nV, nE = e.stats()
types3 = torch.as_tensor((V % 3).astype(np.uint8)).cuda()
src0 = torch.as_tensor(V[V % 3 == 0].astype(np.int32)).cuda().contiguous()
print("%s  RMAT-%d undirected: %d vertices, %d entries, walk length %d, one iteration, %d rounds after one warm-up"
      % (pkg.version(), scale, nV, nE, WL, rep), flush=True)

tb = []
for r in range(4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.set_vertex_types(types3)
    tb.append(time.perf_counter() - t0)
print("set_vertex_types: %d type bytes per entry array (%.1f MB), call %s; first call %.3f ms" % (nE, nE / 1e6, fmt(tb[1:], k=1e3), tb[0] * 1e3))

kw = dict(walk_length=WL, num_walks=1, seed=1)
cases = [
    ("walk(p=1, q=1, force_general=True)", lambda: e.walk(fetch=False, p=1.0, q=1.0, force_general=True, **kw)),
    ("walk_metapath([-1])", lambda: e.walk_metapath([-1], fetch=False, **kw)),
    ("walk_metapath([0, 1, 2]), sources of type 0", lambda: e.walk_metapath([0, 1, 2], fetch=False, sources=src0, **kw)),
    ("walk_metapath([0, 1]), sources of type 0", lambda: e.walk_metapath([0, 1], fetch=False, sources=src0, **kw)),
]
ms = {k: [] for k, _ in cases}
info = {}
for r in range(rep + 1):                           # (round 0 warms every path up: code objects, the sorted rows of the general kernel)
    for name, f in cases:
        st = f()
        info[name] = st
        if r:
            ms[name].append(st["kernel_ms"])
base = None
for name, _ in cases:
    st = info[name]
    med = statistics.median(ms[name])
    rate = st["n_steps"] / (med * 1e-3)
    base = base or rate
    print("    %-46s %s  %d walkers, %d steps, %d dead ends, %d chain steps: %.3g steps/s (%.2f x the general kernel's)"
          % (name, fmt(ms[name]), st["n_walkers"], st["n_steps"], st["dead_ends"], st["fallbacks"], rate, rate / base), flush=True)
