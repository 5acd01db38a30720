"""One-off behind DESIGN §7c: Engine.skipgram (srw_skipgram_windows: count call + allocation + fill call), the fill call alone into
tensors that already exist, and the torch recipe they replace (unfold + validity mask + masked gather + torch.randint of [W, K]) on the
same walk result, alternated; wall time around calls that end in a synchronise.  Next to them the store-only ceiling of the same run:
torch.empty_like(pos).fill_(0).  usage: skipgram_timing.py [scale=20] [repeat=10] [directed=0] [walk_length=80] [context=10]"""
import ctypes as C
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
pkg = _pkg.load()
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rep = int(sys.argv[2]) if len(sys.argv) > 2 else 10
directed = bool(int(sys.argv[3])) if len(sys.argv) > 3 else False
WL = int(sys.argv[4]) if len(sys.argv) > 4 else 80
CTX = int(sys.argv[5]) if len(sys.argv) > 5 else 10


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def recipe(tp, tl, K, n_v):
    win = tp.unfold(1, CTX, 1)                                                  # [n, stride - C + 1, C], a view
    keep = torch.arange(win.shape[1], device=tp.device)[None, :] < (tl - (CTX - 1))[:, None]
    pos = win[keep]                                                             # the masked gather -> [W, C]
    neg = torch.randint(0, n_v, (pos.shape[0], K), dtype=torch.int32, device=tp.device) if K else None
    return pos, neg


def fmt(v):
    return "median %.3f ms (min %.3f, max %.3f)" % (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3)


e = pkg.Engine(0)
e.generate_rmat(scale, directed=directed)
st = e.walk(fetch=False, walk_length=WL, num_walks=1, seed=1)
tp, tl = e.paths_tensor()
n_v = e.num_vertices
print("%s  RMAT-%d %s: %d rows, stride %d, dead ends %d, C = %d, %d rounds after one warm-up" %
      (pkg.version(), scale, "directed" if directed else "undirected", tp.shape[0], tp.shape[1], st["dead_ends"], CTX, rep), flush=True)
for K in (0, 5, 20):
    t = {"skipgram()": [], "fill call": [], "torch recipe": [], "fill_(0)": []}
    sp = pkg.SkipgramParams(CTX, K, 1, 0)
    w = C.c_int64(0)
    for r in range(rep + 1):                       # (round 0 warms every path up: code objects, the allocator)
        a, (pos, neg) = timed(lambda: e.skipgram(CTX, K, seed=1, epoch=r))
        W = pos.shape[0]
        b, _ = timed(lambda: e._ck(pkg.lib().srw_skipgram_windows(e.h, None, None, 0, 1, C.byref(sp), C.c_void_p(pos.data_ptr()),
                                                                 C.c_void_p(neg.data_ptr()) if K else None, W, C.byref(w))))
        c, (rpos, rneg) = timed(lambda: recipe(tp, tl, K, n_v))
        assert torch.equal(rpos, pos)
        del rpos, rneg
        d, _ = timed(lambda: (torch.empty_like(pos).fill_(0), torch.empty_like(neg).fill_(0) if K else None))
        if r:
            for k, v in zip(t, (a, b, c, d)):
                t[k].append(v)
        del pos, neg
    gb = W * (CTX + K) * 4 / 1e9
    print("K = %2d  W = %d  output %.3f GB" % (K, W, gb))
    for k, v in t.items():
        print("    %-13s %s   %.0f GB/s of output" % (k, fmt(v), gb / statistics.median(v)), flush=True)
