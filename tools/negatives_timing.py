"""One-off behind DESIGN §7d: Engine.skipgram_batch under four settings — uniform, degree^0.75 weights, and both with exclusion — next to
Engine.skipgram of the same tree (the yardstick) and the torch recipe the weighted draw replaces (torch.multinomial on the same weights,
reshaped to [W, K]), alternated on the same walk result; wall time around calls that end in a synchronise.  set_negative_weights and
visit_counts are printed once each.  usage: negatives_timing.py [scale=20] [repeat=10] [walk_length=80] [context=10]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
pkg = _pkg.load()
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rep = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WL = int(sys.argv[3]) if len(sys.argv) > 3 else 80
CTX = int(sys.argv[4]) if len(sys.argv) > 4 else 10


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(v):
    return "median %.3f ms (min %.3f, max %.3f)" % (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3)


def multinomial(prob, W, K):
    """the recipe: W * K draws with replacement, in slices of 2^24 (torch.multinomial's limit on num_samples)"""
    total, out = W * K, []
    for i in range(0, total, 1 << 24):
        out.append(torch.multinomial(prob, min(1 << 24, total - i), replacement=True))
    return torch.cat(out).view(W, K)


e = pkg.Engine(0)
e.generate_rmat(scale)
st = e.walk(fetch=False, walk_length=WL, num_walks=1, seed=1)
tp, tl = e.paths_tensor()
print("%s  RMAT-%d undirected: %d rows, stride %d, dead ends %d, C = %d, %d rounds after one warm-up" %
      (pkg.version(), scale, tp.shape[0], tp.shape[1], st["dead_ends"], CTX, rep), flush=True)
t, cnt = timed(lambda: e.visit_counts())
print("visit_counts()           %.3f ms (%d tokens)" % (t * 1e3, int(cnt.sum())))
deg = e.degrees_tensor().double().pow(0.75)
t, q = timed(lambda: e.set_negative_weights(deg))
print("set_negative_weights()   %.3f ms (quantisation in torch included)" % (t * 1e3), flush=True)
prob = q.double()

for K in (5, 20):
    names = ["skipgram() [yardstick]", "batch uniform", "batch weighted", "batch uniform + excl", "batch weighted + excl", "torch.multinomial"]
    tm = {k: [] for k in names}
    for r in range(rep + 1):                       # (round 0 warms every path up: code objects, the allocator)
        row = []
        e.set_negative_weights(None)
        a, (pos, neg) = timed(lambda: e.skipgram(CTX, K, seed=1, epoch=r))
        W = pos.shape[0]
        del pos, neg
        row.append(a)
        for weighted in (False, True):             # (the table is set outside the timed call)
            e.set_negative_weights(q if weighted else None)
            a, out = timed(lambda: e.skipgram_batch(CTX, K, seed=1, epoch=r))
            del out
            row.append(a)
        for weighted in (False, True):
            e.set_negative_weights(q if weighted else None)
            a, out = timed(lambda: e.skipgram_batch(CTX, K, seed=1, epoch=r, exclude_window=True, max_draws=8))
            del out
            row.append(a)
        a, out = timed(lambda: multinomial(prob, W, K))
        del out
        row.append(a)
        if r:
            for k, v in zip(names, row):
                tm[k].append(v)
    print("K = %2d  W = %d  output %.3f GB (pos + neg)" % (K, W, W * (CTX + K) * 4 / 1e9))
    for k in names:
        print("    %-24s %s" % (k, fmt(tm[k])), flush=True)
