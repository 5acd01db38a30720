"""One-off behind DESIGN §7e: one negative-sampling step over a walk batch in three forms, alternated on the same tensors — Engine.sgns_step
in place, Engine.sgns_step in the exact form (into clones), and the torch recipe they replace (two nn.Embedding(sparse=True), gather,
bmm, logsigmoid, backward, optim.SGD.step; the id -> row look-up of the recipe is done once, outside the timed region).  Wall time
around calls that end in a synchronise; next to it the added bytes per second, W (C + K) D 4 / time, to hold against the chip-wide
float-atomic rate, and what a call costs before it adds anything: sgns_step over ONE window (the launch, the synchronisation and the
n_skipped read-back alone — the library's call ends in its own synchronise, so no event can be put between its kernel and its wait).
usage: sgns_timing.py [scale=20] [repeat=10] [walk_length=80] [context=10] [dim=128] [batch_sources=4096]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
pkg = _pkg.load()
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d      # noqa: E731
scale, rep, WL, CTX, D, B = arg(1, 20), arg(2, 10), arg(3, 80), arg(4, 10), arg(5, 128), arg(6, 4096)
LR = 0.025


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(v):
    return "median %.3f ms (min %.3f, max %.3f)" % (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3)


e = pkg.Engine(0)
e.generate_rmat(scale)
V = torch.as_tensor(e.vertices(), dtype=torch.int32, device="cuda")
nV = int(V.numel())
gen = torch.Generator().manual_seed(1)
sources = V[torch.randperm(nV, generator=gen)[:B].cuda()].contiguous()
in0 = ((torch.rand((nV, D), generator=gen) - 0.5) / D).cuda()
out0 = ((torch.rand((nV, D), generator=gen) - 0.5) / D).cuda()
print("%s  RMAT-%d undirected: %d vertices, %d sources, walk length %d, C = %d, D = %d, %d rounds after one warm-up"
      % (pkg.version(), scale, nV, B, WL, CTX, D, rep), flush=True)

for K in (5, 20):
    pos, neg = e.walk_skipgram_batch(sources, CTX, K, sg_seed=1, epoch=0, walk_length=WL, seed=1)
    W, T = int(pos.shape[0]), CTX - 1 + K
    rows = torch.searchsorted(V, torch.cat([pos, neg], dim=1).contiguous()).long()     # the recipe's row indices (every id is a vertex)
    c_idx, t_idx = rows[:, 0].contiguous(), rows[:, 1:].contiguous()
    sign = torch.tensor([1.0] * (CTX - 1) + [-1.0] * K, device="cuda")
    emb_in, emb_out = torch.nn.Embedding(nV, D, sparse=True).cuda(), torch.nn.Embedding(nV, D, sparse=True).cuda()
    opt = torch.optim.SGD(list(emb_in.parameters()) + list(emb_out.parameters()), lr=LR)

    def recipe():
        opt.zero_grad(set_to_none=True)
        f = torch.bmm(emb_out(t_idx), emb_in(c_idx).unsqueeze(2)).squeeze(2)
        loss = -torch.nn.functional.logsigmoid(sign * f).sum()
        loss.backward()
        opt.step()
        return loss

    a, b, na, nb = in0.clone(), out0.clone(), in0.clone(), out0.clone()
    names = ["sgns_step in place", "sgns_step exact form", "torch recipe", "sgns_step, one window"]
    tm = {k: [] for k in names}
    for r in range(rep + 1):                       # (round 0 warms every path up: code objects, the allocator)
        a.copy_(in0); b.copy_(out0); na.copy_(in0); nb.copy_(out0)
        with torch.no_grad():
            emb_in.weight.copy_(in0); emb_out.weight.copy_(out0)
        row = [timed(lambda: e.sgns_step(pos, neg, a, b, LR, loss=True))[0],
               timed(lambda: e.sgns_step(pos, neg, in0, out0, LR, into=(na, nb), loss=True))[0],
               timed(recipe)[0],
               timed(lambda: e.sgns_step(pos[:1], neg[:1], a, b, LR, loss=True))[0]]
        if r:
            for k, v in zip(names, row):
                tm[k].append(v)
    # the three forms did the same step: the exact form against the recipe, the largest difference of an element
    diff = max(float((na - emb_in.weight.detach()).abs().max()), float((nb - emb_out.weight.detach()).abs().max()))
    added = W * (CTX + K) * D * 4
    print("K = %2d  W = %d  added bytes %.3f GB  (largest |exact form - recipe| of a table element: %.3g)" % (K, W, added / 1e9, diff))
    for k in names:
        med = statistics.median(tm[k])
        rate = "  %.3f TB/s of added bytes" % (added / med / 1e12) if k.startswith("sgns_step") and "one" not in k else ""
        print("    %-24s %s%s" % (k, fmt(tm[k]), rate), flush=True)
    del emb_in, emb_out, opt, rows, c_idx, t_idx
