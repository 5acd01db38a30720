"""One-off behind DESIGN §7f: Engine.topk_rows over RMAT-20's nV x 128 table, k = 10, for Q = 1, 32 and 1 024 queries by row, next to
the torch recipe it replaces (normalise, q @ table.T, mask the own row, topk; chunked over the queries where Q x nV floats are too many)
and next to a device copy of the table — the bytes per second one pass over the table cannot beat.  Wall time around calls that end in a
synchronise, one warm-up and `repeat` rounds, median (min - max); for the library also passes x table bytes / time as a fraction of the
copy's rate (a copy reads AND writes the table: its rate is counted on the bytes read alone).
usage: topk_timing.py [scale=20] [repeat=10] [dim=128] [k=10]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.zeros(1, device="cuda")                      # torch's HIP runtime first (tests/conftest.py::_torch_cuda_first)
import _pkg
pkg = _pkg.load()
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d      # noqa: E731
scale, rep, D, K = arg(1, 20), arg(2, 10), arg(3, 128), arg(4, 10)
CHUNK_FLOATS = 2**28                               # the recipe's Q x nV product, 1 GiB at a time


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
nV = len(e.vertices())
gen = torch.Generator().manual_seed(1)
table = ((torch.rand((nV, D), generator=gen) - 0.5)).cuda()
table_bytes = nV * D * 4
other = torch.empty_like(table)
QB = 32 if D <= 256 else 16 if D <= 512 else 8
print("%s  RMAT-%d: table %d x %d float32 (%.3f GB), k = %d, %d rounds after one warm-up" % (pkg.version(), scale, nV, D, table_bytes / 1e9, K, rep), flush=True)

copy = []
for r in range(rep + 1):
    t = timed(lambda: other.copy_(table))[0]
    if r:
        copy.append(t)
floor = table_bytes / statistics.median(copy)
print("device copy of the table  %s  -> %.3f TB/s of table bytes read" % (fmt(copy), floor / 1e12), flush=True)


def recipe(rows, metric):
    t = torch.nn.functional.normalize(table, dim=1) if metric == "cosine" else table
    out_r, out_s = [], []
    step = max(1, CHUNK_FLOATS // nV)
    for a in range(0, len(rows), step):
        idx = rows[a:a + step].long()
        s = t[idx] @ t.T
        s[torch.arange(len(idx), device="cuda"), idx] = float("-inf")
        v, i = torch.topk(s, K, dim=1)
        out_r.append(i); out_s.append(v)
    return torch.cat(out_r), torch.cat(out_s)


for metric in ("cosine", "dot"):
    for Q in (1, 32, 1024):
        rows = torch.randint(0, nV, (Q,), generator=gen).to(torch.int32).cuda()
        tm = {"topk_rows": [], "torch recipe": []}
        for r in range(rep + 1):
            a, (lib_r, lib_s, _) = timed(lambda: e.topk_rows(table, K, rows=rows, metric=metric))
            b, (ref_r, ref_s) = timed(lambda: recipe(rows, metric))
            if r:
                tm["topk_rows"].append(a); tm["torch recipe"].append(b)
        agree = float((lib_r.long() == ref_r).float().mean())
        passes = (Q + QB - 1) // QB
        med = statistics.median(tm["topk_rows"])
        print("%s  Q = %4d  (%d passes; %.4f of the recipe's rows agree, largest |score difference| %.3g)"
              % (metric, Q, passes, agree, float((lib_s - ref_s).abs().max())))
        print("    %-14s %s  %.3f TB/s of table bytes = %.3f of the copy's rate" % ("topk_rows", fmt(tm["topk_rows"]), passes * table_bytes / med / 1e12, passes * table_bytes / med / floor))
        print("    %-14s %s" % ("torch recipe", fmt(tm["torch recipe"])), flush=True)
