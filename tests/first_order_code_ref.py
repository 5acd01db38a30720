"""The compact first-order records' guide code restated in numpy (csrc/device_common.h: CfoEnt, CFO_GD_EDGE) — written from
the rule, not from the kernels.  Shared by tests/test_first_order_code_cpu.py and tests/test_gpu_first_order_reads.py.

  builder  cdf_k = the f64 chain acc += w_k / S (S the left-to-right f64 sum), c_k = min(floor(cdf_k * 2^24), 2^24 - 1),
           guide[j] = first k with cdf_k >= T_j * 2^-24, T_j = ceil(j * 2^24 / deg); the stored 12-bit code of bucket j is
             EDGE   when j - guide[j] == 1 and c[j - 1] == T_j          (the certificate)
             SAT    when the delta is outside -2047 .. 2046              (a genuine 2047 included)
             delta  otherwise
  pick     lattice draw m, bucket j = (m * deg) >> 24, record j loaded; under EDGE the delta is 1 for the bucket's lowest draw
           (((m - 1) * deg) >> 24 < j) and 0 for every other; a positive delta scans forward from j - delta and takes record j from
           the copy it holds; SAT bisects.  Returns (position, records loaded).
"""
import numpy as np

ONE = 1 << 24
EDGE, SAT = 2047, -2048

UNIT_DEGS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 48, 64, 96, 1000, 1024, 3072, 4096)


def rows():
    """[(name, float32 weights)] — the rows of the issue: every unit-weight degree whose thresholds are integers somewhere, and the
    weighted rows that must keep plain deltas."""
    rng = np.random.default_rng(20261019)
    out = [("unit%d" % d, np.ones(d, np.float32)) for d in UNIT_DEGS]
    out.append(("equal3.0", np.full(48, 3.0, np.float32)))
    out.append(("pattern1.5_0.5", np.tile(np.array([1.5, 0.5], np.float32), 32)))           # delta 1 where the certificate fails
    heavy = np.ones(4096, np.float32); heavy[0] = 3.0 * 4095.0                               # cdf_0 = 0.75: deltas 1 .. 3071, 2047 among them
    out.append(("heavy_first", heavy))
    out.append(("int1..16", np.tile(np.arange(1, 17, dtype=np.float32), 4)))
    out.append(("random5decades", (10.0 ** rng.uniform(-2.5, 2.5, 300)).astype(np.float32)))
    return out


def thresholds(deg):
    j = np.arange(deg, dtype=np.uint64)
    return ((j << np.uint64(24)) + np.uint64(deg - 1)) // np.uint64(deg)       # T_j = ceil(j * 2^24 / deg)


def build(w, edge_code=True, certificate=True, saturate_reserved=True):
    """(c [deg] int64, code [deg] int64).  certificate / saturate_reserved = False plant the builder's two defects."""
    w = np.asarray(w, np.float32)
    deg = len(w)
    wd = w.astype(np.float64)
    S = np.cumsum(wd)[-1]                                   # (cumsum adds left to right)
    cdf = np.cumsum(wd / S)
    c = np.minimum(np.floor(cdf * float(ONE)), ONE - 1).astype(np.int64)
    T = thresholds(deg).astype(np.int64)
    guide = np.searchsorted(cdf, T.astype(np.float64) / float(ONE), side="left").astype(np.int64)   # (T * 2^-24 is exact)
    j = np.arange(deg, dtype=np.int64)
    delta = j - guide
    code = np.where((delta < -2047) | (delta > (2046 if saturate_reserved else 2047)), SAT, delta)
    if edge_code:
        cert = np.ones(deg, bool)
        if certificate:
            cert[1:] = c[:-1] == T[1:]
        cert[0] = False
        code = np.where((delta == 1) & cert, EDGE, code)
    return c, code


def coded_buckets(code):
    return np.flatnonzero(code == EDGE)


def is_lowest(m, deg, j):
    return m >= 1 and (((m - 1) * deg) >> 24) < j


def pick(c, code, m, reload=False, drop_lowest_test=False, reuse_at=0):
    """(position, loads).  reload: the pick of before the code (record j loaded again when the scan comes back to it).
    drop_lowest_test / reuse_at != 0 plant the pick's two defects (reuse_at: the kept record stands in for record j + reuse_at)."""
    deg = len(c)
    j = (m * deg) >> 24
    reads = 1
    gd = int(code[j])
    if gd == SAT:
        lo, hi = 0, deg
        while lo < hi:
            mid = lo + ((hi - lo) >> 1); reads += 1
            if c[mid] < m:
                lo = mid + 1
            else:
                hi = mid
        return (lo if lo < deg else 0), reads + 1
    if gd == EDGE:
        gd = 1 if (drop_lowest_test is False and is_lowest(m, deg, j)) else 0
    k = j - gd
    cur = c[j]
    if gd > 0:
        cur = c[k]; reads += 1
        while cur < m:
            k += 1
            if k == j + reuse_at and not reload:
                cur = c[j]                      # the kept record of bucket j, no load
            else:
                cur = c[k]; reads += 1
            if k == j:
                break                           # from j on: the common scan below
    elif gd < 0:
        cur = c[k]; reads += 1
    while cur < m:
        k += 1
        if k >= deg:
            return 0, reads + 1                 # no crossing: edges.head
        cur = c[k]; reads += 1
    return k, reads


def brute(c, m):
    k = int(np.searchsorted(c, m, side="left"))  # first k with c_k >= m
    return k if k < len(c) else 0


def draws(w, c, n_random=3000, seed=1):
    """Sorted distinct 24-bit draws: around every bucket threshold and every c_k, the ends, and random ones."""
    deg = len(c)
    T = thresholds(deg).astype(np.int64)
    rng = np.random.default_rng(seed + deg)
    m = np.concatenate([T - 1, T, T + 1, T + 2, c - 1, c, c + 1, [0, ONE - 1], rng.integers(0, ONE, n_random)])
    return np.unique(np.clip(m, 0, ONE - 1)).astype(np.int64)
