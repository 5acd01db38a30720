"""Mode A (alias tables + rejection) — what its tests are held to, stated without the oracle and without the kernels.
Shared by tests/test_mode_a_ref_cpu.py (the oracle against these statements, and the conditions on the inputs) and
tests/test_gpu_mode_a_edges.py (the device against the oracle bit for bit, and against these statements).

  boundary_rows()             weight rows at the shape boundaries of k_alias_build: the 256-entry tile, the four waves of a block scan,
                              the LDS staging cap of 2048, prefix sums beyond 2^64, the certificate at 29 against 30, zero and
                              subnormal weights, rows that are not alias-regular
  implied_error(w, prob, a)   the distribution a table implies against w / sum(w), in exact rational arithmetic, as a multiple of a
                              derived bound
  transition_probabilities()  the first two steps of the walk in float64, from the text of DESIGN §4.6 (and three wrong readings)
  chi_z()                     Pearson's chi-square of observed triples against such probabilities, as a z score
  stat_graph(), walk_edge_graphs()   the graphs of the statistical test and of the walk's edge cases

  cap_walk()                  the rejection loop replayed where acceptance does not depend on the candidate: the trial cap, exactly

No import of the oracle and none of the product: numpy, fractions and the numpy Philox of tests/skipgram_ref.py."""
from fractions import Fraction

import numpy as np

from skipgram_ref import philox_np

LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4097)
U128_N = 32768
U128_HEAVY = np.float32((2.0 - 2.0 ** -23) * 2.0 ** 14)     # the largest float32 below 2^15: exponent 14, ceil_log2(32768) + 14 = 29
MODELS = ("exact", "nofold", "swap", "unit")


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def boundary_rows():
    """[(name, float32 weights, alias-regular?)] — the names are unique; the order is fixed (row i is vertex i of the GPU file's graph)."""
    rows = []

    def add(name, w, regular=True):
        rows.append((name, _f32(w), bool(regular)))

    for n in LENGTHS:
        add("tie3113_%d" % n, np.resize([3, 1, 1, 3], n))           # D_i == E_j everywhere; n % 4 == 0: every heavy keeps T
        for where, k in (("first", 0), ("mid", n // 2), ("last", n - 1)):
            w = np.ones(n); w[k] = 1000.0
            add("oneheavy_%s_%d" % (where, n), w)
        for where, k in (("first", 0), ("last", n - 1)):
            w = np.full(n, 5.0); w[k] = 0.125
            add("onelight_%s_%d" % (where, n), w)
        for split in (256, 257):                                     # whole tiles without a light / without a heavy, carries live
            if n > split:
                add("lights_then_heavies_%d_%d" % (split, n), [1.0] * split + [5.0] * (n - split))
                add("heavies_then_lights_%d_%d" % (split, n), [5.0] * split + [1.0] * (n - split))
        add("rand_%d" % n, np.random.default_rng(n).random(n) * 8)
        z = np.resize([0, 2, 0, 0, 7, 1], n).astype(np.float64); z[-1] = 1
        add("zeros_%d" % n, z)
        if n >= 512:
            z = z.copy(); z[256:512] = 0                             # one tile of zero weights only (lights of deficit T)
            add("zeros_tile_%d" % n, z)
    # prefix sums beyond 2^64: the deficits of 16 384 lights of about 2^52 each
    half = U128_N // 2
    add("u128_split", [1.0] * half + [U128_HEAVY] * half)
    add("u128_interleaved", np.resize(np.array([1.0, U128_HEAVY]), U128_N))
    rng = np.random.default_rng(128)
    w = np.concatenate([1.0 + rng.random(half), 2.0 ** 14 * (1.0 + rng.random(half))]).astype(np.float32)
    w = np.minimum(w, U128_HEAVY)                                    # (a draw that rounds up to 2^15 would cost the certificate)
    w[:half] = np.minimum(w[:half], np.nextafter(np.float32(2), np.float32(0)))
    add("u128_rand", w[rng.permutation(U128_N)])
    # the certificate ceil_log2(n) + e_max - e_min <= 29 on both sides, on rows that stage in LDS and just beyond
    add("cert_2_29", [1.0, 2.0 ** 28])
    add("cert_2_30", [1.0, 2.0 ** 29], False)
    add("cert_2048_29", [1.0] + [2.0 ** 18] * 2047)
    add("cert_2049_30", [1.0] + [2.0 ** 18] * 2048, False)           # ceil_log2 steps at 2049
    add("cert_2049_29", [1.0] + [2.0 ** 17] * 2048)
    add("subnormal", [1e-45, 3e-45, 2.0 ** -126, 2.0 ** -125] * 16)  # biased exponent 0 counts as -126
    # not alias-regular, alone and inside a row of 2049 entries
    base = np.random.default_rng(2049).random(2049) + 0.5
    for name, bad in (("allzero", None), ("negative", [-1.0]), ("nan", [np.nan]), ("inf", [np.inf]), ("range", [1e-30, 1e30])):
        add("irregular_" + name, [0.0, 0.0, 0.0] if bad is None else [1.0] + bad + [2.0], False)
        w = np.zeros(2049) if bad is None else base.copy()
        if bad is not None:
            w[1500:1500 + len(bad)] = bad
        add("irregular_%s_2049" % name, w, False)
    assert len({r[0] for r in rows}) == len(rows)
    return rows


# ---- the table against the weights ------------------------------------------------------------------------------------------------
_SCALE = 149          # every finite float32 is an integer multiple of 2^-149


def _ints(a):
    """float32 values as exact integers, in units of 2^-149 (a power-of-two scaling in float64 never rounds here)"""
    return [int(x) for x in (np.asarray(a, dtype=np.float32).astype(np.float64) * 2.0 ** _SCALE)]


def implied_error(w, prob, alias):
    """The worst ratio err_k / bound_k of a table against the weights, in exact rational arithmetic on the float32 values.

    The table implies P_k = (sum over slots j of prob_j [j = k] + (1 - prob_j) [alias_j = k]) / n; the weights say w_k / sum(w);
    err_k is the absolute difference.  bound_k = (c_k + 1) * 2^-25 / n with c_k the number of slots whose alias is k.  The bound is
    DERIVED, not measured: the construction keeps, for every slot, an exact quotient kept_j / T in [0, 1] — with those quotients the
    table is the distribution exactly — and stores it as ONE float32 rounding, which is off by at most half a unit in the last place
    of a number below 1, 2^-25.  Entry k receives its own slot and c_k others, so at most c_k + 1 such roundings, each divided by n.
    (Every float32 is a multiple of 2^-149, so the sums below are sums of Python integers over one denominator; the ratio returned
    is a Fraction.)  A result <= 1 says: this table is the weights' distribution up to the rounding of prob."""
    n = len(w)
    one = 1 << _SCALE
    wi, pi = _ints(w), _ints(prob)
    S = sum(wi)
    P = [0] * n                        # n * P_k in units of 2^-149
    c = [0] * n
    for j in range(n):
        a = int(alias[j])
        P[j] += pi[j]
        P[a] += one - pi[j]
        c[a] += 1
    worst = Fraction(0)
    for k in range(n):
        # |P_k / (n 2^149) - w_k / S|  over  (c_k + 1) 2^-25 / n
        num = abs(P[k] * S - wi[k] * n * one) << 25
        den = (c[k] + 1) * one * S
        if num * worst.denominator > worst.numerator * den:
            worst = Fraction(num, den)
    return worst


def table_is_well_formed(prob, alias):
    """0 <= prob <= 1, 0 <= alias < n, and a slot that keeps everything names itself"""
    n = len(prob)
    prob, alias = np.asarray(prob), np.asarray(alias)
    return bool(np.all((prob >= 0) & (prob <= 1)) and np.all((alias >= 0) & (alias < n))
                and np.all(alias[prob == 1] == np.arange(n)[prob == 1]))


def deficit_excess_prefixes(w):
    """(D, E, light indices, heavy indices) of the construction in Python integers: W_k = w_k * 2^(23 - e_min), T = sum W, m_k = W_k n,
    lights m_k < T with deficits T - m_k, heavies with excesses m_k - T, inclusive prefix sums in index order."""
    w = np.asarray(w, dtype=np.float32)
    n = len(w)
    ex = (w[w != 0].view(np.uint32) >> 23) & 0xFF
    emin = int(np.where(ex == 0, -126, ex.astype(np.int64) - 127).min())
    W = [x >> (_SCALE - 23 + emin) for x in _ints(w)]               # the builder's own integers, so that 2^64 means what it means there
    T = sum(W)
    D, E, L, H = [], [], [], []
    d = e = 0
    for k in range(n):
        m = W[k] * n
        if m >= T:
            e += m - T; E.append(e); H.append(k)
        else:
            d += T - m; D.append(d); L.append(k)
    return D, E, L, H


def certificate(w):
    """ceil_log2(n) + e_max - e_min over the non-zero weights (finite, non-negative rows only)"""
    w = np.asarray(w, dtype=np.float32)
    ex = (w[w != 0].view(np.uint32) >> 23) & 0xFF
    e = np.where(ex == 0, -126, ex.astype(np.int64) - 127)
    return (len(w) - 1).bit_length() + int(e.max()) - int(e.min())


# ---- the first two steps in float64 -----------------------------------------------------------------------------------------------
def adjacency(s, d, w, directed):
    """{vertex: (ids int32, weights float32)} in line order; an undirected line (a, b, w) adds b to row a, then a to row b."""
    rows = {}
    for a, b, x in zip(np.asarray(s).tolist(), np.asarray(d).tolist(), _f32(w).tolist()):
        rows.setdefault(a, []).append((b, x))
        rows.setdefault(b, [])
        if not directed:
            rows[b].append((a, x))
    return {v: (np.array([e[0] for e in r], dtype=np.int32), np.array([e[1] for e in r], dtype=np.float32)) for v, r in sorted(rows.items())}


def _merged(ids, weights):
    out = {}
    for y, x in zip(ids.tolist(), weights.tolist()):
        out[y] = out.get(y, 0.0) + x
    tot = sum(out.values())
    return {y: x / tot for y, x in out.items() if x > 0}


def transition_probabilities(neighbors, p, q, model="exact"):
    """{(v, x, y): probability that a walk from v goes to x and then to y}, in float64.  From a source v the first step is ~ w; the
    second step from x with previous v is ~ w * (1/p if y == v, else 1 if y in N(v), else 1/q), parallel edges summed.  A walk that
    stops at x (no out-entry) is the cell (v, x, -1); a source without out-entries has no cell.
    model: "exact", or a deliberately wrong reading, used only to show that a test has teeth — "nofold": the return bias clipped to
    Q = max(1, 1/q) (the envelope without the appendix); "swap": 1 and 1/q exchanged; "unit": weights ignored."""
    assert model in MODELS
    inv_p, inv_q = 1.0 / float(p), 1.0 / float(q)
    ret = min(inv_p, max(1.0, inv_q)) if model == "nofold" else inv_p
    near, far = (inv_q, 1.0) if model == "swap" else (1.0, inv_q)
    out = {}
    for v, (ids, w) in neighbors.items():
        if len(ids) == 0:
            continue
        w = np.ones(len(ids)) if model == "unit" else w.astype(np.float64)
        nv = set(ids.tolist())
        for x, px in _merged(ids, w).items():
            xi, xw = neighbors[x]
            if len(xi) == 0:
                out[(v, x, -1)] = px
                continue
            xw = np.ones(len(xi)) if model == "unit" else xw.astype(np.float64)
            bias = np.array([ret if y == v else near if y in nv else far for y in xi.tolist()])
            for y, py in _merged(xi, xw * bias).items():
                out[(v, x, y)] = px * py
    return out


def triple_counts(paths):
    """{(v1, v2, v3): count} over the rows of a walk_length = 1 walk (-1 where the walk had stopped)"""
    u, c = np.unique(np.asarray(paths)[:, :3], axis=0, return_counts=True)
    return {tuple(int(x) for x in k): int(n) for k, n in zip(u, c)}


def chi_z(obs, expected, NW, emin=10):
    """(z, dof, share of cells left out): Pearson's chi-square of the observed counts against NW * expected[(v, x, y)] (NW walks per
    source) over the cells with NW * p >= emin, as z = (chi2 - dof) / sqrt(2 dof).  dof = cells kept - sources among them (each
    source's counts sum to NW).  An observed cell the expectation does not know is impossible under it: z = inf."""
    kept = [k for k, pr in expected.items() if NW * pr >= emin]
    dof = len(kept) - len({k[0] for k in kept})
    left = 1.0 - len(kept) / max(len(expected), 1)
    if any(k not in expected for k in obs) or dof <= 0:
        return float("inf"), dof, left
    chi = sum((obs.get(k, 0) - NW * expected[k]) ** 2 / (NW * expected[k]) for k in kept)
    return (chi - dof) / np.sqrt(2.0 * dof), dof, left


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
def stat_graph():
    """(src, dst, w): 12 vertices, 60 lines, self-loops, parallel edges whose float64 sums are no float32 values (0.1 + 0.3, ...)"""
    rng = np.random.default_rng(7)
    nv, nl = 12, 60
    s = rng.integers(0, nv, nl).astype(np.int32)
    d = rng.integers(0, nv, nl).astype(np.int32)
    for k in range(0, nl, 7):
        d[k] = s[k]
    for k in range(3, nl, 5):
        s[k], d[k] = s[k - 1], d[k - 1]
    w = rng.choice(np.float32([0.5, 1.0, 1.5, 2.0, 3.25, 7.0, 0.1, 0.3]), nl)
    return s, d, w


STAT_PQ = ((0.25, 4.0), (4.0, 0.5), (0.5, 1.0), (0.25, 0.25), (1.0, 1.0), (2.0, 2.0))
STAT_KW = dict(walk_length=1, num_walks=50000, seed=11)


def model_differs(model, p, q):
    """does the wrong reading change a probability at (p, q)?"""
    return {"nofold": 1.0 / p > max(1.0, 1.0 / q), "swap": q != 1.0, "unit": True}[model]


STAGING_L = (13, 14, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49)
STAGING_PQ = ((1.0, 1.0), (0.25, 4.0))
STAGING_NUM_WALKS = 40                # 51 vertices: 2040 walkers, eight blocks of 256
CAP_KW = dict(p=2.0 ** 20, q=2.0 ** 20, walk_length=7, num_walks=3, seed=3)
HUB_N = 3000


def cap_walk(neighbors, tables, p, q, walk_length, num_walks, seed, cap=65536):
    """The rejection loop of DESIGN §4.6 where it is simplest: a graph without triangles walked with p = q >= 1, so that every
    candidate of a second-order step has the bias 1/p = 1/q and a trial is accepted iff (x3 >> 8) * 2^-24 < 1/q, whatever it drew.
    Trial t of step s draws Philox(ctr = (iteration, source, s, t), key = (seed, 0xA11A5)); slot j = ((x0:x1) * deg) >> 64; the coin
    (x2 >> 8) * 2^-24 < prob[j] keeps j, else alias[j]; the step takes the first accepted trial's candidate, or trial cap - 1's.
    tables: {vertex: (prob, alias)}.  Returns (paths [walkers, walk_length + 2], trials drawn in all)."""
    assert p == q >= 1.0
    verts = sorted(neighbors)
    t = np.arange(cap)
    thr = float(np.float32(1.0) / np.float32(q)) * 2.0 ** 24
    paths, trials = [], 0
    for it in range(num_walks):
        for src in verts:
            path = [src]
            for s in range(1, walk_length + 2):
                ids = neighbors[path[-1]][0]
                x0, x1, x2, x3 = philox_np(it, src, s, t if s > 1 else t[:1], seed, 0xA11A5)
                ok = np.nonzero((x3 >> np.uint64(8)).astype(np.float64) < thr)[0] if s > 1 else [0]
                k = int(ok[0]) if len(ok) else cap - 1
                trials += k + 1
                j = ((int(x0[k]) << 32 | int(x1[k])) * len(ids)) >> 64
                prob, alias = tables[path[-1]]
                if not (np.float32(int(x2[k]) >> 8) * np.float32(2.0 ** -24) < prob[j]):
                    j = int(alias[j])
                path.append(int(ids[j]))
            paths.append(path)
    return np.array(paths, dtype=np.int32), trials


def parallel_groups(s, d, w):
    """{unordered pair: float64 sum of its lines' weights in line order} for the pairs named by more than one line"""
    groups = {}
    for a, b, x in zip(np.asarray(s).tolist(), np.asarray(d).tolist(), _f32(w).tolist()):
        groups.setdefault((min(a, b), max(a, b)), []).append(x)
    out = {}
    for k, xs in groups.items():
        if len(xs) > 1:
            t = 0.0
            for x in xs:
                t += x
            out[k] = t
    return out


def walk_edge_graphs():
    """{name: (src, dst, w, directed)} — the graphs of tests/test_gpu_mode_a_edges.py, sections c to f."""
    G = {}
    # c. path staging: a chain 0 -> 1 -> ... -> 49, every vertex with a light edge to the sink 50 (a dead end at every depth), parallel
    # weighted edges two steps back and a few one step back (return edges: p matters; N(prev) holds the sink: q matters)
    s, d, w = [], [], []
    for i in range(50):
        if i < 49:
            s.append(i); d.append(i + 1); w.append(1.0)
        s.append(i); d.append(50); w.append(0.03)
        if i >= 2 and i % 3 != 1:
            s += [i, i]; d += [i - 2, i - 2]; w += [0.5, 0.25]
        if i >= 1 and i % 4 == 0:
            s.append(i); d.append(i - 1); w.append(0.75)
    G["staging"] = (np.int32(s), np.int32(d), _f32(w), True)
    # d. the trial cap: a path, no triangle, p = q = 2^20 -> every second-order trial is accepted with probability 2^-20
    G["cap"] = (np.int32([0, 1, 2, 3]), np.int32([1, 2, 3, 4]), _f32([1, 2, 1, 3]), False)
    # e. the return edge's weight: parallel groups whose float64 sum is a float32 (1 + 2, 0.5 + 0.5) and is not (0.1 + 0.2 + 0.3,
    # 1000 + 0.001), a self-loop with a parallel twin, a pair named as (a, b) and as (b, a), and simple edges around them
    lines = [(0, 1, 1.0), (0, 1, 2.0), (1, 2, 0.5), (1, 2, 0.5), (2, 3, 0.1), (2, 3, 0.2), (2, 3, 0.3), (3, 4, 1000.0), (3, 4, 0.001),
             (4, 4, 1.5), (4, 4, 0.25), (4, 5, 1.0), (5, 4, 2.5), (5, 0, 1.0), (0, 2, 1.0), (1, 3, 2.0), (3, 5, 0.5), (6, 0, 1.0),
             (6, 3, 0.1), (3, 6, 0.7), (2, 5, 1.25), (7, 6, 3.0), (7, 1, 1.0), (4, 0, 0.3), (0, 4, 0.1)]
    s, d, w = (np.array([e[k] for e in lines]) for k in range(3))
    G["multi"] = (s.astype(np.int32), d.astype(np.int32), _f32(w), False)
    G["multi_directed"] = (s.astype(np.int32), d.astype(np.int32), _f32(w), True)
    # a -> b with weight 1 and b -> a with weight 0 (pairs 0/1, 2/3) or absent (pairs 4/5, 6/7): 1/p > Q and nothing to fold
    lines = [(0, 1, 1.0), (1, 0, 0.0), (1, 2, 1.0), (2, 3, 1.0), (3, 2, 0.0), (3, 4, 2.0), (4, 5, 1.0), (5, 6, 1.0), (5, 0, 0.5),
             (6, 7, 1.0), (7, 0, 1.0), (7, 2, 1.0), (0, 4, 0.5), (2, 6, 0.5), (1, 0, 0.0), (4, 0, 1.0)]
    s, d, w = (np.array([e[k] for e in lines]) for k in range(3))
    G["noreturn"] = (s.astype(np.int32), d.astype(np.int32), _f32(w), True)
    # f. membership by the shorter row: hub 0 with HUB_N leaves; leaves 1 .. 2000 in pairs (degree 2, partners linked), leaves
    # 2001 .. 3000 each with an outer vertex that the hub does not know (outer vertices chained among themselves)
    leaves = np.arange(1, HUB_N + 1)
    outer = HUB_N + 1 + np.arange(1000)
    s = np.concatenate([np.zeros(HUB_N, np.int64), np.arange(1, 2001, 2), np.arange(2001, HUB_N + 1), outer[:-1]])
    d = np.concatenate([leaves, np.arange(2, 2001, 2), outer, outer[1:]])
    w = 1.0 + (np.arange(len(s)) % 5) * 0.5
    G["hub"] = (s.astype(np.int32), d.astype(np.int32), _f32(w), False)
    return G
