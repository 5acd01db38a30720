"""srw_sgns_step restated in numpy float64 from the text of include/stellar_rw.h (vectorised gathers, einsum, np.add.at), with the
quantities the derived tolerance needs for every output element, and the inputs tests/test_sgns_cpu.py and tests/test_gpu_sgns.py
share.

The tolerance (u = 2^-24):    |got - want| <= u (D + m + 8) max(1, S) (|old value| + A)
  m   the number of terms lr g x that land on the element
  A   the sum of |lr x| over those terms (|g| <= 1)
  S   the largest sum_d |in[c][d] out[t][d]| of the call: D u S bounds the error of a dot product in any reduction order, a quarter of
      it reaches sigma (sigma' <= 1/4); m u covers the sum in any arrival order; 8 u the evaluation of sigma, lr g and the product.
For loss[w]:                  u (D + C - 1 + K + 8) max(1, S) sum_i (1 + |f_i|)      (softplus' <= 1, softplus(x) <= 1 + |x|)
"""
import numpy as np

U = 2.0 ** -24


def slots_of(V, ids):
    """position in V (ascending) of every id, -1 for an id that is no entry of V"""
    V = np.asarray(V, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    if V.size == 0:
        return np.full(ids.shape, -1, dtype=np.int64)
    k = np.minimum(np.searchsorted(V, ids), V.size - 1)
    return np.where(V[k] == ids, k, -1)


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


def softplus(x):
    return np.logaddexp(0.0, x)


class Result:
    pass


def step(V, pos, neg, tin, tout, lr, center, new_in, new_out, mutate=None):
    """The header's lines.  tin / tout: the old tables [nV][D]; new_in / new_out: the new tables' contents before the call (the same
    array object for one table in both roles).  lr is taken as the float32 the ABI carries.  mutate: None, "drop_negative" (the last
    negative of the first window that is not skipped makes no add and no loss term) or "flip_g" (the sign of g of that window's first
    target) — the two wrong updates tests/test_sgns_cpu.py holds the tolerance against.
    -> Result: new_in, new_out, loss [W] (float64); skipped; f [Wv][T]; m_in, m_out [nV]; A_in, A_out [nV][D]; S; ok [W] (not skipped).
    With one table new_in is new_out, m_in is m_out and A_in is A_out: the sums over both roles."""
    pos = np.asarray(pos, dtype=np.int64)
    W, C = pos.shape
    neg = np.zeros((W, 0), dtype=np.int64) if neg is None else np.asarray(neg, dtype=np.int64)
    K = neg.shape[1]
    T = C - 1 + K
    tin = np.asarray(tin, dtype=np.float64)
    tout = np.asarray(tout, dtype=np.float64)
    nV, D = tin.shape
    lr = float(np.float32(lr))
    one = new_in is new_out
    r = Result()
    r.new_in = np.array(new_in, dtype=np.float64)
    r.new_out = r.new_in if one else np.array(new_out, dtype=np.float64)
    r.m_in = np.zeros(nV)
    r.m_out = r.m_in if one else np.zeros(nV)
    r.A_in = np.zeros((nV, D))
    r.A_out = r.A_in if one else np.zeros((nV, D))
    sl = np.concatenate([slots_of(V, pos), slots_of(V, neg)], axis=1)            # [W][C + K]
    r.ok = (sl >= 0).all(axis=1)
    r.skipped = int(W - r.ok.sum())
    r.loss = np.zeros(W)
    sl = sl[r.ok]
    c = sl[:, center]                                                             # [Wv]
    t = np.delete(sl, center, axis=1)                                             # [Wv][T]: the other contexts in order, then the negatives
    label = (np.arange(T) < C - 1).astype(np.float64)
    vin, vout = tin[c], tout[t]                                                   # [Wv][D], [Wv][T][D]
    r.f = np.einsum("wd,wtd->wt", vin, vout)
    r.S = float(np.einsum("wd,wtd->wt", np.abs(vin), np.abs(vout)).max()) if r.f.size else 0.0
    g = np.where(label > 0, sigmoid(-r.f), -sigmoid(r.f))                         # label - sigma(f)
    lw = np.where(label > 0, softplus(-r.f), softplus(r.f))
    live = np.ones_like(g)
    if mutate == "drop_negative":
        assert K > 0 and g.shape[0] > 0
        live[0, T - 1] = 0.0
    elif mutate == "flip_g":
        g[0, 0] = -g[0, 0]
    else:
        assert mutate is None
    g = g * live
    r.loss[r.ok] = (lw * live).sum(axis=1)
    np.add.at(r.new_out, t.reshape(-1), ((lr * g)[:, :, None] * vin[:, None, :]).reshape(-1, D))
    np.add.at(r.new_in, c, lr * np.einsum("wt,wtd->wd", g, vout))
    np.add.at(r.m_out, t.reshape(-1), 1.0)
    np.add.at(r.m_in, c, float(T))
    np.add.at(r.A_out, t.reshape(-1), np.broadcast_to(np.abs(lr * vin)[:, None, :], vout.shape).reshape(-1, D))
    np.add.at(r.A_in, c, np.abs(lr * vout).sum(axis=1))
    r.T, r.D = T, D
    return r


def table_bound(r, which, old):
    """the tolerance of every element of new_in ("in") or new_out ("out"); old: the new table's contents before the call"""
    m, A = (r.m_in, r.A_in) if which == "in" else (r.m_out, r.A_out)
    return U * (r.D + m[:, None] + 8.0) * max(1.0, r.S) * (np.abs(np.asarray(old, dtype=np.float64)) + A)


def loss_bound(r):
    b = np.zeros(r.loss.shape)
    b[r.ok] = U * (r.D + r.T + 8.0) * max(1.0, r.S) * (1.0 + np.abs(r.f)).sum(axis=1)
    return b


def worst(got, want, bound):
    """max over the elements of |got - want| / bound, an element with bound 0 counting as 0 when it is exact and as inf when not"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


# ---- the inputs both test files use ------------------------------------------------------------------------------------------------
def tables(nV, D, seed, scale_in=0.5, scale_out=0.1):
    """float32 tables uniform in +-scale"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-scale_in, scale_in, size=(nV, D)).astype(np.float32),
            rng.uniform(-scale_out, scale_out, size=(nV, D)).astype(np.float32))


def tables_for(nV, D, seed):
    """+-0.5 and +-0.1 at D = 64, scaled by sqrt(64 / D) beyond: S = sum_d |in out| stays near 0.8 for every D, as trained embeddings
    keep their dot products and not their elements"""
    sc = (64.0 / D) ** 0.5
    return tables(nV, D, seed, 0.5 * sc, 0.1 * sc)


HEAVY_NV, HEAVY_W, HEAVY_C, HEAVY_K = 16, 4096, 3, 2


def heavy_graph():
    """a ring over the ids 3 .. 18 as load_adjacency takes it: (vertex, [(neighbour, weight)])"""
    ids = list(range(3, 3 + HEAVY_NV))
    return [(v, [(ids[(i + 1) % HEAVY_NV], 1.0), (ids[(i - 1) % HEAVY_NV], 1.0)]) for i, v in enumerate(ids)]


def heavy_windows(seed=11):
    """4 096 hand-made windows over 16 vertices, skewed as a walk's are (vertex i with weight 1 / (i + 1)): thousands of terms on
    the rows of the frequent vertices, tens on the rare ones'.  The last vertex occurs once in the whole call, as the first target
    of window 0: an element with m = 1 next to elements with m in the thousands."""
    rng = np.random.default_rng(seed)
    ids = np.arange(3, 3 + HEAVY_NV, dtype=np.int32)
    p = 1.0 / (1.0 + np.arange(HEAVY_NV - 1))
    draw = lambda shape: ids[rng.choice(HEAVY_NV - 1, size=shape, p=p / p.sum())]      # noqa: E731
    pos, neg = draw((HEAVY_W, HEAVY_C)), draw((HEAVY_W, HEAVY_K))
    pos[0, 1] = ids[-1]
    pos[5] = pos[5, 0]                                   # a window of one vertex: every target is the centre
    neg[5, 0] = pos[5, 0]
    neg[6, 1] = neg[6, 0]                                # the same negative twice
    neg[7, 0] = pos[7, 1]                                # a negative equal to a context
    return ids, pos, neg


# karate (ids as they are, vmin = 1): the shapes of the exact-form tests and the walk whose windows they take
KARATE_WALK = dict(walk_length=20, num_walks=1, seed=5, p=0.5, q=2.0, rng="philox")
KARATE_SG = dict(seed=3, epoch=2)                        # srw_skipgram_batch's keys (no weight table, no exclusion)
KARATE_SHAPES = [(2, 0), (1, 1), (3, 2), (5, 5), (4, 60)]  # 1, 1, 4, 9, 63 targets: the tail of the four-at-a-time reduction, C + K = 64
KARATE_DIMS = [64, 128, 192, 512]
KARATE_W = 96                                            # windows taken from the batch (the first ones)
LR = 0.025


def centers(C):
    return sorted({0, C // 2, C - 1})
