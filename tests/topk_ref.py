"""srw_topk_rows restated in numpy float64 from the header comment of include/stellar_rw.h, the tolerance every returned score is held to,
the rule a result is checked by, and the inputs tests/test_gpu_topk.py and tests/test_topk_cpu.py share.

Scores (float64 of the float32 inputs):
    dot      s = sum_d q[d] r[d]
    cosine   s = dot / (sqrt(sum q^2) sqrt(sum r^2)), exactly 0 when either sum of squares is 0
    a NaN score ranks, and is returned, as -inf.
Query forms: rows only (query = table[rows[i]], that row excluded, a value outside [0, n) skips the query); vectors only (nothing
excluded); both (the vector, rows[i] excluded, -1 none, any other value outside [0, n) skips).  A skipped query returns padding and is
counted.  Order: the k best eligible rows by a stable sort on (-score, row); the tail is padding, row -1 and score -inf.

Tolerance per (query, row), u = 2^-24, derived and not measured:
    dot      eps = (D + 2) u sum_d |q_d r_d|: D products and D - 1 additions in ANY order (with fmaf fewer roundings still)
    cosine   eps = (2 D + 8) u: the dot term divided by the norms is <= (D + 2) u by Cauchy-Schwarz; the denominator — two sums of
             squares, two square roots, a product — has a relative error <= (D + 6) u, the divide is in there, and |cos| <= 1.

The rule for one query (check): s the float64 score, t the reference's k-th score, E the largest eps of the query's eligible rows.
    1. returned rows are distinct, in range and not excluded; there are min(k, eligible rows) of them, then padding
    2. every returned score is within its eps of s(row)
    3. returned scores are non-increasing, and equal bits are in ascending row order
    4. every eligible row with s > t + 2 E is returned, and no row with s < t - 2 E is
Rows inside the band are free; ambiguous() counts the queries where that freedom exists at all (more than one row within 2 E of t)."""
import functools
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
METRICS = ("cosine", "dot")

# (n, D, k): standard-normal tables, 64 queries taken from the rows.  On each at most one query in five is ambiguous under either
# metric (asserted from the reference alone in tests/test_topk_cpu.py); n 2000, D 1024, k 10 is NOT such a shape under cosine.
TOLERANCE_CASES = ((5000, 64, 10), (5000, 128, 64), (1000, 300, 10), (600, 1024, 5))
CASE_Q = 64


@functools.lru_cache(maxsize=None)
def case_inputs(n, D, k):
    """(table float32 [n, D], query rows int32 [64]) of a tolerance case: a pure function of the shape"""
    rng = np.random.default_rng(1000003 * n + 1009 * D + k)
    table = rng.standard_normal((n, D)).astype(np.float32)
    rows = rng.choice(n, size=CASE_Q, replace=False).astype(np.int32)
    table.setflags(write=False); rows.setflags(write=False)
    return table, rows


def all_scores(table, qvec, metric):
    """(S float64 [Q, n] with NaN already -inf, eps float64 [Q, n])"""
    T, Qv = np.asarray(table, dtype=np.float64), np.asarray(qvec, dtype=np.float64)
    D = T.shape[1]
    with np.errstate(all="ignore"):
        # (row by row, not a matrix product: the products are exact in float64 and numpy's sum along a row does not look at where the
        # row stands, so equal rows get equal float64 scores and the stable sort below orders them by row)
        dot = np.stack([(T * q).sum(axis=1) for q in Qv]) if len(Qv) else np.zeros((0, len(T)))
        if metric == "dot":
            S = dot
            eps = (D + 2) * U * np.stack([np.abs(T * q).sum(axis=1) for q in Qv]) if len(Qv) else np.zeros((0, len(T)))
        elif metric == "cosine":
            qq, rr = (Qv * Qv).sum(axis=1), (T * T).sum(axis=1)
            S = dot / (np.sqrt(qq)[:, None] * np.sqrt(rr)[None, :])
            S[qq == 0, :] = 0.0
            S[:, rr == 0] = 0.0
            eps = np.full(S.shape, (2 * D + 8) * U)
        else:
            raise ValueError(metric)
    S = np.where(np.isnan(S), -np.inf, S)
    eps = np.where(np.isfinite(eps), eps, 0.0)             # (a NaN row's score is -inf outright: nothing to tolerate)
    return S, eps


def topk(table, k, rows=None, vectors=None, metric="cosine"):
    """-> rows int64 [Q, k], scores float64 [Q, k], skipped, and what check() needs: S, eps, eligible [Q, n], skip [Q]"""
    table = np.asarray(table, dtype=np.float32)
    n, D = table.shape
    if rows is None and vectors is None:
        raise ValueError("no query form")
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
    Q = len(rows) if rows is not None else len(vectors)
    in_range = (rows >= 0) & (rows < n) if rows is not None else np.zeros(Q, dtype=bool)
    if vectors is None:
        skip = ~in_range
        qvec = np.zeros((Q, D), dtype=np.float32)
        qvec[in_range] = table[rows[in_range]]
    else:
        qvec = np.asarray(vectors, dtype=np.float32)
        skip = (rows != -1) & ~in_range if rows is not None else np.zeros(Q, dtype=bool)
    S, eps = all_scores(table, qvec, metric)
    eligible = np.ones((Q, n), dtype=bool)
    if rows is not None:
        eligible[np.nonzero(in_range)[0], rows[in_range]] = False
    eligible[skip] = False
    out_rows = np.full((Q, k), -1, dtype=np.int64)
    out_scores = np.full((Q, k), -np.inf)
    for i in range(Q):
        order = np.argsort(-S[i], kind="stable")           # rows ascend within equal scores
        order = order[eligible[i][order]][:k]
        out_rows[i, :len(order)] = order
        out_scores[i, :len(order)] = S[i, order]
    return SimpleNamespace(rows=out_rows, scores=out_scores, skipped=int(skip.sum()), S=S, eps=eps, eligible=eligible, skip=skip, k=k, n=n)


def _band(ref, i):
    """(t, E) of query i: the k-th reference score (-inf when fewer than k rows are eligible) and the largest eps of an eligible row"""
    el = ref.eligible[i]
    t = ref.scores[i, ref.k - 1] if ref.rows[i, ref.k - 1] >= 0 else -np.inf
    return t, (ref.eps[i][el].max() if el.any() else 0.0)


def ambiguous(ref):
    """queries with more than one eligible row within 2 E of t"""
    count = 0
    for i in range(len(ref.rows)):
        t, E = _band(ref, i)
        if np.isfinite(t):
            s = ref.S[i][ref.eligible[i]]
            count += int((np.abs(s - t) <= 2 * E).sum() > 1)
        else:
            count += int(t == -np.inf and ref.rows[i, ref.k - 1] >= 0 and (ref.S[i][ref.eligible[i]] == -np.inf).sum() > 1)
    return count


def check(ref, got_rows, got_scores):
    """The rule.  AssertionError names the query and the clause -> the worst |score - s| / eps over the returned rows."""
    got_rows = np.asarray(got_rows); got_scores = np.asarray(got_scores, dtype=np.float32)
    assert got_rows.shape == ref.rows.shape and got_scores.shape == ref.rows.shape, (got_rows.shape, ref.rows.shape)
    worst = 0.0
    for i in range(len(ref.rows)):
        el = ref.eligible[i]
        m = min(ref.k, int(el.sum()))
        r, sc = got_rows[i].astype(np.int64), got_scores[i]
        assert (r[m:] == -1).all() and (sc[m:] == -np.inf).all(), "query %d: the tail after %d rows is not padding: %s %s" % (i, m, r[m:], sc[m:])
        r, sc = r[:m], sc[:m]
        assert ((r >= 0) & (r < ref.n)).all(), "query %d: a row out of range or padding where a row was eligible: %s" % (i, r)      # 1
        assert len(set(r.tolist())) == m, "query %d: a row twice: %s" % (i, r)
        assert el[r].all(), "query %d: an excluded row is returned: %s" % (i, r[~el[r]])
        s, e = ref.S[i, r], ref.eps[i, r]
        same = (sc.astype(np.float64) == s)                                                                                # 2 (-inf == -inf)
        with np.errstate(invalid="ignore"):
            err = np.where(same, 0.0, np.abs(sc.astype(np.float64) - s))
        assert not np.isnan(sc).any() and (err <= e).all(), "query %d: a score off by more than its eps: rows %s err/eps %s" % (
            i, r[~(err <= e)], (err / e)[~(err <= e)])
        if m:
            worst = max(worst, float(np.max(np.where(e > 0, err / np.where(e > 0, e, 1.0), 0.0))))
        assert (sc[:-1] >= sc[1:]).all(), "query %d: scores increase: %s" % (i, sc)                                         # 3
        tie = sc[:-1].view(np.uint32) == sc[1:].view(np.uint32)
        assert (r[:-1][tie] < r[1:][tie]).all(), "query %d: equal score bits out of row order: %s" % (i, r)
        t, E = _band(ref, i)                                                                                               # 4
        must = np.nonzero(el & (ref.S[i] > t + 2 * E))[0]
        missing = np.setdiff1d(must, r)
        assert missing.size == 0, "query %d: rows above the band are missing: %s" % (i, missing)
        assert (s >= t - 2 * E).all(), "query %d: rows below the band are returned: %s" % (i, r[s < t - 2 * E])
    return worst


def check_exact(ref, got_rows, got_scores):
    """rows and score bits equal the reference outright (inputs whose every partial sum is an exact float32)"""
    got_rows = np.asarray(got_rows); got_scores = np.asarray(got_scores, dtype=np.float32)
    want = ref.scores.astype(np.float32)
    assert (want.astype(np.float64) == ref.scores).all(), "the reference's scores are no exact float32 values"
    bad = np.nonzero((got_rows != ref.rows).any(axis=1) | (got_scores.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "queries %s differ: first, rows %s / %s, scores %s / %s" % (
        bad[:8], got_rows[bad[0]], ref.rows[bad[0]], got_scores[bad[0]], want[bad[0]])


@functools.lru_cache(maxsize=None)
def repeated_table(distinct=150, copies=5, D=20, queries=6):
    """(table, query vectors): every one of `distinct` standard-normal vectors stands at `copies` rows, `distinct` rows apart (in
    other tiles of the scan); the queries are some of the vectors"""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((distinct, D)).astype(np.float32)
    table = np.tile(base, (copies, 1))
    qvec = base[rng.choice(distinct, size=queries, replace=False)].copy()
    table.setflags(write=False); qvec.setflags(write=False)
    return table, qvec


def integer_table(n, D, seed):
    """integers in -4 .. 4: every product and every partial sum of up to 1024 of them is an exact float32 in any order; ties everywhere"""
    return np.random.default_rng(seed).integers(-4, 5, size=(n, D)).astype(np.float32)
