"""Rows past the record-packing limits, against the CPU oracle.

The rest of the suite never builds an adjacency row longer than a few hundred thousand entries outside the full-size
scripts, so the limits that change a kernel's behaviour with the row length are crossed here on purpose:
  - CFO_NDEG_MAX = 2^23 - 2 (device_common.h): a 16-byte compact record keeps its neighbour's degree in 23 bits; a longer
    neighbour row makes the compact table escape to the exact 32-byte records (sampler_tables.hip cfo_write);
  - rows beyond 2^24 entries: the 24-bit lattice draw is coarser than the row, the f32 prefix certificate fails for unit
    weights, membership bitmaps need hundreds of 65 536-bit segments, per-edge tables hit their chunk cap;
  - the Mode A regularity certificate ceil_log2(n) + emax - emin <= 29 (alias_tables.hip) on both sides.
The graphs are stars built with numpy (8 M - 18 M entries).  The oracle is O(deg) per step taken from a hub, so
it walks every hub and a seeded sample of the leaves; the device's own variants are compared with its default walk on EVERY
walker.  Each leg asserts the path it means to test (record_bytes, kernel_kind, strategy_steps, alias_row(v)[0]) so that it
cannot pass on another one.  Each leg prints its wall time (pytest -s, or --durations)."""
import time

import numpy as np
import pytest

import oracle_py
from helpers import pkg

pytestmark = pytest.mark.gpu

CFO_NDEG_MAX = (1 << 23) - 2          # device_common.h
BIG = (1 << 24) + (1 << 20) + 3       # a row beyond 2^24 entries, not a power of two
L = 8
N_LEAVES = 96                         # sampled leaf walkers per oracle run (every hub walks too)
# Every vertex walks on the device, and a general-kernel step from a giant row costs O(row) work: millions of distinct leaves put
# millions of walkers on the hub at once (hours of kernel time).  So the hub rows hold parallel lines to a few thousand leaves, and the
# graphs are directed (a leaf's row stays short, as the oracle's O(row) membership scan wants); the hub rows keep their full length.
M_LEAVES = 4096
PQS_BIG = [(1.0, 1.0), (0.25, 4.0), (4.0, 0.5), (0.5, 1.0)]     # every one on the unit row, the first two on weighted rows
# tests/fuzz_parity.py's variant list (hub bitmaps only matter to the on-the-fly samplers, so they go off with the tables)
VARIANTS = [dict(force_general=True), dict(edge_tables=False), dict(edge_tables_all=True), dict(prefix=False),
            dict(binned=False), dict(hub_bitmaps=False, edge_tables=False), dict(compact=False)]


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


class _Leg:
    def __init__(self, name):
        self.name, self.t0 = name, time.time()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        print("[giant rows] %s: %.1f s" % (self.name, time.time() - self.t0), flush=True)


def _extra_leaf_edges(rng, lo, hi, n):
    """n leaf-leaf lines among ids lo..hi-1, no self loops: leaves are not all alike (rows of 1-3 entries, shared neighbours)."""
    a = rng.integers(lo, hi, n).astype(np.int32)
    b = rng.integers(lo, hi, n).astype(np.int32)
    keep = a != b
    return a[keep], b[keep]


def _star(n, rng, w_hub=None, m=M_LEAVES):
    """Directed star: hub 0 with exactly n out-entries over m leaves (1..m, interleaved: parallel lines), every leaf with one line
    back to the hub, plus a few hundred leaf-leaf lines so that leaves are not all alike."""
    a, b = _extra_leaf_edges(rng, 1, m + 1, 512)
    leaves = np.arange(1, m + 1, dtype=np.int32)
    s = np.concatenate([np.zeros(n, np.int32), leaves, a])
    d = np.concatenate([1 + (np.arange(n) % m).astype(np.int32), np.zeros(m, np.int32), b])
    w = None
    if w_hub is not None:
        w = np.concatenate([np.asarray(w_hub, np.float32), rng.integers(1, 17, m + len(a)).astype(np.float32)])
    return s, d, w


def _load(eng, s, d, w=None, directed=False):
    eng.load_coo(s, d, w, directed=directed)
    g = oracle_py.Graph.from_coo(s, d, w, directed=directed)
    assert eng.stats() == (g.num_vertices, g.num_entries)
    verts = eng.vertices()
    assert np.all(verts[1:] > verts[:-1])            # ascending: walker i starts at verts[i]
    return g, verts


def _sources(verts, hubs, rng, n_leaves=N_LEAVES):
    leaves = np.setdiff1d(verts, np.asarray(hubs, np.int32))
    src = np.unique(np.concatenate([np.asarray(hubs, np.int32), rng.choice(leaves, n_leaves, replace=False).astype(np.int32)]))
    sel = np.searchsorted(verts, src)
    assert np.array_equal(verts[sel], src)
    return src, sel


def _same(a, b):
    """a, b: (paths, lens); every walker."""
    if np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]):
        return True, ""
    bad = np.nonzero((a[0] != b[0]).any(axis=1) | (a[1] != b[1]))[0]
    return False, "%d walkers differ, first %d:\n  %s\n  %s" % (len(bad), bad[0], a[0][bad[0]], b[0][bad[0]])


def _against_oracle(eng, g, src, sel, kw, variants=(), sampler="reference"):
    """The default walk (and each variant) against the oracle on the sampled walkers; each variant against the default walk on
    every walker.  Returns the default walk's stats, the variants' stats and the oracle's paths."""
    t0 = time.time()
    ref = g.walk(sources=src, threads=oracle_py.threads(), sampler=1 if sampler == "alias" else 0, **kw)
    t1 = time.time()
    dp, dl, st = eng.walk(sampler=sampler, **kw)
    print("  %s %s: oracle %.1f s, device %.1f s" % (sampler, kw, t1 - t0, time.time() - t1), flush=True)
    ok, why = _same((dp[sel], dl[sel]), ref[:2])
    assert ok, "default walk %s != oracle: %s" % (kw, why)
    vst = []
    for v in variants:
        t1 = time.time()
        vp, vl, vs = eng.walk(sampler=sampler, **kw, **v)
        print("    %s: %.1f s" % (v, time.time() - t1), flush=True)
        ok, why = _same((vp, vl), (dp, dl))
        assert ok, "variant %s %s != default walk: %s" % (v, kw, why)
        assert vs["n_steps"] == st["n_steps"], (v, kw)
        vst.append(vs)
        del vp, vl
    return st, vst, ref[0]


def _strat(st, name):
    return st["strategy_steps"][name]


# ---- 1. the escape boundary: a neighbour row of exactly CFO_NDEG_MAX entries, then one more ------------------------------
@pytest.mark.parametrize("n,record_bytes", [(CFO_NDEG_MAX, 16), (CFO_NDEG_MAX + 1, 32)])
def test_escape_boundary_star(eng, n, record_bytes):
    rng = np.random.default_rng(n)
    with _Leg("escape star n=%d" % n):
        g, verts = _load(eng, *_star(n, rng), directed=True)
        src, sel = _sources(verts, [0], rng)
        kw = dict(p=1.0, q=1.0, walk_length=L, seed=11, first_walk=1)
        st, (vg, vx), _ = _against_oracle(eng, g, src, sel, kw, [dict(force_general=True), dict(compact=False)])
        assert st["kernel_kind"] == 1 and st["record_bytes"] == record_bytes, st
        assert vg["kernel_kind"] == 2 and vx["kernel_kind"] == 1 and vx["record_bytes"] == 32, (vg, vx)
        # p != 1, q == 1: the per-lane q1 kernel needs the compact table, so it runs only below the escape
        st, _, _ = _against_oracle(eng, g, src, sel, dict(kw, p=0.5, q=1.0), [dict(force_general=True)])
        assert st["kernel_kind"] == 2
        assert (_strat(st, "q1_lane") > 0) == (record_bytes == 16), st["strategy_steps"]
        st, _, _ = _against_oracle(eng, g, src, sel, dict(kw, p=0.25, q=4.0), [dict(edge_tables=False)])
        assert st["kernel_kind"] == 2


# ---- 2. one hub beyond 2^24 entries, three weight versions, every variant -------------------------------------------------
def _big_weights(kind, rng):
    if kind == "unit":
        return None
    if kind == "int16":
        return rng.integers(1, 17, BIG).astype(np.float32)
    heavy = 1 << 16                   # a long run of tiny weights, then heavy ones: guide deltas saturate (CFO_GD_SAT, compact records)
    return np.concatenate([np.full(BIG - heavy, 0.001, np.float32), np.full(heavy, 50.0, np.float32)])


@pytest.mark.parametrize("kind,regular", [("unit", 1), ("int16", 1), ("skewed", 0)])
def test_row_beyond_2_24(eng, kind, regular):
    rng = np.random.default_rng(24)
    with _Leg("2^24+ star %s" % kind):
        wh = _big_weights(kind, rng)
        g, verts = _load(eng, *_star(BIG, rng, wh), directed=True)
        assert g.degree(0) == BIG
        src, sel = _sources(verts, [0], rng)
        for p, q in (PQS_BIG if kind == "unit" else PQS_BIG[:2]):
            kw = dict(p=p, q=q, walk_length=L, seed=int(rng.integers(1, 1 << 30)), first_walk=int(rng.integers(0, 4)))
            # the variant list at p = q = 1 (first-order kernel, exact records, general kernel) and, on the unit row, at (0.25, 4), where
            # the general kernel's switches select other samplers: per-edge tables over the 2^24+ row, on-the-fly membership with and
            # without the multi-segment hub bitmaps, the binned search, the prefix sums
            full = p == q == 1.0 or (kind == "unit" and (p, q) == (0.25, 4.0))
            st, vst, _ = _against_oracle(eng, g, src, sel, kw, VARIANTS if full else ())
            print("    strategy steps", {k: v for k, v in st["strategy_steps"].items() if v}, "edge tables", st["edge_tables"], flush=True)
            assert st["kernel_kind"] == (1 if p == q == 1.0 else 2), (kw, st)
            if p == q == 1.0:
                assert st["record_bytes"] == 32, st          # the hub's leaves link a row past CFO_NDEG_MAX: escape
                assert vst[0]["kernel_kind"] == 2 and vst[-1]["record_bytes"] == 32
            elif full:
                byv = {tuple(sorted(v.items())): s for v, s in zip(VARIANTS, vst)}
                # the default walk took per-edge tables (masks over the leaf -> hub pairs) ...
                assert st["strategy_steps"]["edge_mask"] > 0 and st["edge_table_bytes"] > 0, st
                # ... and the tables-off variants the on-the-fly samplers (binned=False turns the tables off too)
                for v in (dict(edge_tables=False), dict(hub_bitmaps=False, edge_tables=False), dict(binned=False)):
                    s2 = byv[tuple(sorted(v.items()))]
                    assert s2["strategy_steps"]["edge_mask"] == 0 and s2["strategy_steps"]["edge_table"] == 0, (v, s2)
                    assert s2["edge_table_bytes"] == 0, (v, s2)
        # Mode A on the same row, both sides of the certificate
        a, b = eng.alias_row(0), g.alias_row(0)
        assert a[0] == b[0] == regular, (a[0], b[0])
        if regular:                   # (Mode A walks over an irregular giant row invert the CDF per step: 65-160 s here, not run)
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
            for p, q in ((1.0, 1.0), (0.25, 4.0)):
                st, _, _ = _against_oracle(eng, g, src, sel, dict(p=p, q=q, walk_length=L, seed=5), sampler="alias")
                assert st["kernel_kind"] == 3


# ---- 2b. a giant row that stays compact: a source with more than 2^24 out-entries and no in-edges --------------------------
def _source_star(n, rng, w_hub=None, m=M_LEAVES):
    """Directed: hub 0 with n out-entries over m leaves; the leaves form a ring (and a few hundred extra lines) and none points back,
    so no record names the hub's row and the compact records need no escape."""
    a, b = _extra_leaf_edges(rng, 1, m + 1, 512)
    leaves = np.arange(1, m + 1, dtype=np.int32)
    s = np.concatenate([np.zeros(n, np.int32), leaves, a])
    d = np.concatenate([1 + (np.arange(n) % m).astype(np.int32), 1 + leaves % m, b])
    w = None
    if w_hub is not None:
        w = np.concatenate([np.asarray(w_hub, np.float32), rng.integers(1, 17, m + len(a)).astype(np.float32)])
    return s, d, w


@pytest.mark.parametrize("kind", ["unit", "skewed"])
def test_compact_records_on_a_giant_source_row(eng, kind):
    """The hub's walkers take their first step through cfo_pick on a 2^24+ row: the 24-bit lattice coarser than the row (unit
    weights: many entries share one c) and, with the skewed weights, saturated guide deltas resolved by bisection."""
    rng = np.random.default_rng(42)
    nw = 32                            # one draw from the hub per iteration
    with _Leg("compact source row %s" % kind):
        sdw = _source_star(BIG, rng, _big_weights(kind, rng))
        g, verts = _load(eng, *sdw, directed=True)
        assert g.degree(0) == BIG
        src, sel = _sources(verts, [0], rng)
        kw = dict(p=1.0, q=1.0, walk_length=4, num_walks=nw, seed=77, first_walk=2)
        ref = g.walk(sources=src, threads=oracle_py.threads(), **kw)
        dp, dl, st = eng.walk(**kw)
        assert st["kernel_kind"] == 1 and st["record_bytes"] == 16, st
        rows = (np.arange(nw)[:, None] * len(verts) + sel[None, :]).ravel()      # iteration-major, like the oracle's
        ok, why = _same((dp[rows], dl[rows]), ref[:2])
        assert ok, "compact walk != oracle: %s" % why
        assert src[0] == 0 and len(np.unique(dp[np.arange(nw) * len(verts) + sel[0], 1])) > 1     # the hub's draws differ
        for v, kind_, rb in ((dict(force_general=True), 2, None), (dict(compact=False), 1, 32)):
            vp, vl, vs = eng.walk(**kw, **v)
            assert vs["kernel_kind"] == kind_ and (rb is None or vs["record_bytes"] == rb), (v, vs)
            ok, why = _same((vp, vl), (dp, dl))
            assert ok, "variant %s != default walk: %s" % (v, why)
        if kind == "unit":
            # the same graph on two virtual shards: a walker seeded on the hub must not travel with a link whose degree is
            # clamped to CFO_NDEG_MAX (it would only ever reach the row's first 2^23 - 2 entries)
            with pkg().Cluster([0, 0]) as cl:
                cl.load_coo(*sdw, directed=True)
                assert cl.stats() == eng.stats()
                cp, cl_, cs = cl.walk(**kw)
                ok, why = _same((cp, cl_), (dp, dl))
                assert ok, "sharded != replicated: %s" % why
                assert cs["n_steps"] == st["n_steps"]


# ---- 4. directed: a hub with more than 2^23 out-entries, some leaves dead ends -----------------------------------------
def test_directed_giant_hub(eng):
    rng = np.random.default_rng(4)
    n = CFO_NDEG_MAX + 4096
    with _Leg("directed hub"):
        m = M_LEAVES
        leaves = np.arange(1, m + 1, dtype=np.int32)
        back = leaves[leaves % 4 != 0]                   # leaves % 4 == 0 have no out-entry: dead ends
        a, b = _extra_leaf_edges(rng, 1, m + 1, 512)
        a, b = a[a % 4 != 0], b[a % 4 != 0]
        s = np.concatenate([np.zeros(n, np.int32), back, a])
        d = np.concatenate([1 + (np.arange(n) % m).astype(np.int32), np.zeros(len(back), np.int32), b])
        g, verts = _load(eng, s, d, directed=True)
        src, sel = _sources(verts, [0], rng)
        for p, q in ((1.0, 1.0), (0.25, 4.0)):
            kw = dict(p=p, q=q, walk_length=L, seed=int(rng.integers(1, 1 << 30)))
            st, _, _ = _against_oracle(eng, g, src, sel, kw, [dict(force_general=True)] + ([dict(compact=False)] if p == 1.0 else []))
            assert st["dead_ends"] > 0
            if p == q == 1.0:
                assert st["kernel_kind"] == 1 and st["record_bytes"] == 32, st


# ---- 5. Mode A: n > 2^24 with weights 1..32 is irregular (1..16 is regular: test_row_beyond_2_24[int16]) -------------------
def test_mode_a_irregular_giant_row(eng):
    """Only the tables: a Mode A walk over an irregular giant row inverts the CDF at every step from the hub (65 s for one call at
    p = q = 1 on this star, profiles/r07_giant_rows.md); the irregular fallback's walks are pinned on small rows by test_mode_a.py."""
    rng = np.random.default_rng(5)
    with _Leg("Mode A 1..32"):
        g, verts = _load(eng, *_star(BIG, rng, rng.integers(1, 33, BIG).astype(np.float32)), directed=True)
        a, b = eng.alias_row(0), g.alias_row(0)
        assert a[0] == b[0] == 0, (a[0], b[0])
        assert len(a[1]) == len(b[1]) == BIG
