"""Metapath walks (srw_vertex_types_set / srw_walk_metapath): unless a test says otherwise EVERY walker is compared, id for id, with the
restatement of the header comment (tests/metapath_ref.py: the oracle's rows, a numpy mask by type, the oracle's draw and the oracle's
RandomSample.sample on the masked weights).  There is no tolerance anywhere in this file.  Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import metapath_ref as mref
from conftest import KARATE
from helpers import pkg, random_multigraph, rmat_lines

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


def assert_rows(got, want, what):
    (gp, gl), (wp, wl) = got, want
    assert gp.shape == wp.shape and gl.shape == wl.shape, (what, gp.shape, wp.shape)
    bad = np.nonzero((gp != wp).any(axis=1) | (gl != wl))[0]
    assert bad.size == 0, "walkers differ %s: %d, first %d\n got=%s (len %d)\nwant=%s (len %d)" % (
        what, bad.size, bad[0], gp[bad[0]], gl[bad[0]], wp[bad[0]], wl[bad[0]])


def check(oracle, e, g, types, pattern, what="", **kw):
    """One walk_metapath call against the restatement: every row, lens, the tail, and the stats."""
    paths, lens, st = e.walk_metapath(pattern, **kw)
    ref = mref.walk(oracle, g, types, pattern, **{k: v for k, v in kw.items()})
    assert_rows((paths, lens), ref[:2], (what, pattern, kw))
    assert (st["n_walkers"], st["n_steps"], st["dead_ends"], st["kernel_kind"]) == (len(lens), ref[2], ref[3], 4), (what, st, ref[2:])
    for k in ("sum_deg_curr", "sum_deg_prev", "ent_reads", "trials", "record_bytes", "edge_tables", "edge_table_bytes"):
        assert st[k] == 0, (k, st)
    return paths, lens, st


def coo_graph(oracle, e, s, d, w, directed):
    e.load_coo(s, d, w, directed=directed)
    return oracle.Graph.from_coo(s, d, w, directed=directed)


# ---- equalities with srw_walk -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karate", "rmat10w", "rmat10d"])
def test_where_the_filter_lets_everything_through_it_is_srw_walk_bit_for_bit(oracle, eng, name):
    e = eng
    if name == "karate":
        e.load_edgelist(KARATE, directed=False)
    else:
        s, d, w = rmat_lines(oracle, 10, edge_factor=8, weighted=name == "rmat10w")
        e.load_coo(s, d, w, directed=name == "rmat10d")
    V = e.vertices()
    for draws in (dict(rng="philox", seed=11), dict(rng="const", const_r=0.37)):
        kw = dict(walk_length=30, num_walks=3, first_walk=5, **draws)
        plain = e.walk(p=1.0, q=1.0, **kw)
        general = e.walk(p=1.0, q=1.0, force_general=True, **kw)
        assert_rows(general[:2], plain[:2], "the two forms of srw_walk")
        for types, pattern in (((V % 5).astype(np.uint8), [-1]), (np.full(len(V), 7, dtype=np.uint8), [7])):
            e.set_vertex_types(types)
            got = e.walk_metapath(pattern, **kw)
            assert_rows(got[:2], plain[:2], (name, pattern, draws))
            assert got[2]["n_steps"] == plain[2]["n_steps"] and got[2]["dead_ends"] == plain[2]["dead_ends"]
            assert got[2]["kernel_kind"] == 4 and got[2]["n_walkers"] == plain[2]["n_walkers"]


# ---- karate ---------------------------------------------------------------------------------------------------------------------------
def test_karate_patterns(oracle, eng):
    e = eng
    e.load_edgelist(KARATE, directed=False)
    g = oracle.Graph.load(KARATE, directed=False)
    V = g.vertices()
    assert np.array_equal(V, e.vertices())
    m64 = [j % 3 for j in range(64)]
    cases = [(2, [0, 1], 80), (3, [0, 1, 2], 80), (3, [0, -1, 2, -1], 80), (3, m64, 80), (3, m64, 20), (3, [1, 2, 0], 80)]
    full = 0
    for mod, pattern, L in cases:
        types = (V % mod).astype(np.uint8)
        e.set_vertex_types(types)
        assert e.vertex_types_len() == len(V)
        for draws in (dict(rng="philox", seed=42), dict(rng="const", const_r=0.0), dict(rng="const", const_r=1.0)):
            paths, lens, st = check(oracle, e, g, types, pattern, "karate", walk_length=L, num_walks=4, **draws)
            full += int((lens == L + 2).sum())
            tp = types[np.searchsorted(V, np.where(paths >= 0, paths, V[0]))]
            want = np.array([pattern[j % len(pattern)] for j in range(L + 2)])
            ok = (paths < 0) | (want[None, :] < 0) | (tp == want[None, :])
            assert ok[lens > 1].all()
    assert full > 0


# ---- hand-made rows -----------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 70001]
# matching entries at the start / at the end of the row: 4, 8 and 64 unit weights put const_r = .25 and .5 exactly on a boundary
RUN = {1: 1, 2: 1, 63: 4, 64: 8, 65: 64, 255: 64, 256: 8, 257: 4, 1023: 64, 70001: 64}


def hub_graph(n, leaf_w=None):
    """A (id 0) -> H (id 1) -> leaves 2 .. n + 1 in row order; directed, the leaves have no row."""
    s = np.concatenate([[0], np.full(n, 1)]).astype(np.int32)
    d = np.concatenate([[1], np.arange(2, n + 2)]).astype(np.int32)
    w = np.concatenate([[1.0], np.ones(n) if leaf_w is None else leaf_w]).astype(np.float32)
    return s, d, w


def placements(n):
    k = np.arange(n)
    return {"end": k >= n - RUN[n], "start": k < RUN[n], "third": k % 3 == 2 if n >= 3 else k == n - 1, "none": np.zeros(n, dtype=bool)}


@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_hub_rows_every_placement_of_the_matching_entries(oracle, eng, n):
    """Sources H and A, pattern [-1, 1, 1], walk_length 1: the hub's row is filtered at step 1 (from H) and at step 2 (from A)."""
    e = eng
    s, d, w = hub_graph(n)
    g = coo_graph(oracle, e, s, d, w, directed=True)
    for name, match in placements(n).items():
        types = np.concatenate([[9, 1], np.where(match, 1, 2)]).astype(np.uint8)
        e.set_vertex_types(types)
        for r in (0.0, 0.25, 0.5, 1.0):
            paths, lens, st = check(oracle, e, g, types, [-1, 1, 1], (n, name), sources=np.array([1, 0], dtype=np.int32), walk_length=1,
                                    rng="const", const_r=r)
            if name == "none":
                assert lens.tolist() == [1, 2] and st["dead_ends"] == 1          # stopped at s = 1 (not counted) and at s = 2
            else:
                assert lens.tolist() == [2, 3] and match[paths[0, 1] - 2] and paths[1, 2] == paths[0, 1]
                if r == 0.0:
                    assert paths[0, 1] - 2 == int(np.flatnonzero(match)[0])      # the first MATCHING entry, whatever the head is


def test_the_fallback_is_the_sublists_head_not_the_rows(oracle, eng):
    """const_r = 1 behind a head that does not match: 4 .. 10 unit weights (the oracle reaches 1 with 4, 5 and 8 of them and falls back
    to the head with 6, 7 and 10), and two weighted rows whose quotients do not reach 1 either.  One hub per row, all in one graph."""
    e = eng
    rows = [np.ones(c, dtype=np.float32) for c in (4, 5, 6, 7, 8, 10)]
    rows += [np.array(r, dtype=np.float32) for r in ([98.8, 46.6, 21.6], [61.2, 11.5, 4.4])]
    s, d, w, types, hubs = [], [], [], {}, []
    nxt = 100
    for i, rw in enumerate(rows):
        hub = i
        hubs.append(hub)
        types[hub] = 5
        for k, x in enumerate([1.0, 1.0] + rw.tolist() + [1.0]):      # two entries that do not match, the candidates, one more that does not
            s.append(hub); d.append(nxt); w.append(x)
            types[nxt] = 1 if 2 <= k < 2 + len(rw) else 2
            nxt += 1
    s, d, w = np.array(s, dtype=np.int32), np.array(d, dtype=np.int32), np.array(w, dtype=np.float32)
    g = coo_graph(oracle, e, s, d, w, directed=True)
    V = g.vertices()
    tv = np.array([types[int(v)] for v in V], dtype=np.uint8)
    e.set_vertex_types(tv)
    src = np.array(hubs, dtype=np.int32)
    paths, lens, st = check(oracle, e, g, tv, [5, 1], "fallback", sources=src, walk_length=0, rng="const", const_r=1.0)
    took = [int(np.flatnonzero(g.neighbors(h)[0] == paths[i, 1])[0]) - 2 for i, h in enumerate(hubs)]      # position in the sublist
    want = [oracle.sample_index(rw, 1.0) for rw in rows]
    assert took == want
    assert [t == 0 for t in took] == [False, False, True, True, False, True, True, True], took
    assert st["fallbacks"] > 0


def test_irregular_weights_take_the_exact_chain(oracle, eng):
    e = eng
    rng = np.random.default_rng(23)
    pool = np.array([1e-8, 3e-5, 0.5, 1.0, 3.25, 1000.0, 3e7, 0.0], dtype=np.float32)
    s, d, w, tl = [], [], [], []
    hubs, nxt = [], 1000
    for hub, n in enumerate((5, 40, 64, 65, 300, 1500)):
        hubs.append(hub)
        ww = rng.choice(pool, size=n)
        tt = rng.integers(1, 3, size=n)
        tt[n // 2], ww[n // 2] = 1, 0.0                                # a matching entry of weight zero
        for k in range(n):
            s.append(hub); d.append(nxt + k); w.append(ww[k]); tl.append(tt[k])
        nxt += n
    s, d, w = np.array(s, dtype=np.int32), np.array(d, dtype=np.int32), np.array(w, dtype=np.float32)
    g = coo_graph(oracle, e, s, d, w, directed=True)
    tv = np.concatenate([np.full(len(hubs), 7), np.array(tl)]).astype(np.uint8)
    assert len(tv) == g.num_vertices
    e.set_vertex_types(tv)
    src = np.array(hubs, dtype=np.int32)
    _, _, st = check(oracle, e, g, tv, [7, 1], "irregular", sources=src, walk_length=0, num_walks=40, rng="philox", seed=3)
    assert st["fallbacks"] > 0, st
    for r in (0.0, 1.0, 0.5):
        check(oracle, e, g, tv, [7, 1], "irregular", sources=src, walk_length=0, rng="const", const_r=r)


# ---- kinds of graph ---------------------------------------------------------------------------------------------------------------------
def test_unit_weight_graph_after_a_biased_walk_built_its_id_rows(oracle, eng):
    e = eng
    s, d, _ = rmat_lines(oracle, 9, edge_factor=8, weighted=False)
    g = coo_graph(oracle, e, s, d, None, directed=False)
    e.walk(fetch=False, p=0.25, q=4.0, walk_length=4)                  # (its tables bring the 4-byte id rows of a unit-weight graph)
    V = g.vertices()
    types = (V % 3).astype(np.uint8)
    e.set_vertex_types(types)
    check(oracle, e, g, types, [0, 1, 2], "unit", walk_length=12, num_walks=2, rng="philox", seed=9)
    check(oracle, e, g, types, [-1, 1], "unit", walk_length=12, rng="const", const_r=0.5)


def test_multi_edges_and_self_loops(oracle, eng):
    e = eng
    s, d, w = random_multigraph(np.random.default_rng(5), 60, 900, True, id_lo=3)
    g = coo_graph(oracle, e, s, d, w, directed=False)
    V = g.vertices()
    types = (V % 3).astype(np.uint8)
    e.set_vertex_types(types)
    for pattern in ([0, 1, 2], [2, -1], [1]):
        check(oracle, e, g, types, pattern, "multigraph", walk_length=16, num_walks=3, rng="philox", seed=2)
    check(oracle, e, g, types, [0, 1, 2], "multigraph", walk_length=16, rng="const", const_r=0.0)


def test_directed_graph_with_destination_only_vertices(oracle, eng):
    e = eng
    s, d, w = random_multigraph(np.random.default_rng(6), 300, 500, True, id_lo=10)
    g = coo_graph(oracle, e, s, d, w, directed=True)
    V = g.vertices()
    assert (np.array([g.degree(int(v)) for v in V]) == 0).any()
    types = (V % 2).astype(np.uint8)
    e.set_vertex_types(types)
    check(oracle, e, g, types, [0, 1], "directed", walk_length=10, num_walks=3, rng="philox", seed=4)
    check(oracle, e, g, types, [-1, 0], "directed", walk_length=10, num_walks=2, rng="philox", seed=4)


@pytest.mark.parametrize("sparse", [True, False])
def test_compacted_ids(oracle, sparse):
    s, d, w = random_multigraph(np.random.default_rng(7), 80, 700, True, id_lo=0)
    if sparse:
        s, d = ((x.astype(np.int64) * 20_000_003 - 1_000_000_000).astype(np.int32) for x in (s, d))       # a sparse id space, negative ids
        assert s.min() < 0
    with pkg().Engine(device=0, compact_ids=not sparse) as e:
        g = coo_graph(oracle, e, s, d, w, directed=False)
        V = g.vertices()
        assert np.array_equal(V, e.vertices())
        types = (np.arange(len(V)) % 3).astype(np.uint8)               # by POSITION in V
        e.set_vertex_types(types)
        check(oracle, e, g, types, [0, 1, 2], "compact", walk_length=14, num_walks=3, rng="philox", seed=8)
        src = np.array([V[3], V[0], V[3], V[len(V) - 1]], dtype=np.int32)
        check(oracle, e, g, types, [0, -1], "compact", sources=src, walk_length=14, num_walks=2, rng="philox", seed=8)


# ---- more walkers than waves in flight ----------------------------------------------------------------------------------------------------
def test_more_walkers_than_waves_in_flight(oracle, eng):
    e = eng
    s, d, w = rmat_lines(oracle, 12, edge_factor=8, weighted=True)
    g = coo_graph(oracle, e, s, d, w, directed=False)
    V = g.vertices()
    types = (V % 3).astype(np.uint8)
    pattern, L, iters = [0, 1, 2], 10, 4
    e.set_vertex_types(types)
    kw = dict(walk_length=L, num_walks=iters, rng="philox", seed=77)
    paths, lens, st = e.walk_metapath(pattern, **kw)
    nw = iters * len(V)
    # (RMAT-12 at edge factor 8 has 2 935 present vertices of its 4 096 ids: 11 740 walkers; the launch is capped at 8 blocks of 4 waves
    #  per CU, 8 192 waves on 256 CUs, so the cursor hands every wave more than one walker)
    assert st["n_walkers"] == nw == len(lens) and nw > 8 * 256 * 4
    only = np.unique(np.concatenate([[0, nw - 1], np.random.default_rng(1).choice(nw, size=2000, replace=False)]))
    ref = mref.walk(oracle, g, types, pattern, only=only, **kw)
    assert_rows((paths[only], lens[only]), (ref[0][only], ref[1][only]), "sampled walkers")
    # every walker: the properties
    assert st["n_steps"] == int((lens - 1).sum())
    assert st["dead_ends"] == int(((lens >= 2) & (lens < L + 2)).sum())
    col = np.arange(L + 2)[None, :]
    live = col < lens[:, None]
    assert (paths[~live] == -1).all() and (paths[live] >= 0).all()
    tp = types[np.searchsorted(V, np.where(live, paths, V[0]))]
    want = np.array([pattern[j % 3] for j in range(L + 2)])[None, :]
    walked = lens > 1
    assert (tp == want)[live & walked[:, None]].all()
    assert (types[np.searchsorted(V, paths[~walked, 0])] != 0).any()   # wrong-typed sources: the one-entry path
    keys = np.unique(np.concatenate([(s.astype(np.int64) << 32) | d, (d.astype(np.int64) << 32) | s]))
    hop = live[:, 1:]
    a, b = paths[:, :-1][hop].astype(np.int64), paths[:, 1:][hop].astype(np.int64)
    assert np.isin((a << 32) | b, keys).all()


# ---- sources ------------------------------------------------------------------------------------------------------------------------------
def test_typed_start_lists(oracle, eng):
    e = eng
    e.load_edgelist(KARATE, directed=False)
    g = oracle.Graph.load(KARATE, directed=False)
    V = g.vertices()
    types = (V % 2).astype(np.uint8)
    e.set_vertex_types(types)
    evens, odds = V[V % 2 == 0], V[V % 2 == 1]
    S = np.array([evens[3], evens[0], odds[1], evens[3], evens[-1]], dtype=np.int32)      # duplicates and an entry of the wrong type
    kw = dict(walk_length=12, num_walks=3, first_walk=1, rng="philox", seed=5)
    a = check(oracle, e, g, types, [0, 1], "sources=", sources=S, **kw)
    assert e.sources_len() is None
    assert a[1].reshape(3, -1)[:, 2].tolist() == [1, 1, 1]
    assert np.array_equal(a[0].reshape(3, len(S), -1)[:, 0], a[0].reshape(3, len(S), -1)[:, 3])
    e.set_sources(S)
    try:
        paths, lens, st = e.walk_metapath([0, 1], **kw)
    finally:
        e.clear_sources()
    assert_rows((paths, lens), a[:2], "set_sources")
    full = e.walk_metapath([0, 1], **kw)
    idx = (np.arange(3)[:, None] * len(V) + np.searchsorted(V, S)[None, :]).reshape(-1)
    assert_rows((full[0][idx], full[1][idx]), a[:2], "rows of the full walk")


# ---- downstream ---------------------------------------------------------------------------------------------------------------------------
def test_downstream_calls_act_on_the_result(oracle, eng, tmp_path):
    import torch
    P = pkg()
    e = eng
    e.load_edgelist(KARATE, directed=False)
    g = oracle.Graph.load(KARATE, directed=False)
    V = g.vertices()
    types = (V % 2).astype(np.uint8)
    e.set_vertex_types(types)
    kw = dict(walk_length=10, num_walks=2, rng="philox", seed=6)
    st = e.walk_metapath([0, 1], fetch=False, **kw)
    ref = mref.walk(oracle, g, types, [0, 1], **kw)
    assert st["n_steps"] == ref[2]
    tp, tl = e.paths_tensor()
    assert np.array_equal(tp.cpu().numpy(), ref[0]) and np.array_equal(tl.cpu().numpy(), ref[1])
    rp, rl = torch.as_tensor(ref[0]).cuda(), torch.as_tensor(ref[1]).cuda()
    pos, neg = e.skipgram_batch(3, num_negatives=2, seed=4, exclude_window=True)
    pos2, neg2 = e.skipgram_batch(3, num_negatives=2, seed=4, exclude_window=True, paths=rp, lens=rl)
    assert pos.shape[0] > 0 and torch.equal(pos, pos2) and torch.equal(neg, neg2)
    assert torch.equal(e.visit_counts(), e.visit_counts(paths=rp, lens=rl))
    assert int(e.visit_counts().sum()) == int(ref[1].sum())
    e.write_paths(str(tmp_path / "dev"), n_parts=2)
    P.save_paths(ref[0], ref[1], str(tmp_path / "host"), n_parts=2)
    for part in ("part-00000", "part-00001"):
        a, b = (open(os.path.join(str(tmp_path / k), "path", part), "rb").read() for k in ("dev", "host"))
        assert a == b and (part != "part-00000" or len(a) > 0)


# ---- lifetime -----------------------------------------------------------------------------------------------------------------------------
def test_lifetime_of_the_types(oracle):
    P = pkg()
    with P.Engine(device=0) as e:
        assert e.vertex_types_len() == -1
        e.load_edgelist(KARATE, directed=False)
        g = oracle.Graph.load(KARATE, directed=False)
        V = g.vertices()
        kw = dict(walk_length=8, rng="philox", seed=1)
        with pytest.raises(P.SrwError, match="srw_walk_metapath.*no vertex types"):
            e.walk_metapath([-1], **kw)
        t2, t3 = (V % 2).astype(np.uint8), (V % 3).astype(np.uint8)
        e.set_vertex_types(t2)
        assert e.vertex_types_len() == len(V)
        check(oracle, e, g, t2, [0, 1], "first set", **kw)
        import torch
        e.set_vertex_types(torch.as_tensor(t3).cuda())                 # replaced by a second set (a device tensor this time)
        check(oracle, e, g, t3, [0, 1, 2], "second set", **kw)
        e.set_vertex_types(t3.tolist())                                # ... and a list
        check(oracle, e, g, t3, [0, 1, 2], "list", **kw)
        with pytest.raises(P.SrwError, match="srw_vertex_types_set: n = 33 types for 34 vertices"):
            e.set_vertex_types(t2[:-1])
        assert e.vertex_types_len() == len(V)
        check(oracle, e, g, t3, [0, 1, 2], "after a refused set", **kw)          # the previous types are still in force
        e.set_vertex_types(None)
        assert e.vertex_types_len() == -1
        with pytest.raises(P.SrwError, match="no vertex types"):
            e.walk_metapath([0, 1], **kw)
        e.set_vertex_types(None)                                       # clearing nothing is fine
        e.set_vertex_types(t2)
        e.load_edgelist(KARATE, directed=True)                         # a load drops them
        assert e.vertex_types_len() == -1
        with pytest.raises(P.SrwError, match="no vertex types"):
            e.walk_metapath([0, 1], **kw)
        gd = oracle.Graph.load(KARATE, directed=True)
        e.set_vertex_types(t2)
        check(oracle, e, gd, t2, [0, 1], "after the load", **kw)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_previous_walk_result_intact(oracle):
    P = pkg()
    L = P.lib()

    def raw(e, params, pattern, m=None, with_params=True, with_pattern=True):
        pat = (C.c_int32 * max(len(pattern), 1))(*pattern)
        st = P.WalkStats()
        rc = L.srw_walk_metapath(e.h, C.byref(params) if with_params else None, pat if with_pattern else None,
                                 len(pattern) if m is None else m, C.byref(st))
        return rc, L.srw_last_error(e.h).decode()

    with P.Engine(device=0) as e:
        ok = P.Engine.params(walk_length=6)
        rc, msg = raw(e, ok, [-1])
        assert rc == P.ERR_INVALID and msg.startswith("srw_walk_metapath") and "no graph" in msg
        assert L.srw_vertex_types_set(e.h, C.c_void_p(256), 34) == P.ERR_INVALID
        assert L.srw_last_error(e.h).decode().startswith("srw_vertex_types_set") and "no graph" in L.srw_last_error(e.h).decode()
        e.load_edgelist(KARATE, directed=False)
        V = e.vertices()
        before = e.walk(p=0.5, q=2.0, walk_length=9, num_walks=2, seed=3)
        rc, msg = raw(e, ok, [-1])
        assert rc == P.ERR_INVALID and "no vertex types" in msg                  # even for an all-wildcard pattern
        e.set_vertex_types((V % 2).astype(np.uint8))
        bad = [
            (dict(), [0, 1], dict(with_params=False), "params is null"),
            (dict(), [0, 1], dict(with_pattern=False), "pattern is null"),
            (dict(), [], dict(), "outside 1 .. 64"),
            (dict(), [0] * 65, dict(), "outside 1 .. 64"),
            (dict(), [0, 1], dict(m=-1), "outside 1 .. 64"),
            (dict(), [0, -2], dict(), r"pattern[1] = -2"),
            (dict(), [256, 0], dict(), r"pattern[0] = 256"),
            (dict(p=2.0), [0, 1], dict(), "p and q must both be 1"),
            (dict(q=0.5), [0, 1], dict(), "p and q must both be 1"),
            (dict(sampler="alias"), [0, 1], dict(), "sampler"),
            (dict(walk_length=-1), [0, 1], dict(), "walk_length"),
            (dict(num_walks=-1), [0, 1], dict(), "num_walks"),
        ]
        for kw, pattern, how, why in bad:
            rc, msg = raw(e, P.Engine.params(**dict(dict(walk_length=6), **kw)), pattern, **how)
            assert rc == P.ERR_INVALID and msg.startswith("srw_walk_metapath") and why in msg, (kw, pattern, how, msg)
        wp = P.Engine.params(walk_length=6)
        wp.rng_mode = 7
        rc, msg = raw(e, wp, [0, 1])
        assert rc == P.ERR_INVALID and msg.startswith("srw_walk_metapath") and "rng_mode" in msg
        # population 1 selected: both entries refuse, the types stay in force
        assert L.srw_shard_select(e.h, 1) == P.OK
        try:
            rc, msg = raw(e, ok, [0, 1])
            assert rc == P.ERR_INVALID and msg.startswith("srw_walk_metapath") and "population 1" in msg
            assert L.srw_vertex_types_set(e.h, None, 0) == P.ERR_INVALID
            assert L.srw_last_error(e.h).decode().startswith("srw_vertex_types_set")
        finally:
            assert L.srw_shard_select(e.h, 0) == P.OK
        assert e.vertex_types_len() == len(V)
        # ... and after all of them the previous result is where it was
        paths = np.empty_like(before[0]); lens = np.empty_like(before[1])
        e._ck(L.srw_fetch_paths(e.h, paths.ctypes.data_as(C.POINTER(C.c_int32)), lens.ctypes.data_as(C.POINTER(C.c_int32))))
        assert_rows((paths, lens), before[:2], "the result from before the refusals")
        assert e.device_paths()[2:] == (len(lens), 11)
        # flags are ignored; a valid call then replaces the result
        wp = P.Engine.params(walk_length=6, force_general=True, edge_tables=False)
        rc, msg = raw(e, wp, [0, 1])
        assert rc == P.OK, msg
        assert e.device_paths()[2:] == (len(V), 8)
    with P.Engine(device=0, rank=0, world=2) as e:                               # a sharded handle
        e.load_edgelist(KARATE, directed=False)
        rc, msg = raw(e, ok, [-1])
        assert rc == P.ERR_INVALID and msg.startswith("srw_walk_metapath") and "world == 1" in msg
        assert L.srw_vertex_types_set(e.h, C.c_void_p(256), 34) == P.ERR_INVALID
        assert "world == 1" in L.srw_last_error(e.h).decode()
        n = C.c_int64(0)
        assert L.srw_vertex_types(e.h, C.byref(n)) == P.OK and n.value == -1
