"""The vertex-sharded cluster walk from a caller-supplied list of start vertices (srw_cluster_set_sources).  Every walker of every
case is compared, bit for bit, with the CPU oracle's walk(sources=...), with the row the same cluster's full walk produces for that
(iteration, source) and with the whole-graph engine's list walk: a draw is keyed by (seed, iteration, source id, step), each shard
seeds the entries of the list it owns, and row lw of a shard leaves for canonical walker iteration * n + position in the list.
Every cluster is Cluster([0] * world): virtual shards on one device.  Run on the MI355X box with `pytest -m gpu`."""
import os

import numpy as np
import pytest

from conftest import KARATE, TESTGRAPH
from helpers import pkg, random_multigraph, rmat_lines

pytestmark = pytest.mark.gpu

PQ = [(1.0, 1.0), (0.25, 1.0), (0.25, 4.0), (4.0, 0.5)]
DRAWS = [dict(rng="philox", seed=11), dict(rng="const", const_r=0.37)]
WORLDS = [1, 2, 3, 8]
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def make_graph(oracle, name):
    """-> (load(cluster or engine), oracle graph)"""
    rng = np.random.default_rng(5)
    if name in ("karate", "karate_directed", "testgraph"):
        path, directed = (TESTGRAPH if name == "testgraph" else KARATE), name != "karate"
        return (lambda e: e.load_edgelist(path, directed=directed)), oracle.Graph.load(path, directed=directed)
    if name == "multigraph":
        s, d, w = random_multigraph(rng, 80, 900, True, id_lo=3)
        return (lambda e: e.load_coo(s, d, w, directed=False)), oracle.Graph.from_coo(s, d, w, directed=False)
    sc, directed, weighted = {"rmat14wd": (14, True, True), "rmat15": (15, False, False)}[name]
    s, d, w = rmat_lines(oracle, sc, edge_factor=8, weighted=weighted)
    return (lambda e: e.load_coo(s, d, w, directed=directed)), oracle.Graph.from_coo(s, d, w, directed=directed)


def make_list(rng, g, n_random):
    """Random order, duplicates, the top-degree hub twice, and a destination-only vertex where the graph has one."""
    verts = g.vertices()
    deg = np.array([g.degree(int(v)) for v in verts])
    pick = rng.choice(verts, size=n_random, replace=True)
    extra = [verts[int(np.argmax(deg))]] * 2 + [pick[0], pick[0]]
    dest_only = verts[deg == 0]
    if len(dest_only):
        extra += [dest_only[0], dest_only[-1]]
    S = np.concatenate([pick, np.array(extra, dtype=np.int32)]).astype(np.int32)
    rng.shuffle(S)
    return S, len(dest_only)


def assert_rows(got, want, what):
    (gp, gl), (wp, wl) = got, want
    assert gp.shape == wp.shape and gl.shape == wl.shape, (what, gp.shape, wp.shape)
    assert np.array_equal(gl, wl), ("lens differ", what)
    bad = np.nonzero((gp != wp).any(axis=1))[0]
    assert bad.size == 0, "paths differ %s: %d walkers, first %d\n got=%s\nwant=%s" % (what, bad.size, bad[0], gp[bad[0]], wp[bad[0]])


def rows_of_full(full_p, full_l, verts, S, num_walks):
    """full[it * nV + rank(S[i])] for every (it, i), in the list walk's order"""
    nv, rank = len(verts), np.searchsorted(verts, S)
    assert np.array_equal(verts[rank], S)
    idx = (np.arange(num_walks)[:, None] * nv + rank[None, :]).reshape(-1)
    return full_p[idx], full_l[idx]


def fetch(cl, n, stride):
    """srw_cluster_fetch_paths into buffers of n rows"""
    P = pkg()
    paths, lens = np.empty((max(n, 1), stride), dtype=np.int32), np.empty(max(n, 1), dtype=np.int32)
    cl._ck(P.lib().srw_cluster_fetch_paths(cl.h, P._i32(paths), P._i32(lens)))
    return paths[:n], lens[:n]


def all_vertices(cl):
    return np.sort(np.concatenate([cl.shard(r).vertices() for r in range(cl.world)]))


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karate", "karate_directed", "testgraph", "multigraph", "rmat14wd", "rmat15"])
def test_cluster_list_walk_equals_the_oracle(oracle, name):
    load, g = make_graph(oracle, name)
    big = name.startswith("rmat")
    S, n_dest_only = make_list(np.random.default_rng(17), g, 300 if big else 40)
    if name in ("karate_directed", "testgraph", "rmat14wd"):
        assert n_dest_only > 0, "the case is meant to have a destination-only vertex"
    L = 24 if big else 12
    cases = [dict(p=p, q=q, walk_length=L, num_walks=3, first_walk=2, **draws) for p, q in PQ for draws in DRAWS]
    refs = [g.walk(sources=S, threads=8, **kw) for kw in cases]
    for world in WORLDS:
        with pkg().Cluster([0] * world) as cl:
            load(cl)
            assert cl.sources_len() is None
            for kw, (rp, rl, rs) in zip(cases, refs):
                paths, lens, st = cl.walk(sources=S, **kw)
                assert_rows((paths, lens), (rp, rl), (name, world, kw))
                assert st["n_walkers"] == 3 * len(S) and st["n_steps"] == rs, (name, world, kw, st)
                assert cl.sources_len() is None                    # sources= holds for the call
            if n_dest_only:                                        # a destination-only vertex walks the one-entry path [v]
                verts = g.vertices()
                v = int(verts[[g.degree(int(x)) == 0 for x in verts]][0])
                paths, lens, _ = cl.walk(sources=[v], walk_length=5, num_walks=2)
                assert lens.tolist() == [1, 1] and paths[:, 0].tolist() == [v, v] and (paths[:, 1:] == -1).all()


# ---- 2. against the full walk of the same cluster and the whole-graph engine, kernel family by kernel family --------------------
def _lists(rng, verts, hub):
    rnd = rng.choice(verts, size=min(500, 2 * len(verts)), replace=True).astype(np.int32)
    return {"random": np.concatenate([rnd, [hub, hub]]).astype(np.int32), "thrice": rng.permutation(np.tile(verts, 3)).astype(np.int32),
            "one": np.array([hub], dtype=np.int32)}


def _families():
    ss = lambda st: st["strategy_steps"]                                                     # noqa: E731
    tab = lambda st: ss(st)["edge_table"] + ss(st)["edge_mask"]                              # noqa: E731
    return [
        # name, walk kwargs, draws, check(stats) for any list, check(stats) for lists of more than one walker
        ("first_order_linked", dict(p=1.0, q=1.0), ["philox"], lambda st: st["kernel_kind"] == 1, None),
        ("first_order_unlinked", dict(p=1.0, q=1.0, compact=False), ["philox", "const"], lambda st: st["kernel_kind"] == 1, None),
        ("first_order_unlinked_const", dict(p=1.0, q=1.0), ["const"], lambda st: st["kernel_kind"] == 1, None),
        ("force_general", dict(p=1.0, q=1.0, force_general=True), ["philox", "const"],
         lambda st: st["kernel_kind"] == 2 and tab(st) == 0 and ss(st)["q1_lane"] == 0, None),
        ("q1_lane", dict(p=0.25, q=1.0), ["philox"], lambda st: st["kernel_kind"] == 2 and st["edge_tables"] == 0, lambda st: ss(st)["q1_lane"] > 0),
        ("tables", dict(p=0.25, q=4.0), ["philox", "const"], lambda st: st["kernel_kind"] == 2 and st["edge_tables"] > 0, None),
        ("tables_directed_pq", dict(p=4.0, q=0.5), ["philox"], lambda st: st["kernel_kind"] == 2 and st["edge_tables"] > 0, lambda st: tab(st) > 0),
        ("tables_off", dict(p=0.25, q=4.0, edge_tables=False), ["philox", "const"],
         lambda st: st["kernel_kind"] == 2 and st["edge_tables"] == 0 and tab(st) == 0, None),
    ]


def _draw_kw(d):
    return dict(rng="philox", seed=23) if d == "philox" else dict(rng="const", const_r=0.61)


@pytest.mark.parametrize("graph,world", [("karate", 2), ("rmat14wd", 3), ("rmat14wd", 8)])
def test_cluster_list_rows_equal_the_full_walk_rows(oracle, graph, world):
    load, g = make_graph(oracle, graph)
    rng = np.random.default_rng(29)
    P = pkg()
    strict = graph != "karate"      # (karate is too small to be sure of tables / the per-lane step: there a list walk runs what the full walk ran)
    sig = lambda st: (st["kernel_kind"], st["edge_tables"] > 0, st["strategy_steps"]["q1_lane"] > 0)   # noqa: E731
    with P.Cluster([0] * world) as cl, P.Engine(device=0) as eng:
        load(cl)
        load(eng)
        verts = all_vertices(cl)
        assert np.array_equal(verts, g.vertices()) and np.array_equal(verts, eng.vertices())
        hub = verts[int(np.argmax([g.degree(int(v)) for v in verts]))]
        lists = _lists(rng, verts, hub)
        for fam, kw, draws, check, check_many in _families():
            for d in draws:
                wkw = dict(walk_length=20, num_walks=3, first_walk=2, **kw, **_draw_kw(d))
                full_p, full_l, st_full = cl.walk(**wkw)
                if strict:
                    assert check(st_full) and (check_many is None or check_many(st_full)), (graph, fam, d, st_full)
                assert st_full["n_walkers"] == 3 * len(verts)
                for lname, S in lists.items():
                    paths, lens, st = cl.walk(sources=S, **wkw)
                    assert st["n_walkers"] == 3 * len(S)
                    if strict:
                        assert check(st), (graph, fam, d, lname, st)
                        if check_many is not None and len(S) > 1:
                            assert check_many(st), (graph, fam, d, lname, st)
                    elif len(S) > 1:
                        assert sig(st) == sig(st_full), (graph, fam, d, lname, st, st_full)
                    assert_rows((paths, lens), rows_of_full(full_p, full_l, verts, S, 3), (graph, world, fam, d, lname, "full walk"))
                    ep, el, est = eng.walk(sources=S, **wkw)
                    assert_rows((paths, lens), (ep, el), (graph, world, fam, d, lname, "whole-graph engine"))
                    assert st["n_steps"] == est["n_steps"]


# ---- 3. batching, populations, the streamed way out -----------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("p,q", [(1.0, 1.0), (0.25, 4.0)])
def test_cluster_list_batches_and_populations(oracle, world, p, q):
    """num_walks = 5: batch 1 is one population per batch, 2 and 5 split a batch into two populations (world > 1), 0 is automatic."""
    load, g = make_graph(oracle, "karate_directed")
    S, _ = make_list(np.random.default_rng(43), g, 30)
    kw = dict(p=p, q=q, walk_length=15, num_walks=5, first_walk=2, seed=9)
    rp, rl, rs = g.walk(sources=S, **kw)
    with pkg().Cluster([0] * world) as cl:
        load(cl)
        cl.set_sources(S)
        for batch in (1, 2, 5, 0):
            paths, lens, st = cl.walk(batch=batch, **kw)
            assert_rows((paths, lens), (rp, rl), (world, p, q, batch))
            assert st["n_walkers"] == 5 * len(S) and st["n_steps"] == rs
        assert cl.sources_len() == len(S)


@pytest.mark.parametrize("world", [2, 8])
def test_cluster_walk_and_save_with_a_list(oracle, tmp_path, monkeypatch, world):
    load, g = make_graph(oracle, "karate_directed")
    S, _ = make_list(np.random.default_rng(41), g, 25)
    n = len(S)
    kw = dict(p=0.25, q=4.0, walk_length=15, num_walks=4, first_walk=2, seed=9)
    rp, rl, rs = g.walk(sources=S, **kw)
    P = pkg()
    with P.Cluster([0] * world) as cl, P.Engine(device=0) as eng:
        load(cl)
        load(eng)
        for n_parts in (1, 7):
            for slice_rows in ("", "5"):                     # the default slice holds the whole list; slices of 5 list positions
                if slice_rows:
                    monkeypatch.setenv("SRW_CLUSTER_SLICE_ROWS", slice_rows)
                else:
                    monkeypatch.delenv("SRW_CLUSTER_SLICE_ROWS", raising=False)
                out = tmp_path / ("o%d%s" % (n_parts, slice_rows))
                st = cl.walk_and_save(str(out), n_parts=n_parts, sources=S, **kw)
                assert st["n_walkers"] == 4 * n and st["n_steps"] == rs
                assert cl.sources_len() is None
                ref, ref2 = tmp_path / ("r%d%s" % (n_parts, slice_rows)), tmp_path / ("e%d%s" % (n_parts, slice_rows))
                oracle.write_paths(rp, rl, str(ref), n_parts=n_parts)
                eng.walk_and_save(str(ref2), n_parts=n_parts, sources=S, **kw)
                names = sorted(x for x in os.listdir(ref / "path") if x.startswith("part-"))
                assert len(names) == n_parts and names == sorted(x for x in os.listdir(out / "path") if x.startswith("part-"))
                for x in names:
                    assert (out / "path" / x).read_bytes() == (ref / "path" / x).read_bytes(), x
                    assert (out / "path" / x).read_bytes() == (ref2 / "path" / x).read_bytes(), x
                assert b"".join((out / "path" / x).read_bytes() for x in names).count(b"\n") == 4 * n
                assert (out / "path" / "_SUCCESS").read_bytes() == b""
        monkeypatch.delenv("SRW_CLUSTER_SLICE_ROWS", raising=False)
        # walk_and_save keeps no result: fetch keeps failing as the valid flag says
        with pytest.raises(P.SrwError) as ei:
            fetch(cl, 4 * n, 17)
        assert "no walk result" in str(ei.value)


# ---- 4. skew --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(1.0, 1.0), (0.25, 4.0)])
def test_cluster_skewed_lists(oracle, p, q):
    """Every source on one shard of eight: that shard seeds everything (the others nothing), its seeds need world x the chunk room of
    an even list.  Short (the 4096-record floor covers it) and tiled until batch * n / world is well past the floor."""
    s, d, w = rmat_lines(oracle, 13, edge_factor=8, weighted=True)
    P = pkg()
    rng = np.random.default_rng(53)
    with P.Cluster([0] * 8) as cl, P.Engine(device=0) as eng:
        cl.load_coo(s, d, w)
        eng.load_coo(s, d, w)
        verts = eng.vertices()
        mine = cl.shard(5).vertices()
        assert 0 < len(mine) < len(verts) / 4
        lists = {"one_shard": rng.permutation(mine).astype(np.int32),
                 "one_shard_tiled": rng.permutation(np.tile(mine, 24000 // len(mine) + 1)).astype(np.int32),
                 "one_entry": mine[:1].astype(np.int32),
                 "thrice": rng.permutation(np.tile(verts, 3)).astype(np.int32)}
        assert len(lists["one_shard_tiled"]) >= 24000
        for lname, S in lists.items():
            for batch in (0, 1):
                kw = dict(p=p, q=q, walk_length=12, num_walks=4, first_walk=1, seed=77)
                paths, lens, st = cl.walk(sources=S, batch=batch, **kw)
                ep, el, est = eng.walk(sources=S, **kw)
                assert_rows((paths, lens), (ep, el), (lname, p, q, batch))
                assert st["n_walkers"] == 4 * len(S) and st["n_steps"] == est["n_steps"]


# ---- 5. owner maps --------------------------------------------------------------------------------------------------------------
def test_cluster_list_under_other_owner_maps(oracle):
    """owner(v) = nonNegativeMod(v, world) (the HashPartitioner table) and the partition ids of a VCut input: the resolve kernel asks the
    shard's own owner map, so every entry of the list is kept by exactly the shard that holds its row."""
    s, d, w = rmat_lines(oracle, 11, edge_factor=8, weighted=True)
    pid = (d.astype(np.int64) % 5).astype(np.int32)
    g = oracle.Graph.from_coo(s, d, w)
    S, _ = make_list(np.random.default_rng(59), g, 400)
    P = pkg()
    for p, q in ((1.0, 1.0), (0.5, 2.0)):
        kw = dict(p=p, q=q, walk_length=12, num_walks=3, first_walk=2, seed=4)
        rp, rl, rs = g.walk(sources=S, threads=8, **kw)
        owned = {}
        for name, ckw, lkw in (("mixed", {}, {}), ("hash_partitioner", dict(hash_partitioner=True), {}),
                               ("partitions", dict(owner_from_partitions=True), dict(pid=pid))):
            with P.Cluster([0] * 3, **ckw) as cl:
                cl.load_coo(s, d, w, **lkw)
                owned[name] = [len(cl.shard(r).vertices()) for r in range(3)]
                paths, lens, st = cl.walk(sources=S, **kw)
                assert_rows((paths, lens), (rp, rl), (name, p, q))
                assert st["n_walkers"] == 3 * len(S) and st["n_steps"] == rs
        assert owned["mixed"] != owned["hash_partitioner"] and owned["mixed"] != owned["partitions"], owned   # (the maps do differ)


# ---- 6. sparse ids: the shards compact them, the list is spelled in the input's ids -----------------------------------------------
@pytest.mark.parametrize("world,p,q,directed", [(2, 1.0, 1.0, False), (3, 0.25, 4.0, False), (4, 4.0, 0.5, True), (2, 0.5, 1.0, False)])
def test_cluster_list_sparse_ids(oracle, world, p, q, directed):
    rng = np.random.default_rng(20 + world)
    s, d, w = random_multigraph(rng, 90, 700, True)
    ids = np.unique(np.concatenate([rng.integers(I32_MIN, I32_MAX, size=86, dtype=np.int64), np.array([I32_MIN, I32_MAX, -1, 0], dtype=np.int64)]))
    while ids.size < 90:
        ids = np.unique(np.concatenate([ids, rng.integers(I32_MIN, I32_MAX, size=4, dtype=np.int64)]))
    ids = rng.permutation(ids).astype(np.int32)
    s, d = ids[s], ids[d]
    g = oracle.Graph.from_coo(s, d, w, directed=directed)
    S, _ = make_list(rng, g, 60)
    S = np.concatenate([S, np.array([I32_MIN, I32_MAX], dtype=np.int32)]) if {I32_MIN, I32_MAX} <= set(g.vertices().tolist()) else S
    kw = dict(p=p, q=q, walk_length=11, num_walks=3, first_walk=2, seed=9)
    rp, rl, rs = g.walk(sources=S, **kw)
    P = pkg()
    with P.Cluster([0] * world) as cl:
        cl.load_coo(s, d, w, directed=directed)
        for batch in (0, 1, 2):
            paths, lens, st = cl.walk(sources=S, batch=batch, **kw)
            assert_rows((paths, lens), (rp, rl), (world, batch))
            assert st["n_steps"] == rs
        absent = int(np.setdiff1d(np.arange(-50, 50), g.vertices())[0])       # inside the id range, no vertex, no slot
        with pytest.raises(P.SrwError) as ei:
            cl.set_sources([int(S[0]), absent])
        assert ei.value.code == P.ERR_INVALID and ("id %d at position 1" % absent) in str(ei.value)


# ---- 7. state -------------------------------------------------------------------------------------------------------------------
def test_cluster_sources_state(oracle, tmp_path):
    P = pkg()
    ks, kd, kwt, _ = P.parse_edgelist(KARATE)
    ks, kd, kwt = np.append(ks, 40).astype(np.int32), np.append(kd, 41).astype(np.int32), np.append(kwt, 1.0).astype(np.float32)
    g = oracle.Graph.from_coo(ks, kd, kwt)                          # karate + the edge (40, 41): ids 35 .. 39 are inside the id range and no vertices
    nv = 36
    kw = dict(walk_length=8, num_walks=2, seed=3)
    with P.Cluster([0] * 3) as cl, P.Engine(device=0) as eng:
        with pytest.raises(P.SrwError) as ei:                      # no graph loaded
            cl.set_sources([1])
        assert ei.value.code == P.ERR_INVALID
        cl.load_coo(ks, kd, kwt)
        assert cl.stats()[0] == nv
        assert cl.sources_len() is None
        A, B = [34, 1, 1, 17], [5, 5, 9]
        cl.set_sources(A)
        assert cl.sources_len() == 4
        paths, lens, st = cl.walk(**kw)
        assert_rows((paths, lens), g.walk(sources=A, **kw)[:2], "set")
        # a set drops the held result; the next walk brings one back
        cl.set_sources(A)
        with pytest.raises(P.SrwError) as ei:
            fetch(cl, 2 * 4, 10)
        assert ei.value.code == P.ERR_INVALID and "no walk result" in str(ei.value)
        # sources= holds for one call and restores the list that was in force
        paths, lens, st = cl.walk(sources=B, **kw)
        assert st["n_walkers"] == 2 * len(B)
        assert_rows((paths, lens), g.walk(sources=B, **kw)[:2], "sources=")
        assert cl.sources_len() == 4
        paths, lens, st = cl.walk(**kw)
        assert_rows((paths, lens), g.walk(sources=A, **kw)[:2], "restored")
        # unknown ids: inside the id range and far outside it; the first bad id and its position; the old list stays in force everywhere
        for bad_list, bad_id, pos in (([1, 2, 37, 36, 3], 37, 2), ([1, 2_000_000_000, -7], 2_000_000_000, 1), ([-2**31, 40], -2**31, 0), ([40, 41, 0], 0, 2)):
            with pytest.raises(P.SrwError) as ei:
                cl.set_sources(bad_list)
            assert ei.value.code == P.ERR_INVALID and ("id %d at position %d" % (bad_id, pos)) in str(ei.value), str(ei.value)
            assert cl.sources_len() == 4
            paths, lens, st = cl.walk(**kw)
            assert_rows((paths, lens), g.walk(sources=A, **kw)[:2], ("after a refused list", bad_list))
        with pytest.raises(TypeError):
            cl.set_sources([1.5])
        with pytest.raises(ValueError):
            cl.set_sources([2**31])
        # a shard on its own still refuses a list
        with pytest.raises(P.SrwError) as ei:
            cl.shard(1).set_sources([1, 2])
        assert ei.value.code == P.ERR_INVALID and "world == 1" in str(ei.value)
        # the empty list: zero walkers, an empty but complete output directory
        cl.set_sources([])
        assert cl.sources_len() == 0
        paths, lens, st = cl.walk(**kw)
        assert paths.shape == (0, 10) and lens.shape == (0,) and st["n_walkers"] == 0 and st["n_steps"] == 0
        st = cl.walk_and_save(str(tmp_path / "empty"), n_parts=3, **kw)
        assert st["n_walkers"] == 0
        eng.load_coo(ks, kd, kwt)
        eng.walk_and_save(str(tmp_path / "empty_ref"), n_parts=3, sources=[], **kw)
        names = sorted(os.listdir(tmp_path / "empty" / "path"))
        assert "_SUCCESS" in names and names == sorted(os.listdir(tmp_path / "empty_ref" / "path"))
        assert all((tmp_path / "empty" / "path" / x).read_bytes() == b"" for x in names)
        # clear: every vertex again
        cl.clear_sources()
        assert cl.sources_len() is None
        paths, lens, st = cl.walk(**kw)
        assert st["n_walkers"] == 2 * nv
        assert_rows((paths, lens), g.walk(**kw)[:2], "cleared")
        # a load clears the list
        cl.set_sources(A)
        cl.load_edgelist(KARATE, directed=True)
        assert cl.sources_len() is None and all(cl.shard(r).sources_len() is None for r in range(3))
        assert cl.walk(fetch=False, **kw)["n_walkers"] == 2 * 34
        cl.set_sources(A)
        cl.generate_rmat(8, 8 << 8, seed=2)
        assert cl.sources_len() is None
