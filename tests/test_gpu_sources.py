"""Walks from a caller-supplied list of start vertices (srw_set_sources): EVERY walker of every case below is compared, bit for bit,
with the CPU oracle's walk(sources=...) and with the row the same handle's full walk produces for that (iteration, source) — a draw
is keyed by (seed, iteration, source id, step), never by the walker's position in the launch.  Walker = iteration * n + position in
the list.  Run on the MI355X box with `pytest -m gpu`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import KARATE, TESTGRAPH
from helpers import digest, pkg, random_multigraph, rmat_lines

pytestmark = pytest.mark.gpu

PQ = [(1.0, 1.0), (0.25, 1.0), (0.25, 4.0), (4.0, 0.5)]
DRAWS = [dict(rng="philox", seed=11), dict(rng="const", const_r=0.37)]


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


def make_graph(oracle, name):
    """-> (Engine kwargs, load(engine), oracle graph)"""
    rng = np.random.default_rng(5)
    if name in ("karate", "karate_directed", "testgraph"):
        path, directed = (TESTGRAPH if name == "testgraph" else KARATE), name != "karate"
        return {}, (lambda e: e.load_edgelist(path, directed=directed)), oracle.Graph.load(path, directed=directed)
    if name in ("multigraph", "multigraph_far_ids"):
        far = name == "multigraph_far_ids"
        # (the far-id case is directed and thin: it has destination-only vertices)
        s, d, w = random_multigraph(rng, 300, 500, True, id_lo=1_900_000_000) if far else random_multigraph(rng, 80, 900, True, id_lo=3)
        directed = far
        return (dict(compact_ids=True) if far else {}), (lambda e: e.load_coo(s, d, w, directed=directed)), \
            oracle.Graph.from_coo(s, d, w, directed=directed)
    sc, directed, weighted = {"rmat14wd": (14, True, True), "rmat15": (15, False, False), "rmat16d": (16, True, False)}[name]
    s, d, w = rmat_lines(oracle, sc, edge_factor=8, weighted=weighted)
    return {}, (lambda e: e.load_coo(s, d, w, directed=directed)), oracle.Graph.from_coo(s, d, w, directed=directed)


def make_list(rng, g, n_random):
    """Random order, duplicates, the hub, and a destination-only vertex where the graph has one."""
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


# ---- 5. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karate", "karate_directed", "testgraph", "multigraph", "multigraph_far_ids", "rmat14wd", "rmat15", "rmat16d"])
def test_list_walk_equals_the_oracle(oracle, name):
    ekw, load, g = make_graph(oracle, name)
    rng = np.random.default_rng(17)
    big = name.startswith("rmat")
    S, n_dest_only = make_list(rng, g, 300 if big else 40)
    if name in ("karate_directed", "testgraph", "multigraph_far_ids", "rmat14wd", "rmat16d"):
        assert n_dest_only > 0, "the case is meant to have a destination-only vertex"
    L = 24 if big else 12
    with pkg().Engine(device=0, **ekw) as e:
        load(e)
        assert e.sources_len() is None
        for p, q in PQ:
            for draws in DRAWS:
                kw = dict(p=p, q=q, walk_length=L, num_walks=3, first_walk=2, **draws)
                rp, rl, rs = g.walk(sources=S, threads=8, **kw)
                paths, lens, st = e.walk(sources=S, **kw)
                assert_rows((paths, lens), (rp, rl), (name, p, q, draws))
                assert st["n_walkers"] == 3 * len(S) and st["n_steps"] == rs
                assert e.sources_len() is None                     # sources= holds for the call
            kw = dict(p=p, q=q, walk_length=L, num_walks=3, first_walk=2, seed=11)
            rp, rl, rs = g.walk(sources=S, threads=8, sampler=1, **kw)
            paths, lens, st = e.walk(sources=S, sampler="alias", **kw)      # Mode A: keyed (iteration, source, step, trial)
            assert_rows((paths, lens), (rp, rl), (name, p, q, "alias"))
            assert st["kernel_kind"] == 3 and st["n_steps"] == rs
        # a destination-only vertex walks the one-entry path [v]
        if n_dest_only:
            verts = g.vertices()
            v = int(verts[[g.degree(int(x)) == 0 for x in verts]][0])
            paths, lens, _ = e.walk(sources=[v], walk_length=5, num_walks=2)
            assert lens.tolist() == [1, 1] and paths[:, 0].tolist() == [v, v] and (paths[:, 1:] == -1).all()


# ---- 6. against the full walk of the same handle, kernel family by kernel family --------------------------------------------------
def _lists(rng, verts, hub):
    rnd = rng.choice(verts, size=min(500, 2 * len(verts)), replace=True).astype(np.int32)
    return {"random": np.concatenate([rnd, [hub, hub]]).astype(np.int32), "thrice": rng.permutation(np.tile(verts, 3)).astype(np.int32),
            "one": np.array([hub], dtype=np.int32)}


def _families():
    ss = lambda st: st["strategy_steps"]                                                     # noqa: E731
    return [
        # name, walk kwargs, draws it applies to, check(stats) for any list, check(stats) for lists of more than one walker
        ("first_order_compact", dict(p=1.0, q=1.0), ["philox"], lambda st: st["kernel_kind"] == 1 and st["record_bytes"] == 16, None),
        ("first_order", dict(p=1.0, q=1.0, compact=False), ["philox", "const"], lambda st: st["kernel_kind"] == 1 and st["record_bytes"] == 32, None),
        ("force_general", dict(p=1.0, q=1.0, force_general=True), ["philox", "const"], lambda st: st["kernel_kind"] == 2, None),
        ("q1_lane", dict(p=0.25, q=1.0), ["philox"], lambda st: st["kernel_kind"] == 2, lambda st: ss(st)["q1_lane"] > 0),
        ("tables_off", dict(p=0.25, q=4.0, edge_tables=False), ["philox", "const"],
         lambda st: st["kernel_kind"] == 2 and st["edge_tables"] == 0 and ss(st)["edge_table"] == 0, None),
        ("alias", dict(p=0.25, q=4.0, sampler="alias"), ["philox"], lambda st: st["kernel_kind"] == 3, lambda st: st["trials"] > 0),
        ("alias_q1", dict(p=4.0, q=1.0, sampler="alias"), ["philox"], lambda st: st["kernel_kind"] == 3, None),
    ]


def _draw_kw(d):
    return dict(rng="philox", seed=23) if d == "philox" else dict(rng="const", const_r=0.61)


@pytest.mark.parametrize("graph", ["karate", "rmat14wd", "multigraph_far_ids"])
def test_list_rows_equal_the_full_walk_rows(oracle, graph):
    """karate and the weighted directed RMAT-14 qualify for every kernel family (asserted from the stats of the full walk AND of each list
    walk); the weighted multigraph with far, compacted ids may be refused the 16-byte records — there a list walk must run the family
    the full walk of the same call ran."""
    ekw, load, g = make_graph(oracle, graph)
    rng = np.random.default_rng(29)
    strict = graph != "multigraph_far_ids"
    sig = lambda st: (st["kernel_kind"], st["record_bytes"], st["edge_tables"] > 0, st["strategy_steps"]["q1_lane"] > 0)   # noqa: E731
    with pkg().Engine(device=0, **ekw) as e:
        load(e)
        verts = e.vertices()
        assert np.array_equal(verts, g.vertices())
        hub = verts[int(np.argmax([g.degree(int(v)) for v in verts]))]
        lists = _lists(rng, verts, hub)
        assert len(lists["thrice"]) == 3 * len(verts) > len(verts)
        for fam, kw, draws, check, check_many in _families():
            for d in draws:
                wkw = dict(walk_length=20, num_walks=3, first_walk=2, **kw, **_draw_kw(d))
                full_p, full_l, st_full = e.walk(**wkw)
                if strict:
                    assert check(st_full) and (check_many is None or check_many(st_full)), (graph, fam, d, st_full)
                assert st_full["n_walkers"] == 3 * len(verts)
                for lname, S in lists.items():
                    paths, lens, st = e.walk(sources=S, **wkw)
                    assert st["n_walkers"] == 3 * len(S)
                    if strict:
                        assert check(st), (graph, fam, d, lname, st)
                        if check_many is not None and len(S) > 1:
                            assert check_many(st), (graph, fam, d, lname, st)
                    elif len(S) > 1:
                        assert sig(st) == sig(st_full), (graph, fam, d, lname, st, st_full)
                    assert_rows((paths, lens), rows_of_full(full_p, full_l, verts, S, 3), (graph, fam, d, lname))


TABLE_KERNELS = [{}, {"SRW_TABLE_LANES": "-1"}]


@pytest.mark.parametrize("kernel", TABLE_KERNELS)
@pytest.mark.parametrize("graph", ["multigraph_all", "rmat14_generated"])
def test_list_rows_equal_the_full_walk_rows_per_edge_tables(monkeypatch, graph, kernel):
    """Per-edge tables, under both forms of the table walk (one walker per lane — the default here — and per wave):
    the small graph with a table for every certified pair (edge_tables_all), weighted RMAT-14 with the default selection."""
    rng = np.random.default_rng(31)
    with pkg().Engine(device=0) as e:
        if graph == "multigraph_all":
            s, d, w = random_multigraph(np.random.default_rng(11), 80, 900, True, id_lo=3)
            e.load_coo(s, d, w, directed=False)
            extra = dict(edge_tables_all=True)
        else:
            e.generate_rmat(14, 16 << 14, seed=9, weighted=True)
            extra = {}
        verts = e.vertices()
        lists = _lists(rng, verts, verts[0])
        for d in ("philox", "const"):
            for p, q in [(0.25, 4.0), (4.0, 0.5)]:
                wkw = dict(p=p, q=q, walk_length=40 if d == "philox" else 12, num_walks=3, first_walk=2, **extra, **_draw_kw(d))
                full_p, full_l, st_full = e.walk(**wkw)                       # the default kernel: results never depend on the form
                assert st_full["edge_tables"] > 0 and (d == "const" or st_full["strategy_steps"]["edge_table"] > 0), st_full
                for k, v in kernel.items(): monkeypatch.setenv(k, v)
                try:
                    for lname, S in lists.items():
                        paths, lens, st = e.walk(sources=S, **wkw)
                        assert st["n_walkers"] == 3 * len(S) and st["edge_tables"] > 0, (graph, kernel, lname, st)
                        if len(S) > 1 and d == "philox":
                            assert st["strategy_steps"]["edge_table"] > 0, (graph, kernel, lname, st)
                        assert_rows((paths, lens), rows_of_full(full_p, full_l, verts, S, 3), (graph, kernel, d, p, q, lname))
                finally:
                    for k in kernel: monkeypatch.delenv(k)


def test_boundary_draws_of_a_list_walk_go_through_the_tie_kernels(monkeypatch):
    """SRW_DEBUG_CHAIN_DEG: every table step on a long row is treated as a boundary draw — the tie records (iteration, source, prev, curr)
    of a list walk, the chain kernels and the redo in the general kernel must give the full walk's rows."""
    rng = np.random.default_rng(37)
    monkeypatch.setenv("SRW_DEBUG_CHAIN_DEG", "600")
    with pkg().Engine(device=0) as e:
        e.generate_rmat(13, 16 << 13, seed=9, weighted=True)
        verts = e.vertices()
        wkw = dict(p=0.25, q=4.0, walk_length=40, num_walks=3, first_walk=2, seed=5)
        full_p, full_l, st_full = e.walk(**wkw)
        assert st_full["strategy_steps"]["handed_over_walkers"] > 0, st_full
        for lname, S in _lists(rng, verts, verts[0]).items():
            paths, lens, st = e.walk(sources=S, **wkw)
            if lname == "thrice":
                assert st["strategy_steps"]["handed_over_walkers"] > 0, (lname, st)
            assert_rows((paths, lens), rows_of_full(full_p, full_l, verts, S, 3), lname)


# ---- 7. the streamed entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,sampler", [(1.0, 1.0, "reference"), (0.25, 4.0, "reference"), (4.0, 0.5, "alias")])
def test_walk_to_host_and_walk_and_save_with_a_list(eng, oracle, tmp_path, p, q, sampler):
    ekw, load, g = make_graph(oracle, "karate_directed")
    load(eng)
    S, _ = make_list(np.random.default_rng(41), g, 25)
    n, stride = len(S), 17
    kw = dict(p=p, q=q, walk_length=15, num_walks=4, first_walk=2, seed=9, sampler=sampler)
    rp, rl, rs = g.walk(sources=S, **dict(kw, sampler=1 if sampler == "alias" else 0))
    eng.set_sources(S)
    try:
        assert eng.sources_len() == n
        paths, lens, st = eng.walk(**kw)
        assert_rows((paths, lens), (rp, rl), "walk")
        for pinned in (True, False):
            hp, hl, hst = eng.walk_to_host(pinned=pinned, **kw)
            assert_rows((hp, hl), (paths, lens), ("walk_to_host", pinned))
            assert hst["n_walkers"] == 4 * n and hst["n_steps"] == rs
        want_dead = [int(((rl[i * n:(i + 1) * n] >= 2) & (rl[i * n:(i + 1) * n] < stride)).sum()) for i in range(4)]
        assert sum(want_dead) > 0                      # (directed karate: the count is not vacuous)
        for device_format in (False, True):
            for n_parts in (1, 5):
                out = tmp_path / ("o%d%d" % (device_format, n_parts))
                sst, dead = eng.walk_and_save(str(out), n_parts=n_parts, device_format=device_format, **kw)
                assert sst["n_walkers"] == 4 * n and sst["n_steps"] == rs and dead == want_dead
                pkg().save_paths(paths, lens, str(tmp_path / ("r%d%d" % (device_format, n_parts))), n_parts=n_parts)
                names = sorted(x for x in os.listdir(out / "path") if x.startswith("part-"))
                assert len(names) == n_parts
                got = b"".join((out / "path" / x).read_bytes() for x in names)
                ref = b"".join((tmp_path / ("r%d%d" % (device_format, n_parts)) / "path" / x).read_bytes() for x in names)
                assert got == ref and got.count(b"\n") == 4 * n
                assert (out / "path" / "_SUCCESS").read_bytes() == b""
        # the resident result of the list walk, written by srw_write_paths
        eng.walk(fetch=False, **kw)
        eng.write_paths(str(tmp_path / "w"), n_parts=3)
        got = b"".join((tmp_path / "w" / "path" / ("part-%05d" % k)).read_bytes() for k in range(3))
        assert got == "".join("\t".join(str(int(x)) for x in r[:m]) + "\n" for r, m in zip(rp, rl)).encode()
    finally:
        eng.clear_sources()


# ---- 8. ids already on the device ------------------------------------------------------------------------------------------------
def test_set_sources_with_a_device_tensor(eng, oracle):
    import torch
    ekw, load, g = make_graph(oracle, "multigraph")
    load(eng)
    S, _ = make_list(np.random.default_rng(43), g, 60)
    kw = dict(p=0.25, q=4.0, walk_length=12, num_walks=3, first_walk=2, seed=3)
    host = eng.walk(sources=S, **kw)
    t = torch.from_numpy(S).to("cuda:0")
    assert t.dtype == torch.int32
    eng.set_sources(t)
    try:
        assert eng.sources_len() == len(S)
        dev = eng.walk(**kw)
        assert_rows(dev[:2], host[:2], "device tensor")
        for bad in (t.to(torch.int64), t.to(torch.float32), torch.from_numpy(S).to(torch.int64)):
            with pytest.raises(TypeError):
                eng.set_sources(bad)
        assert eng.sources_len() == len(S)
        again = eng.walk(**kw)
        assert_rows(again[:2], host[:2], "after the refused tensors")
        # an unknown id in a device list: named with its position, the list in force stays
        t2 = t.clone(); t2[7] = 2; t2[9] = 1          # (the multigraph's ids start at 3)
        with pytest.raises(pkg().SrwError) as ei:
            eng.set_sources(t2)
        assert ei.value.code == pkg().ERR_INVALID and "id 2 " in str(ei.value) and "position 7" in str(ei.value)
        assert_rows(eng.walk(**kw)[:2], host[:2], "after the refused device list")
        # sources= with a tensor for one call: the list from before is back afterwards
        one = eng.walk(sources=t[:5].contiguous(), **kw)
        assert one[2]["n_walkers"] == 15 and eng.sources_len() == len(S)
        assert_rows(eng.walk(**kw)[:2], host[:2], "restored")
    finally:
        eng.clear_sources()


# ---- 9. state -------------------------------------------------------------------------------------------------------------------
def test_sources_state(eng, oracle, tmp_path):
    P = pkg()
    with P.Engine(device=0) as fresh:
        with pytest.raises(P.SrwError) as ei:
            fresh.set_sources([1])
        assert ei.value.code == P.ERR_INVALID and "no graph" in str(ei.value)
    eng.load_edgelist(KARATE)
    g = oracle.Graph.load(KARATE)
    kw = dict(p=0.5, q=2.0, walk_length=10, num_walks=2, seed=6)
    full = eng.walk(**kw)
    S = np.array([34, 1, 1, 7, 20], dtype=np.int32)
    eng.set_sources(S)
    a = eng.walk(**kw)
    assert_rows(a[:2], g.walk(sources=S, **kw)[:2], "karate list")
    for bad_list, bad_id, pos in (([3, 35, 0], 35, 1), ([0], 0, 0), ([1, 2, -5, 99], -5, 2), ([2147483647], 2147483647, 0)):
        with pytest.raises(P.SrwError) as ei:
            eng.set_sources(bad_list)
        assert ei.value.code == P.ERR_INVALID, ei.value
        assert ("id %d " % bad_id) in str(ei.value) and ("position %d" % pos) in str(ei.value), str(ei.value)
        assert eng.sources_len() == len(S)
    assert_rows(eng.walk(**kw)[:2], a[:2], "the previous list is still in force")
    with pytest.raises(TypeError):
        eng.set_sources(np.array([1.0, 2.0]))
    # a list walk feeds everything downstream of a finished walk: the scan sums and the embedding stage
    assert eng.result_scan_sums()[2] == a[2]["n_steps"]
    ids, vec = eng.w2v_fit_device(dim=8, window=3, iterations=1, seed=2, threads=1)
    on_paths = set(int(x) for r, m in zip(a[0], a[1]) for x in r[:m])
    assert sorted(ids.tolist()) == sorted(on_paths) and vec.shape == (len(on_paths), 8)
    # n = 0: zero walkers, an empty part-00000 + _SUCCESS
    eng.set_sources([])
    assert eng.sources_len() == 0
    paths, lens, st = eng.walk(**kw)
    assert len(paths) == 0 and len(lens) == 0 and st["n_walkers"] == 0
    hp, hl, hst = eng.walk_to_host(**kw)
    assert len(hp) == 0 and hst["n_walkers"] == 0
    for device_format in (False, True):
        out = tmp_path / ("empty%d" % device_format)
        sst, dead = eng.walk_and_save(str(out), n_parts=1, device_format=device_format, **kw)
        assert sst["n_walkers"] == 0 and dead == [0, 0]
        assert sorted(os.listdir(out / "path")) == ["_SUCCESS", "part-00000"] and (out / "path" / "part-00000").read_bytes() == b""
    # clear: the full walk again
    eng.clear_sources()
    assert eng.sources_len() is None
    again = eng.walk(**kw)
    assert digest(again[0], again[1]) == digest(full[0], full[1]) and again[2]["n_walkers"] == 2 * 34
    # every load clears the list
    loads = [lambda: eng.load_edgelist(KARATE), lambda: eng.load_coo([1, 2], [2, 3]), lambda: eng.load_adjacency([(1, [(2, 1.0)]), (2, [(1, 1.0)])]),
             lambda: eng.generate_rmat(8, 8 << 8, seed=1)]
    for load in loads:
        eng.load_edgelist(KARATE)
        eng.set_sources([5, 6])
        assert eng.sources_len() == 2
        load()
        assert eng.sources_len() is None
        assert eng.walk(fetch=False, walk_length=3)["n_walkers"] == eng.num_vertices


def test_sharded_handles_refuse_a_list():
    P = pkg()
    with P.Engine(device=0, rank=0, world=2) as e:
        e.load_edgelist(KARATE)
        with pytest.raises(P.SrwError) as ei:
            e.set_sources([1, 2])
        assert ei.value.code == P.ERR_INVALID and "world == 1" in str(ei.value)
        assert e.sources_len() is None
    with P.Cluster([0, 0]) as cl:
        cl.load_edgelist(KARATE)
        sh = cl.shard(1)
        with pytest.raises(P.SrwError) as ei:
            sh.set_sources([1, 2])
        assert ei.value.code == P.ERR_INVALID
        paths, lens, st = cl.walk(walk_length=5, seed=3)
        assert st["n_walkers"] == 34


# ---- 10. the CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_sources_end_to_end(oracle, tmp_path):
    F = [34, 1, 1, 17, 2, 34, 9]
    f = tmp_path / "sources.txt"
    f.write_text("34 1\n1\t17\n\n2 34 9")
    g = oracle.Graph.load(KARATE)
    for fmt in ("true", "false"):
        out = tmp_path / ("out_" + fmt)
        r = subprocess.run([pkg().CLI_PATH, "--cmd", "randomwalk", "--numWalks", "3", "--p", "0.5", "--q", "2", "--walkLength", "10",
                            "--input", KARATE, "--output", str(out), "--seed", "42", "--sources", str(f), "--deviceFormat", fmt],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == ["edges: 156", "vertices: 34", "E Partitions: 156", "V Partitions: 34"] + ["Unfinished Walkers: 0"] * 3
        lines = (out / "path" / "part-00000").read_text().splitlines()
        assert len(lines) == len(F) * 3 and [int(x.split("\t")[0]) for x in lines] == F * 3
        with pkg().Engine(device=0) as e:
            e.load_edgelist(KARATE)
            paths, lens, _ = e.walk(sources=F, p=0.5, q=2.0, walk_length=10, num_walks=3, seed=42)
        assert lines == ["\t".join(str(int(x)) for x in p[:n]) for p, n in zip(paths, lens)]
        rp, rl, _ = g.walk(sources=np.array(F, dtype=np.int32), p=0.5, q=2.0, walk_length=10, num_walks=3, seed=42)
        assert np.array_equal(paths, rp) and np.array_equal(lens, rl)
    # an id that is no vertex of the graph: the job fails and names it
    bad = tmp_path / "bad.txt"
    bad.write_text("1 2 77\n")
    r = subprocess.run([pkg().CLI_PATH, "--cmd", "randomwalk", "--input", KARATE, "--output", str(tmp_path / "out_bad"), "--sources", str(bad)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "id 77 at position 2" in r.stderr
    # --cmd node2vec trains on the list's walks only
    out = tmp_path / "n2v"
    r = subprocess.run([pkg().CLI_PATH, "--cmd", "node2vec", "--numWalks", "2", "--walkLength", "4", "--dim", "8", "--iter", "1", "--input", KARATE,
                        "--output", str(out), "--sources", str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = (out / "path" / "part-00000").read_text().splitlines()
    assert [int(x.split("\t")[0]) for x in lines] == F * 2
    vocab = sorted(int(x.split("\t")[0]) for x in (out / "vec" / "part-00000").read_text().splitlines())
    assert vocab == sorted(set(int(t) for x in lines for t in x.split("\t")))
