"""srw_load_coo_device: a graph from edge arrays that are already in device memory (torch tensors, int32 or int64, pairs of rows or one
[2, E] edge_index) is THE graph srw_load_coo builds from the same values on the host — same stats, vertices, rows (ids and weight
bits, in order) and therefore the same walks, row for row.  What that graph is, the oracle tests pin; karate is held against the
oracle here as well.  Engine.paths_tensor(): the last walk's result as torch tensors over the memory it already lives in.
Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import KARATE, ROOT
from helpers import pkg, random_multigraph
from test_sparse_ids import sparse_multigraph

pytestmark = pytest.mark.gpu

WALKS = [dict(p=1.0, q=1.0), dict(p=0.25, q=4.0), dict(p=0.5, q=1.0)]
WKW = dict(walk_length=12, num_walks=2, seed=13)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def engines():
    """(host-loaded, device-loaded): two handles that every whole-graph case loads anew"""
    a, b = pkg().Engine(device=0), pkg().Engine(device=0)
    yield a, b
    a.close(); b.close()


@pytest.fixture(scope="module")
def karate_lines():
    s, d, w, _ = pkg().parse_edgelist(KARATE)
    return s, d, w


def bits(w):
    return np.asarray(w, dtype=np.float32).view(np.uint32)


def same_neighbors(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def assert_same_graph(host, dev, what, vertices=None):
    assert dev.stats() == host.stats(), what
    hv, dv = host.vertices(), dev.vertices()
    assert np.array_equal(hv, dv), what
    for v in (hv if vertices is None else vertices).tolist():
        assert same_neighbors(host.neighbors(v), dev.neighbors(v)), (what, "row of vertex", v)


def assert_same_walks(host, dev, what):
    for kw in WALKS:
        hp, hl, hs = host.walk(**kw, **WKW)
        dp, dl, ds = dev.walk(**kw, **WKW)
        assert np.array_equal(hl, dl), (what, kw, "lens")
        bad = np.nonzero((hp != dp).any(axis=1))[0]
        assert bad.size == 0, (what, kw, "%d rows differ, first %d" % (bad.size, bad[0] if bad.size else -1))
        assert hs["n_steps"] == ds["n_steps"] and hs["n_walkers"] == ds["n_walkers"], (what, kw)


def forms(s, d, w):
    """the same lines as device tensors: name -> (src, dst) arguments of load_coo"""
    s64, d64 = torch.from_numpy(s.astype(np.int64)).to(DEV), torch.from_numpy(d.astype(np.int64)).to(DEV)
    return {
        "int32 pairs": (torch.from_numpy(s).to(DEV), torch.from_numpy(d).to(DEV)),
        "int64 pairs": (s64, d64),
        "int64 [2, E]": (torch.stack([s64, d64]), None),
        "int32 [2, E]": (torch.from_numpy(np.stack([s, d])).to(DEV), None),      # odd E: the second row starts on a 4-byte boundary
    }


def dev_w(w):
    return None if w is None else torch.from_numpy(w).to(DEV)


def multigraph(E, seed=0):
    """50 vertices: ids -20 .. 24 as sources and destinations (self-loops, duplicate lines, negative ids) and 40 .. 44 as destinations
    only; weights with a 0, a negative and a NaN among them."""
    rng = np.random.default_rng(1000 + E + seed)
    s, d, _ = random_multigraph(rng, 45, E, False, id_lo=-20)
    for k in range(2, E, 11):
        d[k] = 40 + (k // 11) % 5
    w = rng.choice(np.array([0.5, 1.0, 2.0, 3.25], dtype=np.float32), size=E)
    for k, x in enumerate((0.0, -1.5, np.nan)):
        if E > 3 * k + 1:
            w[3 * k + 1] = x
    if E == 1:
        w[0] = 0.0
    return s, d, w


def ingest_pass(id_bytes):
    """ids of one column that ONE pass of k_coo_ingest's grid-stride loop covers: blocks x threads x ids per 16-byte vector"""
    src = open(os.path.join(ROOT, "stellar-random-walk_amd", "csrc", "coo_ingest.hip")).read()
    c = {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("INGEST_TPB", "INGEST_BLOCKS_PER_CU", "INGEST_VEC_BYTES")}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * c["INGEST_BLOCKS_PER_CU"] * c["INGEST_TPB"] * (c["INGEST_VEC_BYTES"] // id_bytes)


# ---- karate: every form, against the host load and the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("weighted", [True, False])
def test_karate_from_device_tensors(engines, oracle, karate_lines, directed, weighted):
    host, dev = engines
    s, d, w = karate_lines
    w = w if weighted else None
    host.load_coo(s, d, w, directed=directed)
    g = oracle.Graph.load(KARATE, directed=directed)
    assert host.stats() == (34, 78 if directed else 156)
    for name, (ts, td) in forms(s, d, w).items():
        assert dev.load_coo(ts, td, dev_w(w), directed=directed) is dev
        assert_same_graph(host, dev, ("karate", name))
        assert_same_walks(host, dev, ("karate", name))
        for kw in WALKS:
            paths, lens, st = dev.walk(**kw, **WKW)
            rp, rl, rs = g.walk(**kw, **WKW)
            assert np.array_equal(lens, rl) and np.array_equal(paths, rp) and st["n_steps"] == rs, (name, kw)


# ---- random multigraphs at the sizes where the head / tail of a column, the wave reduction and the grid stride can go wrong --------------
@pytest.mark.parametrize("E", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025])
def test_multigraphs_from_edge_index_tensors(engines, E):
    host, dev = engines
    s, d, w = multigraph(E)
    directed = E not in (64, 1023)                 # (directed: 40 .. 44 are destinations only)
    host.load_coo(s, d, w, directed=directed)
    f = forms(s, d, w)
    for name in ("int32 [2, E]", "int64 [2, E]"):
        ei = f[name][0]
        tw = dev_w(w)
        before, wbits = ei.clone(), tw.view(torch.int32).clone()
        dev.load_coo(ei, None, tw, directed=directed)
        assert torch.equal(ei, before) and torch.equal(tw.view(torch.int32), wbits), "the caller's arrays were written"
        assert_same_graph(host, dev, (E, name))
        assert_same_walks(host, dev, (E, name))
    # the rows of an int32 [2, E + 1] tensor from its second column on: BOTH rows start off a 16-byte boundary
    wide = torch.from_numpy(np.stack([np.concatenate([[7], s]), np.concatenate([[7], d])]).astype(np.int32)).to(DEV)
    dev.load_coo(wide[0, 1:], wide[1, 1:], dev_w(w), directed=directed)
    assert_same_graph(host, dev, (E, "int32 rows at +4 bytes"))


@pytest.mark.parametrize("dtype,passes", [("int32", 1), ("int32", 2), ("int64", 1), ("int64", 2)])
def test_multigraphs_beyond_one_pass_of_the_ingest_grid(engines, dtype, passes):
    """E just above blocks x threads x ids per vector (the first lanes take a second pass), and above twice that (every lane does)."""
    host, dev = engines
    E = passes * ingest_pass(4 if dtype == "int32" else 8) + (1 if passes == 1 else 77)
    s, d, w = multigraph(E)
    s[E - 1], d[0] = -33, 47                       # the extremes: the very last source, the very first destination
    host.load_coo(s, d, w, directed=True)
    ei = torch.from_numpy(np.stack([s, d]).astype(dtype)).to(DEV)
    dev.load_coo(ei, None, dev_w(w), directed=True)
    assert dev.vertices()[0] == -33 and dev.vertices()[-1] == 47
    assert_same_graph(host, dev, (E, dtype))
    assert_same_walks(host, dev, (E, dtype))


# ---- the smallest / largest id where only one lane sees it ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("where", ["first", "last", "tail"])
def test_extremes_are_found_wherever_they_sit(engines, dtype, where):
    """E = 1027: the first row of the [2, E] tensor has 256 whole vectors and a tail of 3 (int32) or 1 (int64) ids; the second row starts
    off a 16-byte boundary (a head) and ends in a tail of 2 (int32) or none.  `tail`: the element behind the last whole vector of row 0."""
    host, dev = engines
    E = 1027
    base_s, base_d, w = multigraph(E)
    tail = {"int32": 1024, "int64": 1026}[dtype]
    for extreme in (-1000, 1000):                  # the minimum, then the maximum, on that one element only
        s, d = base_s.copy(), base_d.copy()
        if where == "first":
            s[0] = extreme
        elif where == "last":
            d[E - 1] = extreme
        else:
            s[tail] = extreme
        host.load_coo(s, d, w, directed=True)
        ei = torch.from_numpy(np.stack([s, d]).astype(dtype)).to(DEV)
        dev.load_coo(ei, None, dev_w(w), directed=True)
        verts = dev.vertices()
        assert (verts[0] if extreme < 0 else verts[-1]) == extreme, (where, dtype, extreme)
        assert_same_graph(host, dev, (where, dtype, extreme))
    assert_same_walks(host, dev, (where, dtype))


# ---- a sparse id space: compact_ids rewrites its arguments, the caller's tensors stay as they were -------------------------------------------
@pytest.mark.parametrize("dtype", ["int64", "int32"])
def test_sparse_ids_from_a_device_tensor(dtype):
    P = pkg()
    s, d, w = sparse_multigraph(6, n_vertices=70, n_lines=200)
    assert min(s.min(), d.min()) == -2**31 and max(s.max(), d.max()) == 2**31 - 1
    with P.Engine(device=0, compact_ids=True) as host, P.Engine(device=0, compact_ids=True) as dev:
        host.load_coo(s, d, w)
        ei = torch.from_numpy(np.stack([s, d]).astype(dtype)).to(DEV)
        before = ei.clone()
        dev.load_coo(ei, None, dev_w(w))
        assert torch.equal(ei, before), "compact_ids rewrote the caller's tensor"
        assert_same_graph(host, dev, ("sparse", dtype))
        for v in (5, 123456789):
            assert same_neighbors(host.neighbors(v), dev.neighbors(v))
        assert_same_walks(host, dev, ("sparse", dtype))
    with P.Engine(device=0) as host, P.Engine(device=0) as dev:                 # without the flag: sparse by its spread
        host.load_coo(s, d, w, directed=True)
        dev.load_coo(torch.from_numpy(np.stack([s, d]).astype(dtype)).to(DEV), None, dev_w(w), directed=True)
        assert_same_graph(host, dev, ("sparse, no flag", dtype))
        assert_same_walks(host, dev, ("sparse, no flag", dtype))


# ---- errors leave the handle as it was -------------------------------------------------------------------------------------------------
def test_an_int64_id_outside_int32_is_named_and_nothing_changes(engines, karate_lines):
    P = pkg()
    _, dev = engines
    s, d, w = karate_lines
    dev.load_coo(torch.from_numpy(s).to(DEV), torch.from_numpy(d).to(DEV))
    dev.set_sources([1, 34, 2])
    want = [dev.walk(**kw, **WKW)[:2] for kw in WALKS]
    a = torch.from_numpy(np.stack([s, d]).astype(np.int64)).to(DEV)
    a[1, 7] = 2**31
    b = a.clone()
    b[0, 3] = -2**31 - 1
    for t, line, col, bad_id in ((a, 7, "dst", 2**31), (b, 3, "src", -2**31 - 1)):
        with pytest.raises(P.SrwError) as ei:
            dev.load_coo(t)
        msg = str(ei.value)
        assert ei.value.code == P.ERR_INVALID, msg
        assert ("line %d " % line) in msg and ("%s id %d " % (col, bad_id)) in msg, msg
    L = P.lib()
    p = C.c_void_p(a.data_ptr())
    assert L.srw_load_coo_device(dev.h, p, p, None, -1, P.IDS_I64, 0) == P.ERR_INVALID        # n_lines < 0
    assert L.srw_load_coo_device(dev.h, p, p, None, 5, 2, 0) == P.ERR_INVALID                 # an unknown id_type
    assert L.srw_load_coo_device(dev.h, None, p, None, 5, P.IDS_I64, 0) == P.ERR_INVALID
    assert L.srw_load_coo_device(dev.h, p, None, None, 5, P.IDS_I32, 0) == P.ERR_INVALID
    # the graph loaded before — and the list of sources checked against it — still stand
    assert dev.stats() == (34, 156) and dev.sources_len() == 3
    for kw, (wp, wl) in zip(WALKS, want):
        gp, gl, _ = dev.walk(**kw, **WKW)
        assert np.array_equal(gp, wp) and np.array_equal(gl, wl), kw
    dev.clear_sources()


def test_bad_tensors_are_type_errors_and_cpu_tensors_take_the_host_path(engines, karate_lines):
    host, dev = engines
    s, d, w = karate_lines
    host.load_coo(s, d, w)
    dev.load_coo(s, d, w)
    ei = torch.from_numpy(np.stack([s, d]).astype(np.int64)).to(DEV)
    pid = np.zeros(len(s), dtype=np.int32)
    for args, kw in (((ei.t().contiguous().t(),), {}), ((ei[0][::2], ei[1][::2]), {}), ((ei.to(torch.float32),), {}), ((ei[0], ei[1][:-1]), {}),
                     ((ei[0], ei[1].to(torch.int32)), {}), ((ei,), dict(pid=pid)), ((ei[0], ei[1]), dict(pid=pid)), ((ei[0], ei[1].cpu()), {}),
                     ((ei,), dict(w=torch.ones(len(s) - 1, device=DEV)))):
        with pytest.raises(TypeError):
            dev.load_coo(*args, **kw)
    assert_same_graph(host, dev, "after the refused tensors")
    # CPU tensors: .numpy() and the host entry point, partition ids allowed
    dev.load_coo([1, 2], [2, 3])
    dev.load_coo(torch.from_numpy(np.stack([s, d])), None, torch.from_numpy(w), pid=pid)
    assert_same_graph(host, dev, "cpu [2, E] tensor")
    assert dev.partition(1) == 0
    dev.load_coo(torch.from_numpy(s), torch.from_numpy(d))
    assert_same_graph(host, dev, "cpu pairs")
    # a weight tensor of another dtype is converted on the device
    w2 = (np.arange(len(s)) % 5 + 1).astype(np.float32)
    host.load_coo(s, d, w2)
    dev.load_coo(ei, None, torch.from_numpy(w2.astype(np.float64)).to(DEV))
    assert_same_graph(host, dev, "float64 weights")
    dev.load_coo(ei, w=w2)                                                     # ... and host weights go up with the tensors
    assert_same_graph(host, dev, "numpy weights")


def test_an_empty_edge_index_is_the_empty_graph(engines):
    host, dev = engines
    host.load_coo(np.zeros(0, np.int32), np.zeros(0, np.int32))
    dev.load_coo(torch.empty((2, 0), dtype=torch.int64, device=DEV))
    assert dev.stats() == host.stats() == (0, 0)
    assert len(dev.vertices()) == 0
    paths, lens, st = dev.walk(**WKW)
    assert len(paths) == 0 and len(lens) == 0 and st["n_walkers"] == 0


def test_a_device_load_clears_the_sources(engines, karate_lines):
    _, dev = engines
    s, d, _ = karate_lines
    ei = torch.from_numpy(np.stack([s, d])).to(DEV)
    dev.load_coo(ei)
    dev.set_sources([5, 6, 6])
    assert dev.sources_len() == 3
    dev.load_coo(ei)
    assert dev.sources_len() is None
    assert dev.walk(fetch=False, walk_length=3)["n_walkers"] == 34
    dev.set_sources([5])
    dev.load_coo(torch.empty((2, 0), dtype=torch.int32, device=DEV))
    assert dev.sources_len() is None


# ---- vertex-sharded handles: the blocked, owner-filtered build from slices of the caller's arrays ---------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_handles_build_the_same_shards(world):
    P = pkg()
    s, d, w = multigraph(1025, seed=world)
    all_v = np.unique(np.concatenate([s, d]))
    f = forms(s, d, w)
    for r in range(world):
        with P.Engine(device=0, rank=r, world=world) as host, P.Engine(device=0, rank=r, world=world) as dev:
            host.load_coo(s, d, w, directed=True)
            for name in ("int32 [2, E]", "int64 [2, E]"):
                dev.load_coo(f[name][0], None, dev_w(w), directed=True)
                assert dev.shard_capacity() == host.shard_capacity(), (world, r, name)
                n_local = host.shard_capacity()[0]
                ranks = []
                for e in (host, dev):
                    out = np.full(max(n_local, 1), -1, dtype=np.int32)
                    assert P.lib().srw_shard_vertex_ranks(e.h, out.ctypes.data_as(C.POINTER(C.c_int32))) == P.OK
                    ranks.append(out[:n_local])
                assert np.array_equal(ranks[0], ranks[1]), (world, r, name)
                assert_same_graph(host, dev, (world, r, name), vertices=all_v)
    # (every shard together holds every vertex once)
    assert len(all_v) == 50


# ---- the result side ---------------------------------------------------------------------------------------------------------------------
def test_paths_tensor_views_the_result_in_place(engines, karate_lines):
    _, dev = engines
    s, d, _ = karate_lines
    dev.load_coo(torch.from_numpy(np.stack([s, d])).to(DEV))
    paths, lens, st = dev.walk(p=0.25, q=4.0, **WKW)
    tp, tl = dev.paths_tensor()
    dp, dl, n, stride = dev.device_paths()
    assert (tp.data_ptr(), tl.data_ptr()) == (dp, dl)
    assert tp.dtype == torch.int32 and tl.dtype == torch.int32 and tp.is_cuda and tl.is_cuda and tp.device.index == 0
    assert tuple(tp.shape) == (st["n_walkers"], 12 + 2) == (n, stride) and tuple(tl.shape) == (st["n_walkers"],) and n == 68
    assert np.array_equal(tp.cpu().numpy(), paths) and np.array_equal(tl.cpu().numpy(), lens)
    # a tensor among tensors: the lengths recomputed from the -1 tails on the device
    assert torch.equal((tp >= 0).sum(dim=1).to(torch.int32), tl)
    dev.walk(fetch=False, sources=[], **WKW)
    tp, tl = dev.paths_tensor()
    assert tp.numel() == 0 and tl.numel() == 0 and tp.dtype == torch.int32 and tl.dtype == torch.int32
    assert tp.dim() == 2 and tl.dim() == 1
