"""srw_sample_neighbors / Engine.sample_neighbors on the GPU: every element of every layer is held, exactly, against the numpy
restatement of the header comment (tests/neighbors_ref.py).  The inputs and the conditions they meet (the Floyd inputs collide, the
weighted inputs reach every arm of the draw) are those of tests/test_neighbors_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import neighbors_ref as nref
import test_neighbors_cpu as cases
from conftest import KARATE, ROOT
from helpers import pkg, random_multigraph

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def karate(oracle):
    return {d: oracle.Graph.load(KARATE, directed=d) for d in (False, True)}


def check(oracle, e, neighbors, seeds, fanouts, what="", **kw):
    """one call through Engine.sample_neighbors, every element and the unknown count against the restatement -> the layers (numpy)"""
    want, unknown, _ = nref.sample(oracle, neighbors, seeds, fanouts, **{k: v for k, v in kw.items() if k != "no_compact"})
    *got, n_unknown = e.sample_neighbors(seeds, fanouts, return_unknown=True, **kw)
    assert len(got) == len(fanouts) and n_unknown == unknown, (what, n_unknown, unknown)
    F = nref.row_lengths(fanouts)
    out = []
    for l, (g, w) in enumerate(zip(got, want), start=1):
        assert str(g.dtype) == "torch.int32" and tuple(g.shape) == (len(seeds), F[l]) and g.is_cuda and g.is_contiguous()
        g = g.cpu().numpy()
        assert np.array_equal(g, w), (what, fanouts, kw, "layer %d" % l, np.argwhere(g != w)[:6].tolist())
        out.append(g)
    return out


# ---- karate -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("replace", [True, False])
def test_karate(oracle, eng, karate, directed, replace):
    import torch
    g = karate[directed]
    eng.load_edgelist(KARATE, directed=directed)
    rows = nref.Rows(g.neighbors)
    seeds = cases.karate_seeds(g)
    for fanouts in cases.KARATE_FANOUTS:
        check(oracle, eng, rows, seeds, fanouts, "karate", seed=7, epoch=2, replace=replace)
    # the same seeds as a device tensor, int32 and int64, give the same layers as the host list
    a = eng.sample_neighbors(seeds, [3, 2], seed=7, replace=replace)
    for dt in (torch.int32, torch.int64):
        b = eng.sample_neighbors(torch.tensor(seeds, dtype=dt, device="cuda:0"), [3, 2], seed=7, replace=replace)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="outside int32"):
        eng.sample_neighbors(torch.tensor([0, 1 << 40], dtype=torch.int64, device="cuda:0"), [2])
    # zero seeds: empty layers of the right shapes, nothing unknown
    *empty, unknown = eng.sample_neighbors([], [3, 2], return_unknown=True, replace=replace)
    assert [tuple(x.shape) for x in empty] == [(0, 3), (0, 6)] and unknown == 0


def test_keying(oracle, eng, karate):
    """row b depends on (seed, epoch, b, its own seed vertex) and on nothing else in the batch"""
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices().tolist()
    seeds = V + V[:6]
    for replace in (True, False):
        kw = dict(seed=5, epoch=1, replace=replace)
        base = [x.cpu().numpy() for x in eng.sample_neighbors(seeds, [4, 3], **kw)]
        again = [x.cpu().numpy() for x in eng.sample_neighbors(seeds, [4, 3], **kw)]
        assert all(np.array_equal(a, b) for a, b in zip(base, again))                       # a repeat is bit for bit
        i = 9
        perm = list(reversed(seeds))
        perm[i] = seeds[i]                                                                   # every other seed moves, row i stays
        moved = [x.cpu().numpy() for x in eng.sample_neighbors(perm, [4, 3], **kw)]
        assert all(np.array_equal(a[i], b[i]) for a, b in zip(base, moved))
        assert any((a != b).any() for a, b in zip(base, moved))
        for other in (dict(kw, seed=6), dict(kw, epoch=2)):
            diff = [x.cpu().numpy() for x in eng.sample_neighbors(seeds, [4, 3], **other)]
            assert any((a != b).any() for a, b in zip(base, diff)), other
        # a vertex that occurs twice gets independent children
        assert any((a[:6] != a[len(V):]).any() for a in base)


# ---- rows of every kind, with replacement -------------------------------------------------------------------------------------------------
def test_weighted_rows_through_both_record_forms(oracle, eng):
    rows = cases.weighted_rows()
    eng.load_adjacency(rows)
    provider = cases.rows_provider(rows)
    for v, nb in rows:                                                   # the graph is the one the CPU file reasons about
        ids, w = eng.neighbors(v)
        assert np.array_equal(ids, provider(v)[0]) and np.array_equal(w, provider(v)[1], equal_nan=True)
    assert eng.neighbors(cases.W_ABSENT) is None
    seeds = cases.weighted_seeds()
    nb = nref.Rows(provider)
    a = check(oracle, eng, nb, seeds, cases.W_FANOUTS, "weighted rows", seed=1, epoch=0)
    b = check(oracle, eng, nb, seeds, cases.W_FANOUTS, "weighted rows, 32-byte records", seed=1, epoch=0, no_compact=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert (a[0][cases.W_DEAD] == -1).all() and (a[1][cases.W_DEAD] == -1).all()             # the dead end's children and grandchildren
    check(oracle, eng, nb, seeds, [64], "weighted rows", seed=2)
    check(oracle, eng, nb, seeds, [2, 2, 2], "weighted rows", seed=3, epoch=5, no_compact=True)
    check(oracle, eng, nb, seeds, [3, 3], "weighted rows, distinct", seed=4, replace=False)


def test_directed_graph_with_a_destination_only_vertex(oracle, eng):
    s, d, w = (np.array(c) for c in zip(*cases.HAND_LINES))
    eng.load_coo(s.astype(np.int32), d.astype(np.int32), w.astype(np.float32), directed=True)
    g = cases.hand_graph(oracle)
    assert eng.neighbors(4) is not None and len(eng.neighbors(4)[0]) == 0                    # a vertex, with an empty row
    for replace in (True, False):
        for fanouts in ([3, 2], [1], [2, 1, 2], [4]):
            got = check(oracle, eng, g.neighbors, cases.HAND_SEEDS, fanouts, "hand graph", seed=5, epoch=2, replace=replace)
            assert (got[0][4] == -1).all() and (got[0][6] == -1).all() and (got[0][7] == -1).all()


# ---- without replacement: every group width --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", cases.D_FANOUTS)
def test_distinct_positions_at_every_group_width(oracle, eng, f):
    rows = cases.distinct_rows(f)
    eng.load_adjacency(rows)
    provider = cases.rows_provider(rows)
    seeds = cases.D_SEEDS
    (got,) = check(oracle, eng, provider, seeds, [f], "distinct rows", seed=11, replace=False)
    for b, v in enumerate(seeds):
        ids = provider(v)[0]
        kids = got[b]
        if len(ids) <= f:                                                # the row in row order, then -1
            assert kids[:len(ids)].tolist() == ids.tolist() and (kids[len(ids):] == -1).all()
        else:                                                            # f different entries of the row (a row's ids are all different)
            assert (kids >= 0).all() and len(set(kids.tolist())) == f and set(kids.tolist()) <= set(ids.tolist())
    # ... and below a first layer, where a wave holds the children of several parents
    if f <= 16:
        eng.load_edgelist(KARATE, directed=False)
        g = oracle.Graph.load(KARATE, directed=False)
        check(oracle, eng, g.neighbors, g.vertices().tolist(), [3, f], "karate, distinct", seed=2, replace=False)


# ---- other graphs and sizes -----------------------------------------------------------------------------------------------------------------
def test_unit_weight_graph_before_and_after_a_biased_walk_built_its_id_rows(oracle, eng, karate):
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    rows = nref.Rows(g.neighbors)
    seeds = g.vertices().tolist()
    check(oracle, eng, rows, seeds, [5, 4], "before", seed=3, replace=False)
    eng.walk(p=0.5, q=2.0, walk_length=5, num_walks=1, fetch=False)      # (a biased walk lays out the 4-byte id rows of a unit-weight graph)
    check(oracle, eng, rows, seeds, [5, 4], "after", seed=3, replace=False)
    check(oracle, eng, rows, seeds, [5, 4], "after", seed=3, replace=True)


@pytest.mark.parametrize("sparse", [False, True])
def test_compacted_ids(oracle, sparse):
    s, d, w = random_multigraph(np.random.default_rng(7), 40, 300, True, id_lo=0)
    if sparse:                                                           # ids spread over all of int32, -1 among them
        ids = np.sort(np.random.default_rng(8).choice(np.arange(-2**31 + 1, 2**31 - 1, 104729), size=40, replace=False))
        ids[0], ids[-1], ids[20] = -2**31, 2**31 - 1, -1
        s, d = ids[s].astype(np.int32), ids[d].astype(np.int32)
    g = oracle.Graph.from_coo(s, d, w, directed=False)
    V = g.vertices().tolist()
    seeds = V + [V[3], 12345, -1]
    with pkg().Engine(device=0, compact_ids=not sparse) as e:
        e.load_coo(s, d, w, directed=False)
        for replace in (True, False):
            got = check(oracle, e, g.neighbors, seeds, [4, 3], "compacted ids", seed=9, replace=replace)
            assert (got[0][-1] == -1).all()
            if sparse:
                assert (got[0][V.index(-1)] == -1).all()                 # -1 never names a vertex here, not even on a graph that holds one


def test_more_elements_than_one_grid_pass(oracle, eng, karate):
    import torch
    src = open(os.path.join(ROOT, "stellar-random-walk_amd", "csrc", "neighbors.hip")).read()
    per_cu = int(re.search(r"#define SRW_NBR_BLOCKS_PER_CU (\d+)", src).group(1))
    B, fanouts = 4096, [10, 10]
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * per_cu * 256
    assert B * 100 > lanes and B * 10 * 16 > lanes                       # the last layer, per element and per group of 16 lanes
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices()
    seeds = V[np.arange(B) % len(V)].tolist()
    rows = nref.Rows(g.neighbors)
    for replace in (True, False):
        check(oracle, eng, rows, seeds, fanouts, "B = 4096", seed=4, replace=replace)


def test_beyond_2_to_the_31_elements(oracle, eng, karate):
    """B = 2^15 + 1, fanouts [256, 256]: the last layer has 2^31 + 2^16 elements (8.6 GB); row 2^15 starts at element 2^31."""
    import torch
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices()
    B, fanouts = (1 << 15) + 1, [256, 256]
    seeds = torch.as_tensor(V[np.arange(B) % len(V)].astype(np.int32)).to("cuda:0")
    l1, l2 = eng.sample_neighbors(seeds, fanouts, seed=12, epoch=3)
    assert tuple(l2.shape) == (B, 65536) and l2.numel() > 2**31
    picked = [0, (1 << 15) - 1, 1 << 15]
    want, _, _ = nref.sample(oracle, g.neighbors, seeds.cpu().numpy(), fanouts, seed=12, epoch=3, rows=picked)
    for r, b in enumerate(picked):
        assert np.array_equal(l1[b].cpu().numpy(), want[0][r]), b
        assert np.array_equal(l2[b].cpu().numpy(), want[1][r]), b
    for part in l2.split(8192):                                          # every element was written (karate has no dead end)
        assert int(part.min()) >= int(V.min()) and int(part.max()) <= int(V.max())
    del l1, l2
    torch.cuda.empty_cache()


# ---- the C entry point: margins, refusals, side state ---------------------------------------------------------------------------------------
def carve(torch, seeds, F, margin=64):
    """one poisoned int32 buffer: margin | seeds | margin | layer 1 | margin | ... | margin -> (buffer, offset of the seeds, offsets of the layers)"""
    B = len(seeds)
    sizes = [B] + [B * f for f in F[1:]]
    offs, pos = [], margin
    for n in sizes:
        offs.append(pos)
        pos += n + margin
    buf = torch.full((pos,), POISON, dtype=torch.int32, device="cuda:0")
    buf[offs[0]:offs[0] + B] = torch.tensor(seeds, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return buf, offs[0], offs[1:]


def raw(P, e, d_seeds, n_seeds, fanouts, layer_ptrs, replace=1, flags=0, seed=1, epoch=0, n_layers=None, with_np=True, with_fanouts=True,
        with_layers=True):
    L = P.lib()
    fan = (C.c_int32 * max(len(fanouts), 1))(*fanouts)
    ptrs = (C.c_void_p * max(len(layer_ptrs), 1))(*layer_ptrs)
    np_ = P.NeighborParams(seed, epoch, replace, flags)
    unknown = C.c_int64(-7)
    rc = L.srw_sample_neighbors(e.h, C.c_void_p(d_seeds) if d_seeds else None, n_seeds, fan if with_fanouts else None,
                                len(fanouts) if n_layers is None else n_layers, C.byref(np_) if with_np else None,
                                ptrs if with_layers else None, C.byref(unknown))
    return rc, L.srw_last_error(e.h).decode(), unknown.value


def test_poisoned_margins_stay_intact(oracle, eng, karate):
    import torch
    P = pkg()
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    seeds = cases.karate_seeds(g)
    B = len(seeds)
    for replace, fanouts in ((1, [3, 2]), (0, [3, 2]), (1, [65]), (0, [17, 1, 3])):
        F = nref.row_lengths(fanouts)
        buf, s_off, l_off = carve(torch, seeds, F)
        base = buf.data_ptr()
        rc, msg, unknown = raw(P, eng, base + 4 * s_off, B, fanouts, [base + 4 * o for o in l_off], replace=replace, seed=3)
        assert rc == P.OK, msg
        want, n_unknown, _ = nref.sample(oracle, g.neighbors, seeds, fanouts, seed=3, replace=bool(replace))
        assert unknown == n_unknown == 2
        h = buf.cpu().numpy()
        keep = np.ones(len(h), bool)
        keep[s_off:s_off + B] = False
        assert np.array_equal(h[s_off:s_off + B], np.array(seeds, dtype=np.int32))            # the seeds are only read
        for l, o in enumerate(l_off, start=1):
            assert np.array_equal(h[o:o + B * F[l]].reshape(B, F[l]), want[l - 1]), (fanouts, l)
            keep[o:o + B * F[l]] = False
        assert (h[keep] == POISON).all(), (fanouts, np.flatnonzero(h[keep] != POISON)[:8])


def test_every_refusal_leaves_the_outputs_untouched(oracle, karate):
    import torch
    P = pkg()
    L = P.lib()
    g = karate[False]
    seeds = cases.karate_seeds(g)
    B = len(seeds)
    F = nref.row_lengths([3, 2])
    buf, s_off, l_off = carve(torch, seeds, F)
    before = buf.clone()
    base = buf.data_ptr()
    S, L1, L2 = base + 4 * s_off, base + 4 * l_off[0], base + 4 * l_off[1]

    def refused(e, why, *a, **kw):
        rc, msg, unknown = raw(P, e, *a, **kw)
        assert rc == P.ERR_INVALID and unknown == -7, (why, rc, msg)
        if why is not None:
            assert msg.startswith("srw_sample_neighbors") and why in msg, (why, msg)
        torch.cuda.synchronize()
        assert torch.equal(buf, before), why

    with P.Engine(device=0) as e:
        refused(e, "no graph", S, B, [3, 2], [L1, L2])
        e.load_edgelist(KARATE, directed=False)
        refused(e, None, S, B, [3, 2], [L1, L2], with_np=False)
        refused(e, None, S, B, [3, 2], [L1, L2], with_fanouts=False)
        refused(e, None, S, B, [3, 2], [L1, L2], with_layers=False)
        refused(e, "n_layers", S, B, [3, 2], [L1, L2], n_layers=0)
        refused(e, "n_layers", S, B, [3, 2], [L1, L2], n_layers=-1)
        refused(e, "n_layers", S, B, [1] * 9, [L1] * 9)
        refused(e, "outside 1 .. 4096", S, B, [3, 0], [L1, L2])
        refused(e, "outside 1 .. 4096", S, B, [-2, 2], [L1, L2])
        refused(e, "outside 1 .. 4096", S, B, [4097], [L1])
        refused(e, "above 64", S, B, [65], [L1], replace=0)
        refused(e, "above 64", S, B, [2, 65], [L1, L2], replace=0)
        refused(e, "below 2^31", S, B, [4096, 4096, 128], [L1, L2, L2])
        refused(e, "n_seeds", S, -1, [3, 2], [L1, L2])
        refused(e, "n_seeds", S, 1 << 31, [3, 2], [L1, L2])
        refused(e, "unknown bit", S, B, [3, 2], [L1, L2], flags=2)
        refused(e, "unknown bit", S, B, [3, 2], [L1, L2], flags=-1)
        refused(e, "d_seeds is null", 0, B, [3, 2], [L1, L2])
        refused(e, "layer pointer is null", S, B, [3, 2], [L1, 0])
        refused(e, "not aligned", S + 2, B, [3, 2], [L1, L2])
        refused(e, "not aligned", S, B, [3, 2], [L1, L2 + 1])
        refused(e, "overlaps", S, B, [3, 2], [S, L2])                                        # layer 1 on the seeds
        refused(e, "overlaps", S, B, [3, 2], [L1, S + 4 * (B - 1)])                          # layer 2 over the last seed
        refused(e, "overlaps", S, B, [3, 2], [L1, L1])
        refused(e, "overlaps", S, B, [3, 2], [L1, L1 + 4 * (3 * B - 1)])                     # layer 2 over the last element of layer 1
        refused(e, "overlaps", S, B, [3, 2], [L2 - 4 * (3 * B - 1), L2])                     # layer 1 running into layer 2
        assert L.srw_shard_select(e.h, 1) == P.OK
        try:
            refused(e, "population 1", S, B, [3, 2], [L1, L2])
        finally:
            assert L.srw_shard_select(e.h, 0) == P.OK
        # n_seeds == 0 is fine whatever the pointers are, and launches nothing
        for ptrs in ([L1, L2], [0, 0], [L1 + 1, L1 + 1]):
            rc, msg, unknown = raw(P, e, 0, 0, [3, 2], ptrs)
            assert rc == P.OK and unknown == 0, msg
        torch.cuda.synchronize()
        assert torch.equal(buf, before)
        # ... and after all of them a valid call on the same buffers works
        rc, msg, unknown = raw(P, e, S, B, [3, 2], [L1, L2])
        assert rc == P.OK and unknown == 2, msg
        assert not torch.equal(buf, before)
    buf.copy_(before)
    with P.Engine(device=0, rank=0, world=2) as e:                               # a sharded handle
        e.load_edgelist(KARATE, directed=False)
        refused(e, "world == 1", S, B, [3, 2], [L1, L2])


def test_the_handles_other_state_is_untouched(oracle, eng, karate):
    import torch
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices()
    try:
        eng.set_sources(V[:7])
        eng.set_negative_weights(torch.arange(1, len(V) + 1, dtype=torch.int64, device="cuda:0"))
        eng.walk(p=1.0, q=1.0, walk_length=6, num_walks=2, seed=3, fetch=False)
        paths, lens = (x.clone() for x in eng.paths_tensor())
        where = eng.device_paths()
        neg = eng.skipgram_batch(3, num_negatives=5, seed=2)[1].clone()
        for replace in (True, False):
            eng.sample_neighbors(V.tolist(), [4, 3], replace=replace)
            eng.sample_neighbors(V.tolist(), [4, 3], replace=replace, no_compact=True)
        assert eng.device_paths() == where and eng.sources_len() == 7
        p2, l2 = eng.paths_tensor()
        assert torch.equal(p2, paths) and torch.equal(l2, lens)
        assert torch.equal(eng.skipgram_batch(3, num_negatives=5, seed=2)[1], neg)
        again = eng.walk(p=1.0, q=1.0, walk_length=6, num_walks=2, seed=3)
        assert np.array_equal(again[0], paths.cpu().numpy()) and len(again[1]) == 14         # still from the 7 sources
    finally:
        eng.clear_sources()
        eng.set_negative_weights(None)
