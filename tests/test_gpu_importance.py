"""srw_importance_neighbors / Engine.importance_neighbors on the GPU: ids, counts and totals are held, exactly, against the numpy
restatement of the header comment (tests/importance_ref.py).  The inputs and the conditions they meet (every arm is met, a tie sits at
position T, a restart draw on each side of restart_m) are those of tests/test_importance_cpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import importance_ref as iref
import test_importance_cpu as cases
import test_neighbors_cpu as ncases
from conftest import KARATE, ROOT
from helpers import pkg

pytestmark = pytest.mark.gpu

POISON = -0x5A5A5A5B
SEED, EPOCH = cases.SEED, cases.EPOCH


@pytest.fixture(autouse=True)
def _the_entry_point_and_the_method_exist():
    P = pkg()
    assert hasattr(P.lib(), "srw_importance_neighbors"), "libstellar_rw.so lacks srw_importance_neighbors"
    assert hasattr(P.Engine, "importance_neighbors"), "Engine lacks importance_neighbors"


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def karate(oracle):
    return {d: oracle.Graph.load(KARATE, directed=d) for d in (False, True)}


def check(oracle, e, neighbors, seeds, R, L, T, restart_m, what="", rows=None, **kw):
    """one call through Engine.importance_neighbors; ids, counts, total and the unknown count against the restatement (all rows, or
    the rows named) -> (ids, counts, total) as numpy"""
    ref_kw = {k: v for k, v in kw.items() if k != "no_compact"}
    w_ids, w_counts, w_total, unknown, _ = iref.sample(oracle, neighbors, seeds, R, L, T, restart_m, rows=rows, **ref_kw)
    ids, counts, total, n_unknown = e.importance_neighbors(seeds, R, L, T, restart_m=restart_m, return_total=True, return_unknown=True, **kw)
    B = len(seeds)
    for x, shape in ((ids, (B, T)), (counts, (B, T)), (total, (B,))):
        assert str(x.dtype) == "torch.int32" and tuple(x.shape) == shape and x.is_cuda and x.is_contiguous()
    ids, counts, total = (x.cpu().numpy() for x in (ids, counts, total))
    pick = slice(None) if rows is None else np.asarray(rows)
    tag = (what, (R, L, T), restart_m, kw)
    assert n_unknown == unknown, (tag, n_unknown, unknown)
    assert np.array_equal(total[pick], w_total), (tag, "total", np.flatnonzero(total[pick] != w_total)[:6].tolist())
    assert np.array_equal(counts[pick], w_counts), (tag, "counts", np.argwhere(counts[pick] != w_counts)[:6].tolist())
    assert np.array_equal(ids[pick], w_ids), (tag, "ids", np.argwhere(ids[pick] != w_ids)[:6].tolist())
    return ids, counts, total


def invariants(torch, ids, counts, total, R, L, lo, hi):
    """on the device, every row: sum(counts) <= total <= R * L, counts non-increasing and positive exactly where an id stands, ids in
    [lo, hi] or -1"""
    s = counts.sum(dim=1)
    assert bool((s <= total).all()) and bool((total <= R * L).all()) and bool((total >= 0).all())
    assert bool((counts[:, 1:] <= counts[:, :-1]).all()) and bool((counts >= 0).all())
    pad = counts == 0
    assert bool((ids[pad] == -1).all()) and bool(((ids[~pad] >= lo) & (ids[~pad] <= hi)).all())


# ---- karate -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
def test_karate_every_shape(oracle, eng, karate, directed):
    import torch
    g = karate[directed]
    eng.load_edgelist(KARATE, directed=directed)
    rows = iref.Rows(g.neighbors)
    seeds = cases.karate_seeds(g)
    for R, L, T in cases.KARATE_SHAPES:
        for restart_m, keep in cases.karate_variants():
            check(oracle, eng, rows, seeds, R, L, T, restart_m, "karate", seed=SEED, epoch=EPOCH, keep_seed=keep)
    # the cap in its three shapes (L = 1 never consults the restart draw; restart 0 walks all 4096 steps on the undirected graph)
    for (R, L, T), restart_ms in zip(cases.CAP_SHAPES, ((1 << 23,), (0, 1 << 23), (0, 1 << 23))):
        for restart_m in restart_ms:
            for keep in (False, True):
                # (one walk of 4096 steps per seed: the restatement takes a step at a time — six rows of the call are worked out)
                some = [0, 11, 33, 34, 35, 36] if (R, restart_m) == (1, 0) else None
                check(oracle, eng, rows, seeds, R, L, T, restart_m, "karate, the cap", rows=some, seed=SEED, epoch=EPOCH, keep_seed=keep)
    # the padded sort length on both sides of every power of two
    for R, L, T in cases.SORT_EDGE_SHAPES:
        check(oracle, eng, rows, seeds, R, L, T, 1 << 22, "karate, sort lengths", seed=SEED, epoch=EPOCH, keep_seed=directed)
    # the 32-byte records give the same, element for element
    for R, L, T in ((10, 2, 3), (63, 3, 5), (64, 64, 64)):
        a = check(oracle, eng, rows, seeds, R, L, T, 1 << 23, "karate", seed=SEED, epoch=EPOCH)
        b = check(oracle, eng, rows, seeds, R, L, T, 1 << 23, "karate, 32-byte records", seed=SEED, epoch=EPOCH, no_compact=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # restart as a float; the seeds as a device tensor, int32 and int64; zero seeds
    a = eng.importance_neighbors(seeds, 10, 2, 3, restart=0.5, seed=SEED)
    b = eng.importance_neighbors(seeds, 10, 2, 3, restart_m=1 << 23, seed=SEED)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for dt in (torch.int32, torch.int64):
        b = eng.importance_neighbors(torch.tensor(seeds, dtype=dt, device="cuda:0"), 10, 2, 3, seed=SEED)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="outside int32"):
        eng.importance_neighbors(torch.tensor([0, 1 << 40], dtype=torch.int64, device="cuda:0"), 10, 2, 3)
    ids, counts, total, unknown = eng.importance_neighbors([], 10, 2, 3, return_total=True, return_unknown=True)
    assert tuple(ids.shape) == (0, 3) and tuple(counts.shape) == (0, 3) and tuple(total.shape) == (0,) and unknown == 0


def test_keying_and_base(oracle, eng, karate):
    """row b depends on (seed, epoch, base + b, its own seed vertex) and on nothing else in the batch; one call over 100 seeds equals two
    calls of 50 with base = 0 and base = 50"""
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices()
    seeds = V[np.arange(100) % len(V)].tolist()
    kw = dict(seed=5, epoch=1, return_total=True)
    whole = [x.cpu().numpy() for x in eng.importance_neighbors(seeds, 10, 3, 4, **kw)]
    again = [x.cpu().numpy() for x in eng.importance_neighbors(seeds, 10, 3, 4, **kw)]
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))                           # a repeat is bit for bit
    lo = [x.cpu().numpy() for x in eng.importance_neighbors(seeds[:50], 10, 3, 4, base=0, **kw)]
    hi = [x.cpu().numpy() for x in eng.importance_neighbors(seeds[50:], 10, 3, 4, base=50, **kw)]
    assert all(np.array_equal(a, np.concatenate([b, c])) for a, b, c in zip(whole, lo, hi))
    check(oracle, eng, g.neighbors, seeds[50:], 10, 3, 4, 1 << 23, "base", seed=5, epoch=1, base=50)
    check(oracle, eng, g.neighbors, seeds[:3], 10, 3, 4, 1 << 23, "base at the end of its range", seed=5, epoch=1, base=(1 << 32) - 3)
    i = 9
    perm = list(reversed(seeds))
    perm[i] = seeds[i]                                                                       # every other seed moves, row i stays
    moved = [x.cpu().numpy() for x in eng.importance_neighbors(perm, 10, 3, 4, **kw)]
    assert all(np.array_equal(a[i], b[i]) for a, b in zip(whole, moved)) and any((a != b).any() for a, b in zip(whole, moved))
    for other in (dict(kw, seed=6), dict(kw, epoch=2)):
        diff = [x.cpu().numpy() for x in eng.importance_neighbors(seeds, 10, 3, 4, **other)]
        assert any((a != b).any() for a, b in zip(whole, diff)), other
    assert any((a[:32] != a[34:66]).any() for a in whole)                                    # a vertex that occurs twice: independent walks


# ---- a star: the tie order decides --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_star(oracle, sparse):
    ids_map = cases.sparse_star_ids(oracle) if sparse else None
    s, d, w = cases.star_lines(ids_map)
    g = oracle.Graph.from_coo(s, d, w, directed=False)
    V = g.vertices()
    hub, leaf = int(V[0]), int(V[17])
    assert len(g.neighbors(hub)[0]) == cases.STAR_LEAVES
    rows = iref.Rows(g.neighbors)
    with pkg().Engine(device=0, compact_ids=sparse) as e:
        e.load_coo(s, d, w, directed=False)
        # a leaf: the hub has a large count, the seed itself is dropped (and kept with keep_seed)
        seeds = [leaf, hub, leaf, int(V[-1]), 12345, -1]
        ids, counts, total = check(oracle, e, rows, seeds, 64, 8, 8, 1 << 22, "star", seed=SEED, epoch=EPOCH)
        assert ids[0, 0] == hub and counts[0, 0] >= 64 and leaf not in ids[0].tolist()
        kept = check(oracle, e, rows, seeds, 64, 8, 8, 1 << 22, "star, keep_seed", seed=SEED, epoch=EPOCH, keep_seed=True)
        assert kept[2][1] > total[1] and hub in kept[0][1].tolist()      # seeded at the hub: every second visit is the seed's own
        # the hub with R = 4096, L = 1: thousands of leaves with small equal counts — the whole top T is decided by the tie order,
        # and on the sparse ids the order by slot must be the order by signed id (negative ids first)
        ids, counts, total = check(oracle, e, rows, [hub, hub], 4096, 1, 64, 0, "star, the hub", seed=SEED, epoch=EPOCH)
        assert total[0] == 4096 and counts[0, 0] <= 8 and (np.diff(counts[0]) <= 0).all()
        for c in set(counts[0].tolist()):
            run = ids[0][counts[0] == c]
            assert (np.diff(run.astype(np.int64)) > 0).all()                                 # ids ascending inside a run of equal counts
        check(oracle, e, rows, [hub], 4096, 1, 64, 0, "star, the hub, 32-byte records", seed=SEED, epoch=EPOCH, no_compact=True)
        if sparse:                                                       # the vertex -1 heads the hub's row, with a positive count;
            assert (ids_map == -1).any() and e.neighbors(-1) is not None  # as a seed -1 never names a vertex (the seeds above)
            assert ids[0, 0] == -1 and counts[0, 0] > 0 and (ids[0, 1:] != -1).all()
            assert (ids[0] < 0).sum() >= 8 and (ids[0] > 0).sum() >= 8


# ---- rows of every kind -------------------------------------------------------------------------------------------------------------------
def test_weighted_rows_through_both_record_forms(oracle, eng):
    """rows of 1 .. 4 097 entries with unit, 1 .. 16 and skewed weights, an irregular row (a negative and a NaN weight), multi-edges, a
    self-loop and a directed dead end (tests/test_neighbors_cpu.py's rows)"""
    rows = ncases.weighted_rows()
    eng.load_adjacency(rows)
    nb = iref.Rows(ncases.rows_provider(rows))
    seeds = ncases.weighted_seeds()
    for R, L, T in cases.W_SHAPES:
        for restart_m in (0, 1 << 22):
            a = check(oracle, eng, nb, seeds, R, L, T, restart_m, "weighted rows", seed=SEED, epoch=EPOCH, keep_seed=True)
            b = check(oracle, eng, nb, seeds, R, L, T, restart_m, "weighted rows, 32-byte records", seed=SEED, epoch=EPOCH, keep_seed=True,
                      no_compact=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            assert a[2][ncases.W_DEAD] == 0 and (a[0][ncases.W_DEAD] == -1).all()            # a vertex with an empty row
    check(oracle, eng, nb, seeds, 32, 8, 16, 1 << 22, "weighted rows", seed=3, epoch=0)
    # multi-edges: vertex 0 is reached from W_MULTI through three entries and is counted once
    ids, counts, total = check(oracle, eng, nb, [ncases.W_MULTI], 256, 1, 8, 0, "multi-edges", seed=SEED, keep_seed=True)
    assert ids[0].tolist().count(0) == 1 and counts[0][ids[0] == 0][0] > counts[0][ids[0] == 20][0]
    assert ncases.W_MULTI in ids[0].tolist()                                                  # the self-loop, kept with keep_seed


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------
def test_more_seeds_than_one_grid_pass(oracle, eng, karate):
    import torch
    src = open(os.path.join(ROOT, "stellar-random-walk_amd", "csrc", "importance.hip")).read()
    per_cu = int(re.search(r"constexpr int IMP_BLOCKS_PER_CU = (\d+);", src).group(1))
    B, (R, L, T) = 300000, (10, 2, 3)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert B * R > cus * per_cu * 256 and B > cus * 32                  # the walks per lane, the seeds per wave
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices()
    host = V[np.arange(B) % len(V)].astype(np.int32)
    host[1000], host[299999] = -1, 100
    seeds = torch.as_tensor(host).to("cuda:0")
    ids, counts, total, unknown = eng.importance_neighbors(seeds, R, L, T, seed=SEED, epoch=EPOCH, return_total=True, return_unknown=True)
    assert unknown == 2
    picked = np.unique(np.concatenate([[0, 1000, B - 2, B - 1], np.random.default_rng(3).integers(0, B, size=60)]))
    want = iref.sample(oracle, g.neighbors, host, R, L, T, 1 << 23, seed=SEED, epoch=EPOCH, rows=picked)
    sel = torch.as_tensor(picked).to("cuda:0")
    assert np.array_equal(ids[sel].cpu().numpy(), want[0]) and np.array_equal(counts[sel].cpu().numpy(), want[1])
    assert np.array_equal(total[sel].cpu().numpy(), want[2])
    invariants(torch, ids, counts, total, R, L, int(V.min()), int(V.max()))


def test_one_seed_past_the_scratch_chunk(oracle, eng, karate):
    """B = 65 537 at R * L = 4096: 65 536 seeds fill the 1 GiB of visits, the last one is a chunk of its own"""
    import torch
    src = open(os.path.join(ROOT, "stellar-random-walk_amd", "csrc", "importance.hip")).read()
    assert re.search(r"IMP_SCRATCH_BYTES = \(size_t\)1 << 30;", src)
    B, (R, L, T) = 65537, (4096, 1, 64)
    assert (B - 1) * R * L * 4 == 1 << 30
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices()
    host = V[np.arange(B) % len(V)].astype(np.int32)
    seeds = torch.as_tensor(host).to("cuda:0")
    ids, counts, total = eng.importance_neighbors(seeds, R, L, T, seed=SEED, epoch=EPOCH, return_total=True)
    picked = [0, 65535, 65536]
    want = iref.sample(oracle, g.neighbors, host, R, L, T, 1 << 23, seed=SEED, epoch=EPOCH, rows=picked)
    for r, b in enumerate(picked):
        assert np.array_equal(ids[b].cpu().numpy(), want[0][r]) and np.array_equal(counts[b].cpu().numpy(), want[1][r]), b
        assert int(total[b]) == want[2][r], b
    invariants(torch, ids, counts, total, R, L, int(V.min()), int(V.max()))
    del ids, counts, total
    torch.cuda.empty_cache()


# ---- the C entry point: margins, refusals, side state ---------------------------------------------------------------------------------------
def carve(torch, seeds, T, margin=64):
    """one poisoned int32 buffer: margin | seeds | margin | ids | margin | counts | margin | total | margin -> (buffer, the four offsets)"""
    B = len(seeds)
    offs, pos = [], margin
    for n in (B, B * T, B * T, B):
        offs.append(pos)
        pos += n + margin
    buf = torch.full((pos,), POISON, dtype=torch.int32, device="cuda:0")
    buf[offs[0]:offs[0] + B] = torch.tensor(seeds, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return buf, offs


def raw(P, e, d_seeds, n_seeds, d_ids, d_counts, d_total, R=10, L=2, T=3, restart_m=1 << 23, flags=0, seed=SEED, epoch=EPOCH, base=0,
        with_ip=True):
    L_ = P.lib()
    ip = P.ImportanceParams(seed, epoch, base, R, L, T, restart_m, flags)
    unknown = C.c_int64(-7)
    vp = lambda x: C.c_void_p(x) if x else None
    rc = L_.srw_importance_neighbors(e.h, vp(d_seeds), n_seeds, C.byref(ip) if with_ip else None, vp(d_ids), vp(d_counts), vp(d_total),
                                     C.byref(unknown))
    return rc, L_.srw_last_error(e.h).decode(), unknown.value


def test_poisoned_margins_stay_intact(oracle, eng, karate):
    import torch
    P = pkg()
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    seeds = cases.karate_seeds(g)
    B = len(seeds)
    for (R, L, T), with_total in (((10, 2, 3), True), ((65, 1, 5), True), ((3, 5, 64), False), ((64, 64, 64), True)):
        buf, (o_s, o_i, o_c, o_t) = carve(torch, seeds, T)
        base = buf.data_ptr()
        rc, msg, unknown = raw(P, eng, base + 4 * o_s, B, base + 4 * o_i, base + 4 * o_c, base + 4 * o_t if with_total else 0, R=R, L=L, T=T)
        assert rc == P.OK, msg
        want = iref.sample(oracle, g.neighbors, seeds, R, L, T, 1 << 23, seed=SEED, epoch=EPOCH)
        assert unknown == want[3] == 2
        h = buf.cpu().numpy()
        keep = np.ones(len(h), bool)
        assert np.array_equal(h[o_s:o_s + B], np.array(seeds, dtype=np.int32))                # the seeds are only read
        keep[o_s:o_s + B] = False
        assert np.array_equal(h[o_i:o_i + B * T].reshape(B, T), want[0]) and np.array_equal(h[o_c:o_c + B * T].reshape(B, T), want[1])
        keep[o_i:o_i + B * T] = keep[o_c:o_c + B * T] = False
        if with_total:
            assert np.array_equal(h[o_t:o_t + B], want[2])
            keep[o_t:o_t + B] = False
        assert (h[keep] == POISON).all(), ((R, L, T), np.flatnonzero(h[keep] != POISON)[:8])


def test_every_refusal_leaves_the_outputs_untouched(oracle, karate):
    import torch
    P = pkg()
    L = P.lib()
    g = karate[False]
    seeds = cases.karate_seeds(g)
    B, T = len(seeds), 3
    buf, (o_s, o_i, o_c, o_t) = carve(torch, seeds, T)
    before = buf.clone()
    base = buf.data_ptr()
    S, I, Cn, Tt = (base + 4 * o for o in (o_s, o_i, o_c, o_t))

    def refused(e, why, *a, **kw):
        rc, msg, unknown = raw(P, e, *a, **kw)
        assert rc == P.ERR_INVALID and unknown == -7, (why, rc, msg)
        if why is not None:
            assert msg.startswith("srw_importance_neighbors") and why in msg, (why, msg)
        torch.cuda.synchronize()
        assert torch.equal(buf, before), why

    with P.Engine(device=0) as e:
        refused(e, "no graph", S, B, I, Cn, Tt)
        e.load_edgelist(KARATE, directed=False)
        refused(e, None, S, B, I, Cn, Tt, with_ip=False)
        refused(e, "num_walks must be in 1 .. 4096", S, B, I, Cn, Tt, R=0)
        refused(e, "num_walks must be in 1 .. 4096", S, B, I, Cn, Tt, R=-3)
        refused(e, "num_walks must be in 1 .. 4096", S, B, I, Cn, Tt, R=4097, L=1)
        refused(e, "walk_length must be in 1 .. 4096", S, B, I, Cn, Tt, L=0)
        refused(e, "walk_length must be in 1 .. 4096", S, B, I, Cn, Tt, R=1, L=4097)
        refused(e, "must not exceed 4096", S, B, I, Cn, Tt, R=64, L=65)
        refused(e, "must not exceed 4096", S, B, I, Cn, Tt, R=4096, L=4096)
        refused(e, "top must be in 1 .. 64", S, B, I, Cn, Tt, T=0)
        refused(e, "top must be in 1 .. 64", S, B, I, Cn, Tt, T=65)
        refused(e, "restart_m", S, B, I, Cn, Tt, restart_m=(1 << 24) + 1)
        refused(e, "restart_m", S, B, I, Cn, Tt, restart_m=0xFFFFFFFF)
        refused(e, "unknown bit", S, B, I, Cn, Tt, flags=4)
        refused(e, "unknown bit", S, B, I, Cn, Tt, flags=-1)
        refused(e, "n_seeds", S, -1, I, Cn, Tt)
        refused(e, "n_seeds", S, 1 << 31, I, Cn, Tt)
        refused(e, "base + n_seeds", S, B, I, Cn, Tt, base=(1 << 32) - B + 1)
        refused(e, "d_seeds is null", 0, B, I, Cn, Tt)
        refused(e, "d_ids is null", S, B, 0, Cn, Tt)
        refused(e, "d_counts is null", S, B, I, 0, Tt)
        refused(e, "not aligned", S + 2, B, I, Cn, Tt)
        refused(e, "not aligned", S, B, I + 1, Cn, Tt)
        refused(e, "not aligned", S, B, I, Cn + 2, Tt)
        refused(e, "not aligned", S, B, I, Cn, Tt + 3)
        refused(e, "overlaps", S, B, S, Cn, Tt)                                              # ids on the seeds
        refused(e, "overlaps", S, B, I, I, Tt)                                               # counts on ids
        refused(e, "overlaps", S, B, I, I + 4 * (B * T - 1), Tt)                             # counts over the last element of ids
        refused(e, "overlaps", S, B, I, Cn, S + 4 * (B - 1))                                 # total over the last seed
        refused(e, "overlaps", S, B, I, Cn, Cn + 4 * (B * T - 1))                            # total over the last count
        refused(e, "overlaps", S, B, Cn - 4 * (B * T - 1), Cn, Tt)                           # ids running into counts
        refused(e, "overlaps", S, B, I, Cn, I)                                               # total on ids
        assert L.srw_shard_select(e.h, 1) == P.OK
        try:
            refused(e, "population 1", S, B, I, Cn, Tt)
        finally:
            assert L.srw_shard_select(e.h, 0) == P.OK
        # n_seeds == 0 is fine whatever the pointers are, and launches nothing
        for ptrs in ((I, Cn, Tt), (0, 0, 0), (I + 1, I + 1, I + 1)):
            rc, msg, unknown = raw(P, e, 0, 0, *ptrs)
            assert rc == P.OK and unknown == 0, msg
        torch.cuda.synchronize()
        assert torch.equal(buf, before)
        # base + n_seeds == 2^32 exactly is allowed; and after all the refusals a valid call on the same buffers works
        rc, msg, unknown = raw(P, e, S, B, I, Cn, Tt, base=(1 << 32) - B)
        assert rc == P.OK and unknown == 2, msg
        assert not torch.equal(buf, before)
    buf.copy_(before)
    with P.Engine(device=0, rank=0, world=2) as e:                               # a sharded handle
        e.load_edgelist(KARATE, directed=False)
        refused(e, "world == 1", S, B, I, Cn, Tt)


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
        for shape in ((10, 2, 3), (64, 64, 64)):
            eng.importance_neighbors(V.tolist(), *shape)
            eng.importance_neighbors(V.tolist(), *shape, no_compact=True, keep_seed=True)
        assert eng.device_paths() == where and eng.sources_len() == 7
        p2, l2 = eng.paths_tensor()
        assert torch.equal(p2, paths) and torch.equal(l2, lens)
        assert torch.equal(eng.skipgram_batch(3, num_negatives=5, seed=2)[1], neg)
        again = eng.walk(p=1.0, q=1.0, walk_length=6, num_walks=2, seed=3)
        assert np.array_equal(again[0], paths.cpu().numpy()) and len(again[1]) == 14         # still from the 7 sources
    finally:
        eng.clear_sources()
        eng.set_negative_weights(None)


def test_always_restarting_is_a_histogram_of_first_order_draws(oracle, eng, karate):
    """restart_m = 2^24 with keep_seed: every walk is exactly one first-order step, so a seed's counts are the histogram of R independent
    RandomSample.sample draws — exactly the restatement's, and supported inside Engine.neighbors(seed)"""
    g = karate[False]
    eng.load_edgelist(KARATE, directed=False)
    V = g.vertices().tolist()
    R = 512
    for L in (1, 8):
        ids, counts, total = check(oracle, eng, g.neighbors, V, R, L, 64, 1 << 24, "one step", seed=SEED, epoch=EPOCH, keep_seed=True)
        assert (total == R).all()
        for b, v in enumerate(V):
            nb = set(eng.neighbors(v)[0].tolist())
            got = ids[b][counts[b] > 0].tolist()
            assert set(got) <= nb and counts[b].sum() == R, v
            w0 = iref.words(b, np.arange(R), 0, EPOCH, SEED)[0]
            row = iref.Rows(g.neighbors)
            hist = np.bincount(row(v)[0][row.pick(oracle, v, (w0 >> np.uint64(8)).astype(np.int64))], minlength=max(V) + 1)
            assert all(hist[i] == c for i, c in zip(got, counts[b][counts[b] > 0].tolist()))
