"""srw_importance_neighbors and Engine.importance_neighbors — what can be checked without a GPU: the symbol, its declaration, the refusals
that come before a handle or a device is touched, and the footing of the restatement the GPU tests hold every element to
(tests/importance_ref.py): its words are the oracle's Philox, its draw over a row is oracle_py.sample_index's, a graph of five vertices
worked by hand, five planted misreadings of the header comment that it must notice, its visit counts against the closed form of
personalised PageRank, and the conditions on the inputs tests/test_gpu_importance.py relies on (every arm is met, a tie sits exactly at
position T, a restart draw sits on each side of restart_m).  The inputs of the GPU file are built here, so that both files speak about
the same ones."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import importance_ref as iref
import test_neighbors_cpu as ncases
from conftest import KARATE, ROOT
from helpers import pkg


@pytest.fixture(autouse=True)
def _the_entry_point_and_the_method_exist():
    """The restatement's tests below are the footing of a feature: without the symbol or the method they have nothing to stand under,
    and they say so instead of passing."""
    P = pkg()
    assert hasattr(P.lib(), "srw_importance_neighbors"), "libstellar_rw.so lacks srw_importance_neighbors"
    assert hasattr(P.Engine, "importance_neighbors"), "Engine lacks importance_neighbors"


def test_the_library_exports_the_entry_point():
    P = pkg()
    assert "srw_importance_neighbors" in P.EXPORTS and hasattr(P.lib(), "srw_importance_neighbors")
    assert P.EXPORTS.index("srw_sample_neighbors") < P.EXPORTS.index("srw_importance_neighbors") < P.EXPORTS.index("srw_host_alloc")


def test_the_header_declares_the_function_and_states_the_semantics():
    text = open(os.path.join(ROOT, "include", "stellar_rw.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", text))             # (a comment's lines joined: a phrase may run over a line end)
    assert ("typedef struct { uint32_t seed; uint32_t epoch; uint32_t base; int32_t num_walks; int32_t walk_length; int32_t top; "
            "uint32_t restart_m; int32_t flags; } srw_importance_params;") in flat
    assert "enum { SRW_IMP_KEEP_SEED = 1, SRW_IMP_NO_COMPACT = 2" in flat
    assert ("int32_t srw_importance_neighbors(srw_handle *h, const void *d_seeds /* int32 [n_seeds] */, int64_t n_seeds, "
            "const srw_importance_params *ip, void *d_ids /* int32 [n_seeds][top] */, void *d_counts /* int32 [n_seeds][top] */, "
            "void *d_total /* int32 [n_seeds], or NULL */, int64_t *n_unknown /* or NULL */);") in flat
    assert flat.index("srw_sample_neighbors(srw_handle *h") < flat.index("srw_importance_params;") < flat.index("srw_host_alloc(")
    for said in ("R = num_walks, L = walk_length, T = top", "WITHIN THE CALL, never the vertex id",
                 "ctr = (base + b, w, s, epoch), key = (seed, 65)", "65 is this stream's", "seed k + b of a call with base = 0",
                 "(words[1] >> 8) < restart_m", "0 means never, 2^24 means always", "the first step is never cut",
                 "ends if N(curr) is empty", "m = words[0] >> 8, u = m * 2^-24", "RandomSample.scala:12-25", "step 1 of srw_walk",
                 "the 24-bit lattice included", "first-order at every step", "Arriving at next is one visit",
                 "Without SRW_IMP_KEEP_SEED the visits of the seed's own vertex are dropped", "the walk still passes through it",
                 "before any truncation", "at most R * L", "c descending, then by id ascending", "as a signed int32",
                 "padding is id -1 with count 0", "also on a graph with compacted ids", "counted in *n_unknown", "but is not counted",
                 "gets independent walks", "device_common.h:vertex_slot", "the only read-back", "every offset is 64-bit", "at most 1 GiB",
                 "vertex types and negative weights are untouched", "num_walks outside 1 .. 4096", "walk_length outside 1 .. 4096",
                 "num_walks * walk_length > 4096", "top outside 1 .. 64", "restart_m > 2^24", "flags with an unknown bit",
                 "base + n_seeds > 2^32", "n_seeds == 0 is SRW_OK whatever the pointers are"):
        assert said in flat, said


def test_the_struct_is_32_bytes():
    P = pkg()
    assert C.sizeof(P.ImportanceParams) == 32
    assert [n for n, _ in P.ImportanceParams._fields_] == ["seed", "epoch", "base", "num_walks", "walk_length", "top", "restart_m", "flags"]
    assert (P.IMP_KEEP_SEED, P.IMP_NO_COMPACT) == (1, 2)


def test_the_kernels_are_on_the_build_list():
    csrc = os.path.join(ROOT, "stellar-random-walk_amd", "csrc")
    assert re.search(r"^HIP_SRC\s*:=.*\bimportance\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    src = open(os.path.join(csrc, "importance.hip")).read()
    for k in ("k_imp_walk", "k_imp_topk", "cfo_pick<NT>", "fo_pick<NT>", "lane_pick_sequential", "vertex_slot", "g.cfo_reload", "__shared__"):
        assert k in src, k
    assert "atomicAdd(unknown" in src and src.count("atomic") == 2          # the unknown count, and the comment that says so


def test_null_arguments_are_refused_not_touched():
    """No handle can exist here (srw_create needs a device): what is reachable is the refusal of a NULL h."""
    P = pkg()
    L = P.lib()
    n = C.c_int64(-7)
    ip = P.ImportanceParams(1, 0, 0, 10, 2, 3, 1 << 23, 0)
    assert L.srw_importance_neighbors(None, C.c_void_p(64), 3, C.byref(ip), C.c_void_p(128), C.c_void_p(256), C.c_void_p(512),
                                      C.byref(n)) == P.ERR_INVALID
    assert L.srw_importance_neighbors(None, None, 0, None, None, None, None, None) == P.ERR_INVALID
    assert n.value == -7 and (ip.num_walks, ip.walk_length, ip.top, ip.restart_m) == (10, 2, 3, 1 << 23)


def test_the_engine_method_has_the_agreed_parameters():
    E = pkg().Engine
    sig = inspect.signature(E.importance_neighbors)
    assert list(sig.parameters) == ["self", "seeds", "num_walks", "walk_length", "top", "restart", "seed", "epoch", "base", "keep_seed",
                                    "return_total", "return_unknown", "no_compact", "restart_m"]
    assert [sig.parameters[k].default for k in ("restart", "seed", "epoch", "base", "keep_seed", "return_total", "return_unknown",
                                                 "no_compact", "restart_m")] == [0.5, 1, 0, 0, False, False, False, False, None]
    doc = E.importance_neighbors.__doc__
    assert "counts.float() / total.clamp(min=1)[:, None]" in doc and "PinSAGE" in doc and "personalised PageRank" in doc


def engine_without_a_handle():
    """Anything that reached the library would fail differently (there is no GPU here, and the handle is NULL)."""
    P = pkg()
    e = P.Engine.__new__(P.Engine)
    e.h, e.device = None, 0
    return e


def test_seeds_are_refused_before_the_library_is_called():
    e = engine_without_a_handle()
    t = torch.zeros((6,), dtype=torch.int32)
    bad = [
        (t, "in device memory"),
        (t.to(torch.int64), "in device memory"),
        (t.to(torch.int16), r"torch\.int32 or torch\.int64"),
        (t.to(torch.float32), r"torch\.int32 or torch\.int64"),
        (t.view(2, 3), "one-dimensional"),
        (torch.zeros((12,), dtype=torch.int32)[::2], "contiguous"),
        (np.zeros((2, 3), dtype=np.int32), "one-dimensional"),
        (np.zeros(4, dtype=np.float32), "must be integers"),
        ([0.5, 1.0], "must be integers"),
        (7, "one-dimensional"),
    ]
    for seeds, why in bad:
        with pytest.raises(TypeError, match="importance_neighbors.*" + why):
            e.importance_neighbors(seeds, 10, 2, 3)


def test_the_shape_and_the_restart_are_refused_before_the_library_is_called():
    e = engine_without_a_handle()
    bad = [
        (dict(num_walks=0), r"num_walks is outside 1 \.\. 4096"),
        (dict(num_walks=4097, walk_length=1), r"num_walks is outside 1 \.\. 4096"),
        (dict(num_walks=2.0), "num_walks must be an integer"),
        (dict(num_walks=True), "num_walks must be an integer"),
        (dict(num_walks="3"), "num_walks must be an integer"),
        (dict(walk_length=0), r"walk_length is outside 1 \.\. 4096"),
        (dict(num_walks=1, walk_length=4097), r"walk_length is outside 1 \.\. 4096"),
        (dict(walk_length=1.5), "walk_length must be an integer"),
        (dict(walk_length=None), "walk_length must be an integer"),
        (dict(num_walks=64, walk_length=65), "must not exceed 4096"),
        (dict(num_walks=4096, walk_length=2), "must not exceed 4096"),
        (dict(top=0), r"top is outside 1 \.\. 64"),
        (dict(top=65), r"top is outside 1 \.\. 64"),
        (dict(top=3.0), "top must be an integer"),
        (dict(restart=-0.01), r"restart must be in \[0, 1\]"),
        (dict(restart=1.0001), r"restart must be in \[0, 1\]"),
        (dict(restart=float("nan")), r"restart must be in \[0, 1\]"),
        (dict(restart="0.5"), "restart must be a number"),
        (dict(restart=None), "restart must be a number"),
        (dict(restart_m=-1), "restart_m must be an integer in 0"),
        (dict(restart_m=(1 << 24) + 1), "restart_m must be an integer in 0"),
        (dict(restart_m=0.5), "restart_m must be an integer in 0"),
    ]
    for kw, why in bad:
        args = dict(num_walks=10, walk_length=2, top=3)
        args.update(kw)
        with pytest.raises(TypeError, match="importance_neighbors.*" + why):  # ... before the seeds are touched or uploaded
            e.importance_neighbors([0, 1], **args)
    E = pkg().Engine
    assert E._importance_shape(4096, 1, 64) == (4096, 1, 64) and E._importance_shape(np.int64(64), np.int32(64), 1) == (64, 64, 1)


def test_restart_becomes_restart_m():
    E = pkg().Engine
    assert E._importance_restart(0) == 0 and E._importance_restart(0.0) == 0
    assert E._importance_restart(1) == 1 << 24 and E._importance_restart(1.0) == 1 << 24
    assert E._importance_restart(0.5) == 1 << 23
    assert E._importance_restart(2.0 ** -24) == 1
    assert E._importance_restart(np.float32(0.25)) == 1 << 22
    assert E._importance_restart(0.9, restart_m=5) == 5 and E._importance_restart(0.9, restart_m=1 << 24) == 1 << 24
    assert E._importance_restart(0.9, restart_m=np.int64(0)) == 0


# ---- the restatement's own footing --------------------------------------------------------------------------------------------------
def test_the_words_are_the_oracles_philox(oracle):
    b = np.array([0, 3, 70000, (1 << 32) - 1]).reshape(-1, 1, 1)
    w = np.array([0, 1, 4095]).reshape(1, -1, 1)
    s = np.array([0, 1, 4095]).reshape(1, 1, -1)
    w0, w1 = iref.words(b, w, s, 9, 77)
    for i, bb in enumerate(b.ravel().tolist()):
        for j, ww in enumerate(w.ravel().tolist()):
            for k, ss in enumerate(s.ravel().tolist()):
                o = oracle.philox((bb, ww, ss, 9), (77, 65))
                assert (int(w0[i, j, k]), int(w1[i, j, k])) == (o[0], o[1])


def hand_words(oracle, b, w, s, seed, epoch, base=0):
    return oracle.philox((base + b, w, s, epoch), (seed, 65))


@pytest.mark.parametrize("shape", [(6, 4, 3), (1, 1, 1), (16, 3, 5)])
@pytest.mark.parametrize("keep_seed", [False, True])
def test_five_vertices_worked_by_hand(oracle, shape, keep_seed):
    """test_neighbors_cpu's graph (every row's weights sum to a power of two, so its CDF is exact): 3 -> 4 and 4 is a dead end, 2 has a
    self-loop; the seeds are every vertex, vertex 0 twice, the absent id 7 and -1.  The walks are written out once more, scalar by scalar."""
    R, L, T = shape
    g = ncases.hand_graph(oracle)
    seed, epoch, base, restart_m = 5, 2, 3, 1 << 22
    ids, counts, total, unknown, arms = iref.sample(oracle, g.neighbors, ncases.HAND_SEEDS, R, L, T, restart_m, seed=seed, epoch=epoch,
                                                    base=base, keep_seed=keep_seed)
    assert unknown == 2                                                  # 7 and -1
    dead = cuts = 0
    for b, sv in enumerate(ncases.HAND_SEEDS):
        tally = {}
        if sv in ncases.HAND_CDF:
            for w in range(R):
                curr = sv
                for s in range(L):
                    o = hand_words(oracle, b, w, s, seed, epoch, base)
                    if s >= 1 and (o[1] >> 8) < restart_m:
                        cuts += 1
                        break
                    cdf = ncases.HAND_CDF[curr]
                    if not cdf:
                        dead += 1
                        break
                    u = (o[0] >> 8) / float(1 << 24)
                    curr = next(x for acc, x in cdf if acc >= u)         # (acc = 1 >= u always: the head fallback is never needed)
                    if keep_seed or curr != sv:
                        tally[curr] = tally.get(curr, 0) + 1
        want = sorted(tally.items(), key=lambda kv: (-kv[1], kv[0]))
        assert total[b] == sum(tally.values()), b
        row = [(int(i), int(c)) for i, c in zip(ids[b], counts[b])]
        assert row == (want + [(-1, 0)] * T)[:T], (b, row, want)
    assert (arms["dead_ends"], arms["restart_cuts"]) == (dead, cuts)
    assert (ids[4] == -1).all() and total[4] == 0 and (ids[6] == -1).all() and (ids[7] == -1).all()   # the dead end is a vertex: not unknown
    if R >= 6:
        assert not (np.array_equal(ids[0], ids[5]) and np.array_equal(counts[0], counts[5]))           # vertex 0 twice: independent walks
        assert dead >= 1


# ---- the inputs of tests/test_gpu_importance.py ----------------------------------------------------------------------------------------
SEED, EPOCH = 7, 2


def karate_seeds(g):
    """all 34 vertices, then a duplicate, an absent id and -1"""
    V = g.vertices().tolist()
    return V + [V[0], 100, -1]


KARATE_SHAPES = ((10, 2, 3), (1, 1, 1), (64, 1, 5), (65, 1, 5), (63, 3, 5), (3, 5, 64))
CAP_SHAPES = ((4096, 1, 64), (1, 4096, 64), (64, 64, 64))
# L = 1 on a graph without dead ends: every walk arrives once, so the number of visits — what is sorted — is R, on both sides of every
# power of two at which the sorted length (and the room it is given) changes (64 | 65 and 4096 are among the shapes above)
SORT_EDGE_SHAPES = ((128, 1, 5), (129, 1, 5), (256, 1, 7), (257, 1, 7), (512, 1, 7), (513, 1, 7), (1024, 1, 9), (1025, 1, 9), (2048, 1, 9),
                    (2049, 1, 9))


def boundary_restart_m(R=10, b=3, w=2):
    """restart_m on a word of the stream itself: d = the restart draw of (seed b, walk w, step 1) under (SEED, EPOCH).  With
    restart_m = d + 1 that draw equals restart_m - 1 (the walk is cut), with restart_m = d it equals restart_m (it is not)."""
    assert w < R
    d = int(iref.words(b, w, 1, EPOCH, SEED)[1]) >> 8
    assert 0 < d < (1 << 24) - 1
    return d + 1, d


def karate_variants():
    """(restart_m, keep_seed) of the small shapes"""
    m_cut, m_keep = boundary_restart_m()
    return [(m, k) for m in (0, 1 << 24, 1 << 23, m_cut, m_keep) for k in (False, True)]


STAR_LEAVES = 5000


def star_lines(ids=None):
    """hub 0 and the leaves 1 .. 5000, undirected, unit weights; ids: the vertex ids to use instead (ascending, 5001 of them)"""
    hub = np.zeros(STAR_LEAVES, dtype=np.int64)
    leaf = np.arange(1, STAR_LEAVES + 1, dtype=np.int64)
    if ids is not None:
        hub, leaf = ids[hub], ids[leaf]
    return hub.astype(np.int32), leaf.astype(np.int32), np.ones(STAR_LEAVES, dtype=np.float32)


def star_top_leaf(oracle):
    """the leaf (1 .. 5000) at the head of the hub's row under (R, L, T) = (4096, 1, 64): the largest count, the smallest id among those"""
    s, d, w = star_lines()
    g = oracle.Graph.from_coo(s, d, w, directed=False)
    return int(iref.sample(oracle, g.neighbors, [0], 4096, 1, 64, 0, seed=SEED, epoch=EPOCH)[0][0, 0])


def sparse_star_ids(oracle):
    """5001 ascending ids spread over all of int32, the hub the smallest; the leaf at the head of the hub's row (star_top_leaf: the rows
    depend on the order of the ids only) is the vertex -1, every id before it is negative"""
    k = star_top_leaf(oracle)
    rng = np.random.default_rng(8)
    neg = np.sort(rng.choice(np.arange(-2**31 + 1, -1, 9973), size=k - 1, replace=False))
    pos = np.sort(rng.choice(np.arange(0, 2**31 - 1, 9973), size=STAR_LEAVES - k, replace=False))
    ids = np.concatenate([[-2**31], neg, [-1], pos]).astype(np.int64)
    assert len(ids) == STAR_LEAVES + 1 and (np.diff(ids) > 0).all() and ids[k] == -1 and k > 100
    return ids


W_SHAPES = ((32, 8, 16), (8, 64, 64), (300, 1, 8))


def test_the_lookup_in_the_running_sums_is_the_oracles_draw(oracle):
    """every row the GPU file walks over: importance_ref.Rows.pick against oracle_py.sample_index"""
    rng = np.random.default_rng(5)
    checked = 0
    for directed in (False, True):
        g = oracle.Graph.load(KARATE, directed=directed)
        rows = iref.Rows(g.neighbors)
        checked += sum(rows.check_against(oracle, v, rng, n=16) for v in g.vertices().tolist())
    rows = iref.Rows(ncases.rows_provider(ncases.weighted_rows()))
    for v in range(ncases.W_N):
        if rows(v) is not None and len(rows(v)[0]):
            checked += rows.check_against(oracle, v, rng, n=16)
    assert rows.running_sums(ncases.W_IRREGULAR) is None                 # a negative and a NaN weight: the oracle, draw by draw
    s, d, w = star_lines()
    g = oracle.Graph.from_coo(s, d, w, directed=False)
    rows = iref.Rows(g.neighbors)
    checked += rows.check_against(oracle, 0, rng) + rows.check_against(oracle, 17, rng)
    assert checked > 5000


def test_planted_misreadings_are_noticed(oracle):
    g = oracle.Graph.load(KARATE, directed=False)
    seeds = karate_seeds(g)
    rows = iref.Rows(g.neighbors)
    m_cut, _ = boundary_restart_m()
    kw = dict(seed=SEED, epoch=EPOCH)
    good = iref.sample(oracle, rows, seeds, 10, 2, 3, 1 << 23, **kw)
    for defect in ("vertex_key", "restart_at_0", "ties_desc", "seed_kept"):
        wrong = iref.sample(oracle, rows, seeds, 10, 2, 3, 1 << 23, defect=defect, **kw)
        assert any((a != b).any() for a, b in zip(good[:3], wrong[:3])), defect
    # <= instead of <: only a draw that equals restart_m tells them apart — the boundary value is one
    _, m_keep = boundary_restart_m()
    good = iref.sample(oracle, rows, seeds, 10, 2, 3, m_keep, keep_seed=True, **kw)
    wrong = iref.sample(oracle, rows, seeds, 10, 2, 3, m_keep, keep_seed=True, defect="restart_le", **kw)
    assert wrong[2][3] == good[2][3] - 1 and wrong[4]["restart_cuts"] == good[4]["restart_cuts"] + 1
    # keyed by the vertex id, vertex 0's two rows would be the same
    by_id = iref.sample(oracle, rows, seeds, 10, 2, 3, 1 << 23, defect="vertex_key", **kw)
    assert np.array_equal(by_id[0][0], by_id[0][34]) and np.array_equal(by_id[1][0], by_id[1][34])
    good = iref.sample(oracle, rows, seeds, 10, 2, 3, 1 << 23, **kw)
    assert not (np.array_equal(good[0][0], good[0][34]) and np.array_equal(good[1][0], good[1][34]))


def test_the_semantics_are_monte_carlo_personalised_pagerank(oracle):
    """restart = 0.5, L = 4, keep_seed, N = 8192 walks per seed (8 epochs x R = 1024) on karate: the per-walk visit counts of the
    restatement against E[s, v] = sum_{k=1..4} 0.5^(k-1) (P^k)[s, v] in float64; every cell with N E >= 100; z from the sample mean and
    the sample variance over the walks; |z| <= 5."""
    g = oracle.Graph.load(KARATE, directed=False)
    V = g.vertices().tolist()
    n = len(V)
    pos = {v: i for i, v in enumerate(V)}
    P = np.zeros((n, n))
    for v in V:
        ids, w = g.neighbors(v)
        for x, ww in zip(ids.tolist(), w.astype(np.float64).tolist()):
            P[pos[v], pos[x]] += ww
    P /= P.sum(axis=1, keepdims=True)
    E, Pk = np.zeros((n, n)), np.eye(n)
    for k in range(1, 5):
        Pk = Pk @ P
        E += 0.5 ** (k - 1) * Pk
    R, L, epochs = 1024, 4, 8
    N = R * epochs
    rows = iref.Rows(g.neighbors)
    lut = np.full(max(V) + 1, -1)
    lut[V] = np.arange(n)
    s1, s2 = np.zeros((n, n)), np.zeros((n, n))
    for epoch in range(epochs):
        vis, _ = iref.visits(oracle, rows, V, R, L, 1 << 23, seed=11, epoch=epoch)
        X = np.zeros((n, R, n))                                          # visits of vertex v by walk w of seed s
        for s in range(L):
            col = vis[:, :, s]
            ok = col != iref.HOLE
            bi, wi = np.nonzero(ok)
            np.add.at(X, (bi, wi, lut[col[ok]]), 1.0)
        s1 += X.sum(axis=1)
        s2 += (X * X).sum(axis=1)
    mean = s1 / N
    var = (s2 - N * mean * mean) / (N - 1)
    cells = N * E >= 100
    z = (mean[cells] - E[cells]) / np.sqrt(var[cells] / N)
    print("cells %d, worst |z| %.2f" % (cells.sum(), np.abs(z).max()))
    assert cells.sum() >= 600
    assert np.abs(z).max() <= 5.0


def test_the_gpu_files_inputs_meet_every_arm(oracle):
    """restart cuts, dead ends, ties at the T boundary and dropped seed visits are all met by the GPU file's cases; one case has a tie
    exactly at position T; one restart draw equals restart_m - 1 and one equals restart_m."""
    met = dict.fromkeys(iref.ARMS, 0)
    kw = dict(seed=SEED, epoch=EPOCH)
    for directed in (False, True):
        g = oracle.Graph.load(KARATE, directed=directed)
        rows, seeds = iref.Rows(g.neighbors), karate_seeds(g)
        for R, L, T in KARATE_SHAPES:
            for restart_m, keep in karate_variants():
                arms = iref.sample(oracle, rows, seeds, R, L, T, restart_m, keep_seed=keep, **kw)[4]
                for k in met:
                    met[k] += arms[k]
    print(met)
    assert all(met[k] >= 1 for k in iref.ARMS), met
    assert met["dead_ends"] >= 10 and met["boundary_ties"] >= 10
    # the boundary value: the draw of (b = 3, w = 2, s = 1) is consulted (karate undirected has no dead end, step 0 is never cut) and
    # falls on either side
    g = oracle.Graph.load(KARATE, directed=False)
    seeds = karate_seeds(g)
    m_cut, m_keep = boundary_restart_m()
    d = int(iref.words(3, 2, 1, EPOCH, SEED)[1]) >> 8
    assert d == m_cut - 1 == m_keep
    cut, _ = iref.visits(oracle, g.neighbors, seeds, 10, 2, m_cut, rows=[3], **kw)
    kept, _ = iref.visits(oracle, g.neighbors, seeds, 10, 2, m_keep, rows=[3], **kw)
    assert cut[0, 2, 0] != iref.HOLE and cut[0, 2, 1] == iref.HOLE and kept[0, 2, 1] != iref.HOLE
    # a tie exactly at position T in the DGL shape: row b has more than T vertices and c[T - 1] == c[T]
    ids, counts, total, _, arms = iref.sample(oracle, g.neighbors, seeds, 10, 2, 3, 1 << 23, **kw)
    assert arms["boundary_ties"] >= 1
    # the star seeded at the hub with L = 1: thousands of vertices with small equal counts — the whole top T is decided by the tie order
    s, dd, w = star_lines()
    star = oracle.Graph.from_coo(s, dd, w, directed=False)
    ids, counts, total, _, arms = iref.sample(oracle, star.neighbors, [0], 4096, 1, 64, 1 << 23, **kw)
    assert arms["boundary_ties"] == 1 and total[0] == 4096 and 1 <= counts[0, 63] <= counts[0, 0] <= 8
    assert len(set(ids[0].tolist())) == 64 and (ids[0] > 0).all()
    # the weighted rows: the irregular row, the multi-edges, the self-loop and the dead end are all walked over
    nb = iref.Rows(ncases.rows_provider(ncases.weighted_rows()))
    vis, arms = iref.visits(oracle, nb, ncases.weighted_seeds(), 32, 8, 1 << 22, **kw)
    seen = set(vis[vis != iref.HOLE].tolist())
    assert {ncases.W_IRREGULAR, ncases.W_MULTI, ncases.W_DEAD} <= seen and arms["dead_ends"] >= 5
