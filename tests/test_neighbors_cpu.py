"""srw_sample_neighbors and Engine.sample_neighbors — what can be checked without a GPU: the symbol, its declaration, the refusals that
come before a handle or a device is touched, and the footing of the restatement the GPU tests hold every element to
(tests/neighbors_ref.py): a graph of five vertices worked by hand in both modes, three planted misreadings of the header comment that
it must notice, and the conditions on the inputs tests/test_gpu_neighbors.py relies on (its Floyd inputs collide, its weighted inputs
reach every arm of the draw).  The inputs of the GPU file are built here, so that both files speak about the same ones."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import first_order_code_ref as foref
import neighbors_ref as nref
from conftest import KARATE, ROOT
from helpers import pkg


@pytest.fixture(autouse=True)
def _the_entry_point_and_the_method_exist():
    """The restatement's tests below are the footing of a feature: without the symbol or the method they have nothing to stand under,
    and they say so instead of passing."""
    P = pkg()
    assert hasattr(P.lib(), "srw_sample_neighbors"), "libstellar_rw.so lacks srw_sample_neighbors"
    assert hasattr(P.Engine, "sample_neighbors"), "Engine lacks sample_neighbors"


def test_the_library_exports_the_entry_point():
    P = pkg()
    assert "srw_sample_neighbors" in P.EXPORTS and hasattr(P.lib(), "srw_sample_neighbors")


def test_the_header_declares_the_function_and_states_the_semantics():
    text = open(os.path.join(ROOT, "include", "stellar_rw.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", text))             # (a comment's lines joined: a phrase may run over a line end)
    assert "typedef struct { uint32_t seed; uint32_t epoch; int32_t replace; int32_t flags; } srw_neighbor_params;" in flat
    assert "enum { SRW_NBR_NO_COMPACT = 1" in flat
    assert ("int32_t srw_sample_neighbors(srw_handle *h, const void *d_seeds /* int32 [n_seeds] */, int64_t n_seeds, "
            "const int32_t *fanouts /* host, [n_layers] */, int32_t n_layers, const srw_neighbor_params *np, "
            "void *const *d_layers /* host array of n_layers device pointers */, int64_t *n_unknown /* or NULL */);") in flat
    assert flat.index("srw_walk_metapath(srw_handle *h, const srw_walk_params") < flat.index("srw_neighbor_params;") < flat.index("srw_host_alloc(")
    for said in ("F_0 = 1 and F_l = F_{l-1} * fanouts[l-1]", "element (b, j / fanouts[l-1]) of layer l-1", "layer 0 is the seed list",
                 "No relabelling and no edge list are produced", "out of scope", "Ids are the input's ids",
                 "ctr = (b, j, l, epoch), key = (seed, 64)", "WITHIN THE CALL, never the vertex id", "64 is this stream's",
                 "m = word >> 8, u = m * 2^-24", "RandomSample.scala:12-25", "step 1 of srw_walk", "Multi-edges and self-loops",
                 "beyond 2^24 entries", "srw_graph_neighbors order", "in row order, then -1", "J = deg - f + i",
                 "t = (uint64(word_i) * (J + 1)) >> 32", "else entry J", "Positions are distinct", "-1 included",
                 "device_common.h:vertex_slot", "the only read-back", "every offset is 64-bit", "n_layers outside 1 .. 8",
                 "a fanout outside 1 .. 4096", "a fanout above 64 with replace == 0", "F_L >= 2^31", "flags with an unknown bit",
                 "n_seeds == 0 is SRW_OK whatever the pointers are", "vertex types and negative weights are untouched"):
        assert said in flat, said


def test_the_struct_is_16_bytes():
    P = pkg()
    assert C.sizeof(P.NeighborParams) == 16
    assert [n for n, _ in P.NeighborParams._fields_] == ["seed", "epoch", "replace", "flags"]
    assert P.NBR_NO_COMPACT == 1


def test_the_kernels_are_on_the_build_list():
    csrc = os.path.join(ROOT, "stellar-random-walk_amd", "csrc")
    assert re.search(r"^HIP_SRC\s*:=.*\bneighbors\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    src = open(os.path.join(csrc, "neighbors.hip")).read()
    for k in ("k_nbr_replace", "k_nbr_distinct", "cfo_pick<NT>", "fo_pick<NT>", "lane_pick_sequential", "vertex_slot", "g.cfo_reload"):
        assert k in src, k


def test_null_arguments_are_refused_not_touched():
    """No handle can exist here (srw_create needs a device): what is reachable is the refusal of a NULL h."""
    P = pkg()
    L = P.lib()
    n = C.c_int64(-7)
    np_ = P.NeighborParams(1, 0, 1, 0)
    fan = (C.c_int32 * 2)(3, 2)
    layers = (C.c_void_p * 2)(64, 128)
    assert L.srw_sample_neighbors(None, C.c_void_p(64), 3, fan, 2, C.byref(np_), layers, C.byref(n)) == P.ERR_INVALID
    assert L.srw_sample_neighbors(None, None, 0, None, 0, None, None, None) == P.ERR_INVALID
    assert n.value == -7 and list(layers) == [64, 128] and list(fan) == [3, 2]


def test_the_engine_method_has_the_agreed_parameters():
    E = pkg().Engine
    sig = inspect.signature(E.sample_neighbors)
    assert list(sig.parameters) == ["self", "seeds", "fanouts", "seed", "epoch", "replace", "return_unknown", "no_compact"]
    assert [sig.parameters[k].default for k in ("seed", "epoch", "replace", "return_unknown", "no_compact")] == [1, 0, True, False, False]
    doc = E.sample_neighbors.__doc__
    assert "parent = j // f_l" in doc and "X[e.rows_of(" in doc


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
        (t.to(torch.uint8), r"torch\.int32 or torch\.int64"),
        (t.to(torch.float32), r"torch\.int32 or torch\.int64"),
        (t.view(2, 3), "one-dimensional"),
        (torch.zeros((12,), dtype=torch.int32)[::2], "contiguous"),
        (np.zeros((2, 3), dtype=np.int32), "one-dimensional"),
        (np.zeros(4, dtype=np.float32), "must be integers"),
        ([0.5, 1.0], "must be integers"),
        (7, "one-dimensional"),
    ]
    for seeds, why in bad:
        for replace in (True, False):
            with pytest.raises(TypeError, match="sample_neighbors.*" + why):
                e.sample_neighbors(seeds, [3, 2], replace=replace)


def test_fanouts_are_refused_before_the_library_is_called():
    e = engine_without_a_handle()
    bad = [
        ([], True, r"1 \.\. 8 entries"),
        ([2] * 9, True, r"1 \.\. 8 entries"),
        ([[3, 2]], True, r"1 \.\. 8 entries"),
        ([3, 1.5], True, "must be integers"),
        (["a"], True, "must be integers"),
        ([True], True, "must be integers"),
        ([3, 0], True, r"outside 1 \.\. 4096"),
        ([-1], True, r"outside 1 \.\. 4096"),
        ([4097], True, r"outside 1 \.\. 4096"),
        ([65], False, "above 64 needs replace=True"),
        ([2, 65], False, "above 64 needs replace=True"),
        ([4096, 4096, 128], True, r"below 2\^31"),
        ("32", True, "sequence of integers"),
        (3, True, "sequence of integers"),
        (None, True, "sequence of integers"),
    ]
    for fanouts, replace, why in bad:
        with pytest.raises(TypeError, match="sample_neighbors.*" + why):     # ... before the seeds are touched or uploaded
            e.sample_neighbors([0, 1], fanouts, replace=replace)
    P = pkg()
    assert P.Engine._neighbor_fanouts([25, 10], False).tolist() == [25, 10]
    assert P.Engine._neighbor_fanouts(np.array([4096, 4096, 127]), True).dtype == np.int32
    assert P.Engine._neighbor_fanouts((64,), False).tolist() == [64] and P.Engine._neighbor_fanouts((65,), True).tolist() == [65]


# ---- the restatement's own footing --------------------------------------------------------------------------------------------------
def test_the_words_are_the_oracles_philox(oracle):
    W = nref.words([0, 3, 70000], 5, 2, 9, 77)
    for r, b in enumerate((0, 3, 70000)):
        for j in range(5):
            assert int(W[r, j]) == oracle.philox((b, j, 2, 9), (77, 64))[0]


# Five vertices, directed, rows in line order; every row's weights sum to a power of two, so its CDF is exact:
#   N(0) = [3 (w 1), 1 (w 1), 2 (w 2), 4 (w 4)]     acc = 1/8, 1/4, 1/2, 1
#   N(1) = [0 (w 1), 3 (w 3)]                       acc = 1/4, 1
#   N(2) = [2 (w 1, a self-loop), 0 (w 1)]          acc = 1/2, 1
#   N(3) = [4 (w 1)]                                acc = 1
#   N(4) = []                                       a destination-only vertex
HAND_LINES = [(0, 3, 1.0), (0, 1, 1.0), (0, 2, 2.0), (0, 4, 4.0), (1, 0, 1.0), (1, 3, 3.0), (2, 2, 1.0), (2, 0, 1.0), (3, 4, 1.0)]
HAND_CDF = {0: [(0.125, 3), (0.25, 1), (0.5, 2), (1.0, 4)], 1: [(0.25, 0), (1.0, 3)], 2: [(0.5, 2), (1.0, 0)], 3: [(1.0, 4)], 4: []}
HAND_ROWS = {v: [x for _, x in c] for v, c in HAND_CDF.items()}
HAND_SEEDS = [0, 1, 2, 3, 4, 0, 7, -1]              # every vertex, vertex 0 twice, an absent id, -1


def hand_graph(oracle):
    s, d, w = (np.array(c) for c in zip(*HAND_LINES))
    return oracle.Graph.from_coo(s, d, w.astype(np.float32), directed=True)


def hand_word(oracle, b, j, l, seed, epoch):
    return oracle.philox((b, j, l, epoch), (seed, 64))[0]


@pytest.mark.parametrize("fanouts", [[3, 2], [1], [2, 1, 2]])
def test_five_vertices_worked_by_hand_with_replacement(oracle, fanouts):
    g = hand_graph(oracle)
    seed, epoch = 5, 2
    layers, unknown, _ = nref.sample(oracle, g.neighbors, HAND_SEEDS, fanouts, seed=seed, epoch=epoch, replace=True)
    assert unknown == 2                                                  # 7 and -1
    prev = np.array(HAND_SEEDS).reshape(-1, 1)
    for l, f in enumerate(fanouts, start=1):
        L = layers[l - 1]
        assert L.shape == (len(HAND_SEEDS), prev.shape[1] * f) and L.dtype == np.int32
        for b in range(L.shape[0]):
            for j in range(L.shape[1]):
                parent = int(prev[b, j // f])
                cdf = HAND_CDF.get(parent, [])                           # (7 and -1: no row)
                if not cdf:
                    assert L[b, j] == -1
                    continue
                u = (hand_word(oracle, b, j, l, seed, epoch) >> 8) / float(1 << 24)
                want = next(x for acc, x in cdf if acc >= u)             # (acc = 1 >= u always: the head fallback is never needed)
                assert L[b, j] == want, (l, b, j, parent, u)
        prev = L
    # vertex 0 occurs twice: the draws are keyed by b, so its two subtrees are independent
    assert any(not np.array_equal(L[0], L[5]) for L in layers) or fanouts == [1]


@pytest.mark.parametrize("fanouts", [[2], [3], [2, 2], [4], [1, 5]])
def test_five_vertices_worked_by_hand_without_replacement(oracle, fanouts):
    g = hand_graph(oracle)
    seed, epoch = 9, 1
    layers, unknown, collisions = nref.sample(oracle, g.neighbors, HAND_SEEDS, fanouts, seed=seed, epoch=epoch, replace=False)
    assert unknown == 2
    prev = np.array(HAND_SEEDS).reshape(-1, 1)
    seen = 0
    for l, f in enumerate(fanouts, start=1):
        L = layers[l - 1]
        for b in range(L.shape[0]):
            for jp in range(prev.shape[1]):
                row = HAND_ROWS.get(int(prev[b, jp]), [])
                got = L[b, jp * f:(jp + 1) * f].tolist()
                if len(row) <= f:
                    assert got == row + [-1] * (f - len(row))
                    continue
                pos = []
                for i in range(f):                                       # the header's Floyd, written out once more
                    J = len(row) - f + i
                    t = (hand_word(oracle, b, jp * f + i, l, seed, epoch) * (J + 1)) >> 32
                    if t in pos:
                        seen += 1
                        t = J
                    pos.append(t)
                assert len(set(pos)) == f
                assert got == [row[t] for t in pos], (l, b, jp)
        prev = L
    assert collisions == seen


# ---- the inputs of tests/test_gpu_neighbors.py ------------------------------------------------------------------------------------------
def karate_seeds(g):
    """all vertices, then duplicates, an absent id and -1"""
    V = g.vertices().tolist()
    return V + [V[0], V[0], V[33], 100, -1, V[5]]


KARATE_FANOUTS = ([3, 2], [1], [64], [5, 1, 4])


def weights_of(kind, deg):
    if kind == "unit":
        return np.ones(deg, np.float32)
    if kind == "int16":
        return np.tile(np.arange(1, 17, dtype=np.float32), (deg + 15) // 16)[:deg]
    w = np.ones(deg, np.float32)                        # "skew": first_order_code_ref's heavy_first — cdf_0 = 0.75, guide deltas in the hundreds
    w[0] = 3.0 * max(deg - 1, 1)
    return w


W_DEGS = (1, 2, 63, 64, 65, 4097)
W_KINDS = ("unit", "int16", "skew")
W_IRREGULAR, W_MULTI, W_DEAD, W_ABSENT, W_N = 18, 19, 20, 21, 23
W_FANOUTS = [8, 4]


def weighted_rows():
    """load_adjacency rows: vertex 3 * d + k has W_DEGS[d] entries with weights of W_KINDS[k]; every row walks round the ids 0 .. 22,
    so the second layer meets every row.  18: a negative and a NaN weight; 19: multi-edges and a self-loop; 20: a dead end; 21: named
    by the rows but without one of its own (no vertex on this surface); 22: a plain row."""
    rows = []
    for d, deg in enumerate(W_DEGS):
        for k, kind in enumerate(W_KINDS):
            v = 3 * d + k
            ids = (v + 1 + np.arange(deg)) % W_N
            rows.append((v, list(zip(ids.tolist(), weights_of(kind, deg).tolist()))))
    rows.append((W_IRREGULAR, [(0, 1.0), (5, -0.5), (17, 2.0), (20, float("nan")), (19, 1.0)]))
    rows.append((W_MULTI, [(19, 1.0), (0, 1.0), (0, 2.0), (0, 1.0), (20, 1.0), (18, 4.0)]))
    rows.append((W_DEAD, []))
    rows.append((22, [(18, 1.0), (19, 2.0), (21, 1.0), (16, 4.0)]))
    return rows


def weighted_seeds():
    return list(range(W_N)) + [W_DEAD, 17, 17, 100, -1]


def rows_provider(rows):
    """neighbors(v) of a load_adjacency graph: the first occurrence of a vertex wins, an id without a row is no vertex"""
    table = {}
    for v, nb in rows:
        table.setdefault(int(v), (np.array([e[0] for e in nb], dtype=np.int32), np.array([e[-1] for e in nb], dtype=np.float32)))
    return lambda v: table.get(int(v))


D_FANOUTS = (1, 2, 16, 17, 33, 64)
D_SEEDS = [0, 1, 2, 3, 4] * 8                         # (a row of f + 1 entries collides at a given child with probability 1 / 3 at f = 2: several tries)


def distinct_rows(f):
    """rows of f - 1, f, f + 1, 2 f and 4 097 entries (vertices 0 .. 4), weights 1 .. 16 (which the draw ignores), every entry of a row
    a different id (no rows of their own): distinct positions are distinct ids"""
    rows = []
    for v, deg in enumerate((f - 1, f, f + 1, 2 * f, 4097)):
        ids = 100 + 8192 * v + np.arange(deg)
        rows.append((v, list(zip(ids.tolist(), weights_of("int16", deg).tolist()))))
    return rows


def test_planted_misreadings_are_noticed(oracle):
    g = oracle.Graph.load(KARATE, directed=False)
    seeds = karate_seeds(g)
    rows = nref.Rows(g.neighbors)
    good = nref.sample(oracle, rows, seeds, [3, 2], seed=3)
    wrong = nref.sample(oracle, rows, seeds, [3, 2], seed=3, defect="vertex_key")
    assert any((a != b).any() for a, b in zip(good[0], wrong[0]))
    wrong = nref.sample(oracle, rows, seeds, [3, 2], seed=3, defect="parent_mod")
    assert np.array_equal(good[0][0], wrong[0][0]) and (good[0][1] != wrong[0][1]).any()      # (layer 1 has one parent per row)
    good = nref.sample(oracle, rows, seeds, [5, 4], seed=3, replace=False)
    wrong = nref.sample(oracle, rows, seeds, [5, 4], seed=3, replace=False, defect="floyd_j_minus_1")
    assert good[2] >= 1 and any((a != b).any() for a, b in zip(good[0], wrong[0]))
    # ... and on the graph worked by hand: the seed index keys the draw, so vertex 0's two subtrees differ; keyed by the id they would not
    h = hand_graph(oracle)
    by_id = nref.sample(oracle, h.neighbors, HAND_SEEDS, [3, 2], seed=5, epoch=2, defect="vertex_key")[0]
    assert all(np.array_equal(L[0], L[5]) for L in by_id)


def test_the_floyd_inputs_collide(oracle):
    """every group width takes the "already taken -> J" branch in the GPU file's inputs, and the karate cases do too"""
    for f in D_FANOUTS:
        rows = distinct_rows(f)
        _, unknown, collisions = nref.sample(oracle, rows_provider(rows), D_SEEDS, [f], seed=11, replace=False)
        print("f = %d: %d Floyd collisions" % (f, collisions))
        assert unknown == 0 and (collisions >= 1 if f > 1 else collisions == 0), f      # (one child has no earlier child to collide with)
    g = oracle.Graph.load(KARATE, directed=False)
    for fan in ([3, 2], [5, 1, 4]):
        assert nref.sample(oracle, g.neighbors, karate_seeds(g), fan, seed=1, replace=False)[2] >= 1, fan


def test_the_weighted_inputs_reach_every_arm_of_the_draw(oracle):
    """regular rows, the irregular row, and compact records that need more than one read (tests/first_order_code_ref.py's pick)"""
    rows = weighted_rows()
    nb = nref.Rows(rows_provider(rows))
    seeds = weighted_seeds()
    layers, unknown, _ = nref.sample(oracle, nb, seeds, W_FANOUTS, seed=1, epoch=0)
    assert unknown == 3                                                  # 21 has no row, 100, -1
    F = nref.row_lengths(W_FANOUTS)
    prev = np.array(seeds).reshape(-1, 1)
    regular = irregular = multi_read = dead_children = 0
    built = {}
    for l, f in enumerate(W_FANOUTS, start=1):
        W = nref.words(np.arange(len(seeds)), F[l], l, 0, 1)
        for b in range(len(seeds)):
            for j in range(F[l]):
                p = int(prev[b, j // f])
                r = nb(p)
                if r is None or len(r[0]) == 0:
                    dead_children += p == W_DEAD
                    continue
                if p == W_IRREGULAR:
                    irregular += 1
                    continue
                regular += 1
                if p not in built:
                    built[p] = foref.build(r[1])
                c, code = built[p]
                k, reads = foref.pick(c, code, int(W[b, j]) >> 8)
                assert r[0][k] == layers[l - 1][b, j]                     # the compact pick's model agrees with the oracle's draw
                multi_read += reads > 1
        prev = layers[l - 1]
    print("regular %d, irregular %d, more than one read %d, children of the dead end %d" % (regular, irregular, multi_read, dead_children))
    assert regular >= 100 and irregular >= 4 and multi_read >= 10 and dead_children >= 8
    assert (layers[1][W_DEAD] == -1).all() and (layers[0][W_DEAD] == -1).all()     # the dead end's children and grandchildren
    assert set(len(nb(v)[0]) for v in range(18)) == set(W_DEGS)
