"""srw_vertex_types_set / srw_vertex_types / srw_walk_metapath and Engine.set_vertex_types / vertex_types_len / walk_metapath — what can be
checked without a GPU: the symbols, their declarations, the refusals that come before a handle or a device is touched, and the footing of
the restatement the GPU tests hold every walker to (tests/metapath_ref.py): it is the oracle's walk where the filter lets everything
through, a graph of five vertices worked by hand, three planted misreadings of the header comment that it must notice, and the
condition on the inputs tests/test_gpu_metapath.py uses (the filter is exercised and most walks still walk)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import metapath_ref as mref
from conftest import KARATE, ROOT
from helpers import pkg


def test_the_library_exports_the_entry_points():
    P = pkg()
    for s in ("srw_vertex_types_set", "srw_vertex_types", "srw_walk_metapath"):
        assert s in P.EXPORTS and hasattr(P.lib(), s)


def test_the_header_declares_the_functions_and_states_the_semantics():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "stellar_rw.h")).read())
    assert "int32_t srw_vertex_types_set(srw_handle *h, const void *d_types, int64_t n);" in flat
    assert "int32_t srw_vertex_types(const srw_handle *h, int64_t *n);" in flat
    assert ("int32_t srw_walk_metapath(srw_handle *h, const srw_walk_params *params, const int32_t *pattern, int32_t m, "
            "srw_walk_stats *stats);") in flat
    for said in ("pattern[j mod m]", "pattern[s mod m]", "IN ROW ORDER", "THAT SUBLIST", "sublist's HEAD", "one-entry path [src]",
                 "kernel_kind = 4", "bit for bit srw_walk's", "d_types == NULL clears", "Loading a graph drops them",
                 "no types in force (even for an all-wildcard pattern)", "4 = metapath"):
        assert said in flat, said


def test_the_kernels_are_on_the_build_list():
    csrc = os.path.join(ROOT, "stellar-random-walk_amd", "csrc")
    assert re.search(r"^HIP_SRC\s*:=.*\bmetapath\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    src = open(os.path.join(csrc, "metapath.hip")).read()
    for k in ("k_entry_types", "k_walk_metapath", "wave_pick_typed"):
        assert k in src


def test_null_arguments_are_refused_not_touched():
    """No handle can exist here (srw_create needs a device): what is reachable is the refusal of a NULL h / n."""
    P = pkg()
    L = P.lib()
    n = C.c_int64(-7)
    assert L.srw_vertex_types_set(None, None, 0) == P.ERR_INVALID
    assert L.srw_vertex_types_set(None, C.c_void_p(64), 3) == P.ERR_INVALID
    assert L.srw_vertex_types(None, C.byref(n)) == P.ERR_INVALID
    assert n.value == -7
    wp, st = P.Engine.params(walk_length=3), P.WalkStats()
    pat = (C.c_int32 * 2)(0, 1)
    assert L.srw_walk_metapath(None, C.byref(wp), pat, 2, C.byref(st)) == P.ERR_INVALID
    assert L.srw_walk_metapath(None, None, None, 0, None) == P.ERR_INVALID
    assert st.n_walkers == 0 and st.kernel_kind == 0


def test_engine_methods_have_the_agreed_parameters():
    E = pkg().Engine
    assert list(inspect.signature(E.set_vertex_types).parameters) == ["self", "types"]
    assert list(inspect.signature(E.vertex_types_len).parameters) == ["self"]
    sig = inspect.signature(E.walk_metapath)
    assert list(sig.parameters) == ["self", "pattern", "fetch", "sources", "kw"]
    assert (sig.parameters["fetch"].default, sig.parameters["sources"].default) == (True, None)
    assert sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert "pattern[j mod m]" in E.walk_metapath.__doc__ and "set_vertex_types" in E.walk_metapath.__doc__


def engine_without_a_handle():
    """Anything that reached the library would fail differently (there is no GPU here, and the handle is NULL)."""
    P = pkg()
    e = P.Engine.__new__(P.Engine)
    e.h, e.device = None, 0
    return e


def test_vertex_types_are_refused_before_the_library_is_called():
    e = engine_without_a_handle()
    t = torch.zeros((6,), dtype=torch.uint8)
    bad = [
        (t, "in device memory"),
        (t.to(torch.int32), r"must be torch\.uint8"),
        (t.to(torch.int8), r"must be torch\.uint8"),
        (t.to(torch.float32), r"must be torch\.uint8"),
        (t.view(2, 3), "one-dimensional"),
        (torch.zeros((12,), dtype=torch.uint8)[::2], "contiguous"),
        (np.zeros((2, 3), dtype=np.uint8), "one-dimensional"),
        (np.zeros(4, dtype=np.float32), "must be integers"),
        ([0.5, 1.0], "must be integers"),
        ([True, False], "must be integers"),
        ([0, 1, 256], r"outside the range 0 \.\. 255"),
        ([0, -1, 2], r"outside the range 0 \.\. 255"),
        (np.array([0, 1 << 40]), r"outside the range 0 \.\. 255"),
        (7, "one-dimensional"),
    ]
    for types, why in bad:
        with pytest.raises(TypeError, match="set_vertex_types.*" + why):
            e.set_vertex_types(types)


def test_patterns_are_refused_before_the_library_is_called():
    e = engine_without_a_handle()
    bad = [
        ([], r"1 \.\. 64 entries"),
        ([0] * 65, r"1 \.\. 64 entries"),
        ([[0, 1]], r"1 \.\. 64 entries"),
        ([0, 1.5], "must be integers"),
        (["a"], "must be integers"),
        ([True], "must be integers"),
        ([0, 256], r"outside -1 \.\. 255"),
        ([-2, 0], r"outside -1 \.\. 255"),
        ("01", "sequence of integers"),
        (3, "sequence of integers"),
        (None, "sequence of integers"),
    ]
    for pattern, why in bad:
        with pytest.raises(TypeError, match="walk_metapath.*" + why):
            e.walk_metapath(pattern, walk_length=3)
        with pytest.raises(TypeError, match="walk_metapath.*" + why):       # ... and before the start list is touched
            e.walk_metapath(pattern, sources=[0, 1], walk_length=3)
    P = pkg()
    assert P.Engine._metapath_pattern([0, -1, 255]).tolist() == [0, -1, 255]
    assert P.Engine._metapath_pattern(np.arange(64)).dtype == np.int32
    assert P.Engine._metapath_pattern((7,)).tolist() == [7]


# ---- the restatement's own footing --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def karate(oracle):
    return {d: oracle.Graph.load(KARATE, directed=d) for d in (False, True)}


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("rng,const_r", [("philox", 0.0), ("const", 1.0), ("const", 0.0)])
def test_where_the_filter_lets_everything_through_it_is_the_oracles_walk(oracle, karate, directed, rng, const_r):
    g = karate[directed]
    nV = g.num_vertices
    kw = dict(walk_length=20, num_walks=2, first_walk=3, rng=rng, const_r=const_r, seed=11)
    ref = g.walk(p=1.0, q=1.0, **kw)
    mixed = (g.vertices() % 3).astype(np.int64)
    for types, pattern in ((mixed, [-1]), (mixed, [-1, -1, -1]), (np.full(nV, 7), [7]), (np.zeros(nV, dtype=np.int64), [0])):
        paths, lens, steps, dead = mref.walk(oracle, g, types, pattern, **kw)
        assert np.array_equal(lens, ref[1]) and np.array_equal(paths, ref[0]), (pattern, np.flatnonzero((paths != ref[0]).any(axis=1))[:5])
        assert steps == ref[2] == int((lens - 1).sum())
        assert dead == int(((lens >= 2) & (lens < kw["walk_length"] + 2)).sum())


def test_sample_py_is_the_oracles_sample(oracle):
    rng = np.random.default_rng(5)
    rows = [np.ones(n, dtype=np.float32) for n in (1, 2, 3, 6, 7, 10, 64)]
    rows += [np.array(r, dtype=np.float32) for r in ([98.8, 46.6, 21.6], [61.2, 11.5, 4.4], [0.0, 2.0, 0.0, 1.0])]
    rows += [rng.choice(np.array([1e-8, 0.5, 1.0, 3.25, 1000.0, 3e7], dtype=np.float32), size=n) for n in (5, 17, 40)]
    for w in rows:
        for r in (0.0, 0.25, 0.5, 1.0, 0.99999994, float(rng.random())):
            k, found = mref.sample_py(w, r)
            assert k == oracle.sample_index(w, r), (w, r)
            assert found or k == 0
    # the rows the GPU file plants behind a head that does not match: at r = 1 the oracle falls back to the head
    for w in ([98.8, 46.6, 21.6], [61.2, 11.5, 4.4], [1.0] * 6, [1.0] * 7, [1.0] * 10):
        assert mref.sample_py(np.array(w, dtype=np.float32), 1.0) == (0, False)
    for n in (4, 5, 8):
        assert mref.sample_py(np.ones(n, dtype=np.float32), 1.0) == (n - 1, True)


# Five vertices, directed, rows in line order.  Types: 0 -> a, 1 -> b, 2 -> b, 3 -> a, 4 -> b (destination only).
#   N(0) = [3 (w 1), 1 (w 1), 2 (w 2), 4 (w 1)]     the head is of type a
#   N(1) = [0 (w 1), 3 (w 3)]
#   N(2) = [2 (w 1, a self-loop), 0 (w 1)]
#   N(3) = [4 (w 1)]
#   N(4) = []
HAND_LINES = [(0, 3, 1.0), (0, 1, 1.0), (0, 2, 2.0), (0, 4, 1.0), (1, 0, 1.0), (1, 3, 3.0), (2, 2, 1.0), (2, 0, 1.0), (3, 4, 1.0)]
HAND_TYPES = [0, 1, 1, 0, 1]
# pattern [a, b], walk_length 2: positions 0 .. 3 need a, b, a, b.  Sources 1, 2 and 4 are of type b: the one-entry path.
#   source 0, step 1 (needs b): the sublist of N(0) is [1, 2, 4] with weights 1, 2, 1 -> S = 4, acc = .25, .75, 1
#       r = 0 -> 1 (the first candidate, not the head 3);  r = .5 -> 2;  r = 1 -> 4
#     r = 0:  step 2 from 1 (needs a): [0, 3], weights 1, 3 -> acc = .25 >= 0 -> 0;  step 3 from 0 (needs b) -> 1         [0, 1, 0, 1]
#     r = .5: step 2 from 2 (needs a): the self-loop is of type b, the sublist is [0] -> 0;  step 3 from 0 -> 2            [0, 2, 0, 2]
#     r = 1:  step 2 from 4: an empty row, at a step s > 1: a dead end                                                     [0, 4]
#   source 3, step 1 (needs b): [4] -> 4 for every r;  step 2 from 4: an empty row: a dead end                             [3, 4]
HAND = {
    0.0: ([[0, 1, 0, 1], [1], [2], [3, 4], [4]], 4, 1),
    0.5: ([[0, 2, 0, 2], [1], [2], [3, 4], [4]], 4, 1),
    1.0: ([[0, 4], [1], [2], [3, 4], [4]], 2, 2),
}


def hand_graph(oracle):
    s, d, w = (np.array(c) for c in zip(*HAND_LINES))
    return oracle.Graph.from_coo(s, d, w.astype(np.float32), directed=True)


@pytest.mark.parametrize("r", sorted(HAND))
def test_five_vertices_worked_by_hand(oracle, r):
    g = hand_graph(oracle)
    assert g.vertices().tolist() == [0, 1, 2, 3, 4]
    want, want_steps, want_dead = HAND[r]
    paths, lens, steps, dead = mref.walk(oracle, g, HAND_TYPES, [0, 1], walk_length=2, rng="const", const_r=r)
    assert [p[:n].tolist() for p, n in zip(paths, lens)] == want
    assert (paths[np.arange(4)[None, :] >= lens[:, None]] == -1).all()
    assert (steps, dead) == (want_steps, want_dead)


# ---- the inputs of the GPU file's karate cases ------------------------------------------------------------------------------------------
KARATE_CASE = dict(walk_length=20, num_walks=4, seed=42)


def karate_case(oracle, g, **kw):
    return mref.walk(oracle, g, (g.vertices() % 2).astype(np.int64), [0, 1], **dict(KARATE_CASE, **kw))


def test_planted_misreadings_are_noticed(oracle, karate):
    """Each one changes at least one row of the karate case, under the draw that reaches the rule it breaks."""
    g = karate[False]
    for defect, rng_kw in (("zero_weight", dict(rng="const", const_r=0.0)),     # acc >= 0 already holds at a head that does not match
                           ("head0", dict(rng="const", const_r=1.0)),           # six unit weights never reach 1: the SUBLIST's head
                           ("s_minus_1", dict(rng="philox"))):
        good = karate_case(oracle, g, **rng_kw)
        wrong = karate_case(oracle, g, defect=defect, **rng_kw)
        assert (good[0] != wrong[0]).any(axis=1).sum() >= 1, defect
    # ... and a planted misreading shows in the hand-worked graph too: a candidate of weight zero at the head of N(0)
    paths, lens, _, _ = mref.walk(oracle, hand_graph(oracle), HAND_TYPES, [0, 1], walk_length=2, rng="const", const_r=0.0, defect="zero_weight")
    assert paths[0, 1] == 3


def test_the_karate_case_exercises_the_filter_and_most_walks_still_walk(oracle, karate):
    g = karate[False]
    L = KARATE_CASE["walk_length"]
    paths, lens, steps, dead = karate_case(oracle, g)
    plain = g.walk(p=1.0, q=1.0, rng="philox", **KARATE_CASE)
    full = float((lens == L + 2).mean())
    multi = lens > 1
    differ = (paths != plain[0]).any(axis=1)
    print("full length: %.3f of %d walkers; multi-entry rows: %d, of which %d differ from the plain walk's" %
          (full, len(lens), int(multi.sum()), int((multi & differ).sum())))
    assert full >= 0.40
    assert multi.any() and (differ[multi]).all()
    # every row obeys the pattern, and the rows of the wrong-typed sources are the one-entry paths
    tp = dict(zip(g.vertices().tolist(), (g.vertices() % 2).tolist()))
    for p, n in zip(paths, lens):
        if tp[int(p[0])] == 1:
            assert n == 1
        else:
            assert all(tp[int(v)] == j % 2 for j, v in enumerate(p[:n]))
