"""srw_topk_rows / srw_vertex_rows and Engine.topk_rows / rows_of / most_similar — what can be checked without a GPU: the symbols, their
declarations, the struct, the refusals that come before a handle or a device is touched, and the footing of the numpy restatement and
of the rule the GPU tests hold every result to (tests/topk_ref.py): a table worked by hand, planted wrong answers on the inputs
tests/test_gpu_topk.py uses, and the cap on how many queries leave the rule any freedom."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import topk_ref as tref
from conftest import ROOT
from helpers import pkg


def test_the_library_exports_the_entry_points():
    P = pkg()
    for s in ("srw_topk_rows", "srw_vertex_rows"):
        assert s in P.EXPORTS and hasattr(P.lib(), s)


def test_the_header_declares_the_struct_and_the_functions():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "stellar_rw.h")).read())
    assert "typedef struct { int32_t dim; int32_t k; int32_t metric; int32_t reserved; } srw_topk_params;" in flat
    assert ("int32_t srw_topk_rows(srw_handle *h, const void *d_table /* float32 [n_rows][dim] */, int64_t n_rows, "
            "const void *d_qvec /* float32 [n_queries][dim] or NULL */, const void *d_qrow /* int32 [n_queries] or NULL */, "
            "int64_t n_queries, const srw_topk_params *tp, "
            "void *d_rows /* int32 [n_queries][k] */, void *d_scores /* float32 [n_queries][k] */, "
            "int64_t *n_skipped /* or NULL */);") in flat
    assert ("int32_t srw_vertex_rows(srw_handle *h, const void *d_ids /* int32 [n] */, int64_t n, void *d_rows /* int32 [n] */, "
            "int64_t *n_unknown /* or NULL */);") in flat
    for said in ("findSynonyms", "exactly 0", "NaN score ranks", "score descending, row ascending", "row -1, score -inf", "overflow"):
        assert said in flat, said


def test_the_kernels_are_on_the_build_list():
    csrc = os.path.join(ROOT, "stellar-random-walk_amd", "csrc")
    assert re.search(r"^HIP_SRC\s*:=.*\btopk\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    assert os.path.exists(os.path.join(csrc, "topk.hip"))


def test_the_struct_has_the_declared_fields_and_size():
    P = pkg()
    assert [f[0] for f in P.TopkParams._fields_] == ["dim", "k", "metric", "reserved"]
    assert C.sizeof(P.TopkParams) == 16
    tp = P.TopkParams(128, 10, 1, 0)
    assert (tp.dim, tp.k, tp.metric, tp.reserved) == (128, 10, 1, 0)
    assert [getattr(P.TopkParams, f).offset for f in ("dim", "k", "metric", "reserved")] == [0, 4, 8, 12]
    assert P.TOPK_METRICS == {"cosine": 0, "dot": 1}


def test_null_arguments_are_refused_not_touched():
    """No handle can exist here (srw_create needs a device): what is reachable is the refusal of a NULL h / tp."""
    P = pkg()
    L = P.lib()
    tp, n = P.TopkParams(64, 10, 0, 0), C.c_int64(-7)
    assert L.srw_topk_rows(None, None, 0, None, None, 0, C.byref(tp), None, None, C.byref(n)) == P.ERR_INVALID
    assert L.srw_topk_rows(None, None, 0, None, None, 0, None, None, None, C.byref(n)) == P.ERR_INVALID
    assert L.srw_vertex_rows(None, None, 0, None, C.byref(n)) == P.ERR_INVALID
    assert n.value == -7


def test_engine_methods_have_the_agreed_parameters():
    E = pkg().Engine
    sig = inspect.signature(E.topk_rows)
    assert list(sig.parameters) == ["self", "table", "k", "rows", "vectors", "metric"]
    assert [sig.parameters[k].default for k in ("rows", "vectors", "metric")] == [None, None, "cosine"]
    sig = inspect.signature(E.rows_of)
    assert list(sig.parameters)[:2] == ["self", "ids"]
    assert all(p.default is not inspect.Parameter.empty for p in list(sig.parameters.values())[2:])
    sig = inspect.signature(E.most_similar)
    assert list(sig.parameters) == ["self", "emb", "ids", "k", "metric"]
    assert (sig.parameters["k"].default, sig.parameters["metric"].default) == (10, "cosine")
    assert "w2v_fit" in E.most_similar.__doc__ and "topk_rows" in E.most_similar.__doc__


def test_tensor_arguments_are_refused_before_the_library_is_called():
    """An Engine without a handle: anything that reached the library would fail differently (there is no GPU here)."""
    P = pkg()
    e = P.Engine.__new__(P.Engine)
    e.h, e.device = None, 0
    table = torch.zeros((9, 6), dtype=torch.float32)
    rows = torch.zeros((4,), dtype=torch.int32)
    vec = torch.zeros((4, 6), dtype=torch.float32)
    bad = [
        (table, rows, None, "in device memory"),
        (table, None, vec, "in device memory"),
        (table, rows, vec, "in device memory"),
        (table, None, None, "at least one of rows and vectors"),
        (table.double(), rows, None, r"table must be torch\.float32"),
        (table, rows.long(), None, r"rows must be torch\.int32"),
        (table, rows, vec.half(), r"vectors must be torch\.float32"),
        (table[:, ::2], rows, None, "table must be contiguous"),
        (table, rows[::2], None, "rows must be contiguous"),
        (table, None, vec[:, ::2], r"vectors must be \[Q, D\]"),
        (table, None, torch.zeros((4, 12))[:, ::2], "vectors must be contiguous"),
        (table[0], rows, None, r"table must be \[n, D\]"),
        (table, rows.view(2, 2), None, r"rows must be \[Q\]"),
        (table, rows[:3], vec, r"rows must be \[Q\]"),
        (table, None, vec[0], r"vectors must be \[Q, D\]"),
        (table, None, torch.zeros((4, 5)), r"vectors must be \[Q, D\]"),
        (table.numpy(), rows, None, "table must be a torch tensor"),
        (table, rows.numpy(), None, "rows must be a torch tensor"),
        (table, None, vec.numpy(), "vectors must be a torch tensor"),
    ]
    for t, r, v, why in bad:
        with pytest.raises(TypeError, match="topk_rows.*" + why):
            e.topk_rows(t, 3, rows=r, vectors=v)
    with pytest.raises(TypeError, match="rows_of.*torch.int32"):
        e.rows_of(torch.zeros((4,), dtype=torch.int64))
    with pytest.raises(TypeError, match="rows_of.*one-dimensional"):
        e.rows_of(torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(TypeError, match="rows_of.*handle's device"):
        e.rows_of(torch.zeros((4,), dtype=torch.int32))


# ---- the restatement's own footing --------------------------------------------------------------------------------------------------
HAND = np.array([[1, 0, 0], [0, 2, 0], [1, 1, 0], [0, 0, 0], [-1, 0, 0], [2, 0, 0], [1, 1, 0]], dtype=np.float32)


def double_loop(table, q, metric):
    out = []
    for r in range(len(table)):
        dot = qq = rr = 0.0
        for d in range(table.shape[1]):
            dot += float(q[d]) * float(table[r, d]); qq += float(q[d]) ** 2; rr += float(table[r, d]) ** 2
        out.append(dot if metric == "dot" else (0.0 if qq == 0 or rr == 0 else dot / (qq ** 0.5 * rr ** 0.5)))
    return out


def test_the_restatement_on_a_table_worked_by_hand():
    h = 0.5 ** 0.5
    # query = row 0 = (1, 0, 0), itself excluded: dots 0 1 0 -1 2 1 of rows 1 .. 6; rows 2 and 6 are equal, row 3 is zero
    r = tref.topk(HAND, 4, rows=[0], metric="dot")
    assert r.rows.tolist() == [[5, 2, 6, 1]] and r.scores.tolist() == [[2.0, 1.0, 1.0, 0.0]] and r.skipped == 0
    r = tref.topk(HAND, 4, rows=[0], metric="cosine")
    assert r.rows.tolist() == [[5, 2, 6, 1]] and np.allclose(r.scores, [[1.0, h, h, 0.0]], rtol=1e-15) and r.scores[0, 3] == 0
    r = tref.topk(HAND, 8, rows=[0, 7, -1], metric="cosine")               # six eligible rows; 7 and, by row, -1 are no rows
    assert r.rows.tolist() == [[5, 2, 6, 1, 3, 4, -1, -1]] + [[-1] * 8] * 2 and r.skipped == 2
    assert r.scores[0, 4] == 0 and r.scores[0, 5] == -1 and (r.scores[0, 6:] == -np.inf).all() and (r.scores[1:] == -np.inf).all()
    r = tref.topk(HAND, 3, vectors=[[0, 1, 0]], metric="dot")              # nothing excluded
    assert r.rows.tolist() == [[1, 2, 6]] and r.scores.tolist() == [[2.0, 1.0, 1.0]]
    r = tref.topk(HAND, 3, vectors=[[0, 1, 0]] * 3, rows=[1, -1, 9], metric="dot")
    assert r.rows.tolist() == [[2, 6, 0], [1, 2, 6], [-1, -1, -1]] and r.skipped == 1
    r = tref.topk(HAND, 2, vectors=[[0, 0, 0]], metric="cosine")           # a zero query scores 0 everywhere: the first rows win
    assert r.rows.tolist() == [[0, 1]] and r.scores.tolist() == [[0.0, 0.0]]
    nan = HAND.copy(); nan[5, 1] = np.nan
    r = tref.topk(nan, 7, vectors=[[1, 0, 0]], metric="dot")               # the NaN row ranks last, as -inf
    assert r.rows[0, -1] == 5 and r.scores[0, -1] == -np.inf and r.rows[0, 0] == 0
    for metric in tref.METRICS:
        for q in ([1, 0, 0], [0.5, -2, 3], [0, 0, 0]):
            S, eps = tref.all_scores(HAND, [q], metric)
            assert np.allclose(S[0], double_loop(HAND, q, metric), rtol=1e-15, atol=0)
    S, eps = tref.all_scores(HAND, [[0.5, -2, 3]], "dot")
    assert np.allclose(eps[0], 5 * tref.U * np.abs(HAND * np.array([0.5, -2, 3])).sum(axis=1))
    assert (tref.all_scores(HAND, [[1, 0, 0]], "cosine")[1] == 14 * tref.U).all()


def test_the_rule_accepts_the_reference_and_a_float32_evaluation():
    n, D, k = tref.TOLERANCE_CASES[0]
    table, rows = tref.case_inputs(n, D, k)
    for metric in tref.METRICS:
        ref = tref.topk(table, k, rows=rows, metric=metric)
        assert tref.check(ref, ref.rows, ref.scores.astype(np.float32)) <= 1.0 / (D + 2)               # one rounding of the score: u |s|
        # float32 arithmetic in a naive order, ranked by its own scores
        q = table[rows]
        dot = np.zeros((len(rows), n), dtype=np.float32)
        for d in range(D):
            dot += q[:, d:d + 1] * table[None, :, d]
        if metric == "cosine":
            nq = np.sqrt((q * q).sum(axis=1, dtype=np.float32)); nr = np.sqrt((table * table).sum(axis=1, dtype=np.float32))
            dot = dot / (nq[:, None] * nr[None, :])
        dot[np.arange(len(rows)), rows] = -np.inf
        got = np.argsort(-dot, axis=1, kind="stable")[:, :k]
        worst = tref.check(ref, got, np.take_along_axis(dot, got, axis=1))
        assert worst < 0.2, (metric, worst)


def planted(ref, table, rows, metric):
    """(name, rows, scores) of wrong answers cut from the reference's own"""
    good_r, good_s = ref.rows.copy(), ref.scores.astype(np.float32)
    k = ref.k
    out = []
    i = 3
    t, E = tref._band(ref, i)
    low = np.nonzero(ref.eligible[i] & (ref.S[i] < t - 4 * E))[0]
    r, s = good_r.copy(), good_s.copy()
    r[i, k - 1] = low[np.argmax(ref.S[i, low])]                            # the best of the rows more than 4 eps below the k-th
    s[i, k - 1] = ref.S[i, r[i, k - 1]]
    out.append(("the k-th row replaced by one more than 4 eps below it", r, s))
    r, s = good_r.copy(), good_s.copy()
    q, row = table[rows[i]].astype(np.float64), table[good_r[i, 0]].astype(np.float64)
    if metric == "dot":
        s[i, 0] = (q[:-1] * row[:-1]).sum()
    else:
        s[i, 0] = (q[:-1] * row[:-1]).sum() / np.sqrt((q[:-1] ** 2).sum() * (row[:-1] ** 2).sum())
    out.append(("a score with its last element dropped", r, s))
    r, s = good_r.copy(), good_s.copy()
    r[i, 0] = rows[i]
    s[i, 0] = ref.S[i, rows[i]]
    out.append(("an excluded row returned", r, s))
    r, s = good_r.copy(), good_s.copy()
    r[i, k - 1], s[i, k - 1] = -1, -np.inf
    out.append(("a padding row where a row was eligible", r, s))
    return out


@pytest.mark.parametrize("metric", tref.METRICS)
def test_the_rule_rejects_planted_wrong_answers(metric):
    n, D, k = tref.TOLERANCE_CASES[0]
    table, rows = tref.case_inputs(n, D, k)
    ref = tref.topk(table, k, rows=rows, metric=metric)
    tref.check(ref, ref.rows, ref.scores.astype(np.float32))
    for name, r, s in planted(ref, table, rows, metric):
        with pytest.raises(AssertionError, match="query 3"):
            tref.check(ref, r, s)
            pytest.fail("not noticed: " + name)
    # two tied rows swapped: the table whose every vector stands at five far-apart rows
    table, qvec = tref.repeated_table()
    ref = tref.topk(table, 20, vectors=qvec, metric=metric)
    s = ref.scores.astype(np.float32)
    tref.check(ref, ref.rows, s)
    assert s[2, 5] == s[2, 6] and ref.rows[2, 5] < ref.rows[2, 6]
    r = ref.rows.copy()
    r[2, [5, 6]] = r[2, [6, 5]]
    with pytest.raises(AssertionError, match="query 2: equal score bits out of row order"):
        tref.check(ref, r, s)


@pytest.mark.parametrize("n,D,k", tref.TOLERANCE_CASES)
@pytest.mark.parametrize("metric", tref.METRICS)
def test_at_most_one_query_in_five_is_ambiguous(n, D, k, metric):
    """so that the band of clause 4 hides nothing: from the reference alone"""
    table, rows = tref.case_inputs(n, D, k)
    for ref in (tref.topk(table, k, rows=rows, metric=metric), tref.topk(table, k, vectors=table[rows], metric=metric)):
        amb = tref.ambiguous(ref)
        print("n %d D %d k %d %s: %d of %d queries ambiguous" % (n, D, k, metric, amb, len(rows)))
        assert 5 * amb <= len(rows)


def test_integer_tables_are_exact_in_float32():
    t = tref.integer_table(50, 1024, 1)
    assert np.abs(t).max() == 4 and (t == np.round(t)).all()
    assert 1024 * 16 < 2 ** 24                                             # every partial sum of 1024 products of such values is an exact float32
