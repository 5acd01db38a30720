"""srw_topk_rows / srw_vertex_rows and Engine.topk_rows / rows_of / most_similar on the device against the float64 restatement of the
header (tests/topk_ref.py; its footing: tests/test_topk_cpu.py).  Two kinds of check: EXACT ones — the dot metric on tables of integers
in -4 .. 4, where every partial sum is an exact float32 in any order and ties are everywhere, so rows and score bits must equal the
reference outright — at every size where the kernels take another path (a tile of 128 rows, one grid pass of CUs x 3 tiles, a pass of
32 / 16 / 8 queries, chunks of 32 dimensions); and TOLERANCE ones under the rule of topk_ref.check, on the shapes whose ambiguity cap
the CPU file asserts.  Each tolerance check prints its worst score error / eps.  Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import topk_ref as tref
from conftest import KARATE
from helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 128                                                                 # rows per block tile (topk.hip)
WORST = {}                                                                 # what -> worst score error / eps, for the last test to print


def qb_of(D):
    return 32 if D <= 256 else 16 if D <= 512 else 8


def grid_rows():
    return torch.cuda.get_device_properties(0).multi_processor_count * 3 * TILE


def dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)                # (a copy: the shared inputs are read-only)


def i32(a):
    return None if a is None else dev(np.asarray(a, dtype=np.int32))


def f32(a):
    return None if a is None else dev(np.asarray(a, dtype=np.float32))


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)                                             # no graph: the search needs none
    yield e
    e.close()


def run(e, table, k, rows=None, vectors=None, metric="dot"):
    t = table if torch.is_tensor(table) else f32(table)
    r, s, skipped = e.topk_rows(t, k, rows=i32(rows), vectors=vectors if torch.is_tensor(vectors) else f32(vectors), metric=metric)
    assert r.dtype == torch.int32 and s.dtype == torch.float32 and tuple(r.shape) == tuple(s.shape)
    return r.cpu().numpy(), s.cpu().numpy(), skipped


def exact(e, table, k, rows=None, vectors=None):
    ref = tref.topk(table, k, rows=rows, vectors=vectors, metric="dot")
    r, s, skipped = run(e, table, k, rows, vectors, "dot")
    tref.check_exact(ref, r, s)
    assert skipped == ref.skipped
    return ref


def held(what, e, table, k, rows=None, vectors=None, metric="cosine"):
    ref = tref.topk(table, k, rows=rows, vectors=vectors, metric=metric)
    r, s, skipped = run(e, table, k, rows, vectors, metric)
    worst = tref.check(ref, r, s)
    print("%s: worst score error / eps %.4f" % (what, worst))
    WORST[what] = worst
    assert skipped == ref.skipped
    return ref, r, s


def int_queries(Q, D, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=(Q, D)).astype(np.float32)


# ---- exact: the dot metric on integer tables --------------------------------------------------------------------------------------------
def test_exact_row_counts(eng):
    D, k = 5, 2
    vec = int_queries(3, D, 1)
    for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, grid_rows() - 1, grid_rows() + 1):      # ..., and more than one grid pass
        table = tref.integer_table(n, D, n)
        exact(eng, table, k, vectors=vec)
        exact(eng, table, k, rows=[0, n - 1, n // 2])


@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_exact_k(eng, k):
    table = tref.integer_table(700, 3, 2)                                  # 729 possible rows among 700: ties at every score
    exact(eng, table, k, vectors=int_queries(5, 3, 3))
    exact(eng, table, k, rows=[0, 699, 128, 127, 350])


def test_exact_k_above_the_row_count(eng):
    table = tref.integer_table(40, 4, 4)
    ref = exact(eng, table, 64, vectors=int_queries(3, 4, 5))
    assert (ref.rows[:, 40:] == -1).all() and (ref.rows[:, :40] >= 0).all()
    ref = exact(eng, table, 64, rows=[0, 39, 17])
    assert (ref.rows[:, 39:] == -1).all() and (ref.rows[:, :39] >= 0).all()
    ref = exact(eng, table[:1], 2, rows=[0])                               # one row, and that one excluded: padding only
    assert ref.rows.tolist() == [[-1, -1]] and ref.skipped == 0


@pytest.mark.parametrize("D", [8, 300, 1024])
def test_exact_query_counts(eng, D):
    QB = qb_of(D)
    table = tref.integer_table(300, D, D)
    for Q in (1, QB - 1, QB, QB + 1, 3 * QB + 1 if D == 8 else 2 * QB + 1):       # ..., three passes
        exact(eng, table, 4, vectors=int_queries(Q, D, Q))
    rows = np.random.default_rng(D).integers(0, 300, size=2 * QB + 1)
    exact(eng, table, 4, rows=rows)


@pytest.mark.parametrize("D", [1, 3, 4, 5, 63, 64, 65, 129, 300, 1024])
def test_exact_dims(eng, D):
    table = tref.integer_table(257, D, 100 + D)
    exact(eng, table, 5, vectors=int_queries(9, D, D))
    exact(eng, table, 5, rows=[0, 256, 128, 127, 5])


@pytest.mark.parametrize("D", [4, 5])
def test_exact_base_four_bytes_past_a_16_byte_boundary(eng, D):
    n, Q = 300, 5
    table, vec = tref.integer_table(n, D, 6), int_queries(Q, D, 7)
    buf, qbuf = torch.zeros(n * D + 8, device=DEV), torch.zeros(Q * D + 8, device=DEV)
    t, v = buf[1:1 + n * D].view(n, D), qbuf[1:1 + Q * D].view(Q, D)
    t.copy_(f32(table)); v.copy_(f32(vec))
    assert t.data_ptr() % 16 == 4 and v.data_ptr() % 16 == 4 and t.is_contiguous()
    ref = tref.topk(table, 7, vectors=vec, metric="dot")
    r, s, _ = run(eng, t, 7, vectors=v)
    tref.check_exact(ref, r, s)
    ref = tref.topk(table, 7, rows=[0, 299, 3], metric="dot")
    r, s, _ = run(eng, t, 7, rows=[0, 299, 3])
    tref.check_exact(ref, r, s)


@pytest.mark.parametrize("k", [3, 64])
def test_exact_scores_ascending_and_descending_with_the_row(eng, k):
    n = 1000
    table = np.arange(n, dtype=np.float32).reshape(n, 1)
    ref = exact(eng, table, k, vectors=[[1.0], [-1.0]])                    # ascending: every tile inserts; descending: none after the first
    assert ref.rows[0].tolist() == list(range(n - 1, n - 1 - k, -1)) and ref.rows[1].tolist() == list(range(k))


def test_exact_all_rows_equal_and_exclusions_at_the_ends(eng):
    n = 500
    table = np.tile(np.array([[1, -2, 3]], dtype=np.float32), (n, 1))
    ref = exact(eng, table, 6, vectors=[[1, 1, 1]])
    assert ref.rows.tolist() == [list(range(6))]
    ref = exact(eng, table, 6, rows=[0, n - 1, 3])
    assert ref.rows.tolist() == [[1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5], [0, 1, 2, 4, 5, 6]]
    table = tref.integer_table(n, 6, 9)
    ref = exact(eng, table, 64, rows=[0, n - 1])
    assert 0 not in ref.rows[0] and n - 1 not in ref.rows[1]
    vec = table[[0, n - 1]]
    exact(eng, table, 64, vectors=vec, rows=[0, n - 1])
    exact(eng, table, 64, vectors=vec, rows=[-1, -1])                      # -1 with a vector: nothing excluded


@pytest.mark.parametrize("metric", tref.METRICS)
def test_repeated_vectors_come_back_adjacent_with_equal_bits(eng, metric):
    """every distinct vector stands at five rows, 150 rows apart: position independence"""
    table, qvec = tref.repeated_table()
    ref, r, s = held("repeated vectors, " + metric, eng, table, 20, vectors=qvec, metric=metric)
    for i in range(len(qvec)):
        for g in range(0, 20, 5):
            assert (r[i, g:g + 5] % 150 == r[i, g] % 150).all() and (np.diff(r[i, g:g + 5]) == 150).all(), (i, r[i])
            assert (s[i, g:g + 5].view(np.uint32) == s[i, g:g + 5].view(np.uint32)[0]).all(), (i, s[i])


# ---- under the rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,k", tref.TOLERANCE_CASES)
@pytest.mark.parametrize("metric", tref.METRICS)
def test_tolerance_cases(eng, n, D, k, metric):
    table, rows = tref.case_inputs(n, D, k)
    t, vec = table, table[rows]
    what = "n %d D %d k %d %s" % (n, D, k, metric)
    _, r_row, s_row = held(what + " by row", eng, t, k, rows=rows, metric=metric)
    _, r_vec, s_vec = held(what + " by vector", eng, t, k, vectors=vec, metric=metric)
    assert (r_vec[:, 0] == rows).all()                                     # nothing excluded: the query's own row leads
    ref, r_both, s_both = held(what + " by vector with exclusion", eng, t, k, vectors=vec, rows=rows, metric=metric)
    assert np.array_equal(r_row, r_both) and np.array_equal(s_row.view(np.uint32), s_both.view(np.uint32))
    assert tref.ambiguous(ref) * 5 <= len(rows)


def test_zero_rows_nan_rows_and_skipped_queries(eng):
    n, D, k = 500, 20, 10
    table = np.random.default_rng(12).standard_normal((n, D)).astype(np.float32)
    table[7] = 0.0
    table[11, 3] = np.nan
    rows = [3, 7, -1, n, 2**31 - 1, 5, 11]
    for metric in tref.METRICS:
        ref, r, s = held("zero / NaN / skipped, " + metric, eng, table, k, rows=rows, metric=metric)
        assert ref.skipped == 3
        assert (r[2:5] == -1).all() and (s[2:5] == -np.inf).all()          # padding, and the neighbours intact (held above)
        assert 11 not in r[0] and 11 not in r[5]
        if metric == "dot":                                                # a NaN query: every score ranks as -inf, the first rows win
            assert (r[6] == np.arange(k)).all() and (s[6] == -np.inf).all()
        else:                                                              # ... but for the zero row, whose cosine is 0 whatever the query
            assert r[6].tolist() == [7] + [x for x in range(k) if x != 7] and s[6, 0] == 0 and (s[6, 1:] == -np.inf).all()
            assert r[1].tolist() == list(range(7)) + [8, 9, 10] and (s[1] == 0).all() and not np.signbit(s[1]).any()       # the zero query
    # the NaN row last, as -inf, and the zero row at exactly 0: a table small enough for k to reach them
    small = table[:40]
    ref, r, s = held("zero / NaN rows in reach", eng, small, 64, vectors=small[[3, 5]], metric="cosine")
    assert (r[:, 39] == 11).all() and (s[:, 39] == -np.inf).all() and (r[:, 40:] == -1).all()
    for i in range(2):
        at = r[i].tolist().index(7)
        assert s[i, at] == 0 and not np.signbit(s[i, at])


def test_a_call_repeats_bit_for_bit_whatever_shares_its_pass(eng):
    n, D, k = tref.TOLERANCE_CASES[0]
    table, rows = tref.case_inputs(n, D, k)
    t = f32(table)
    for metric in tref.METRICS:
        r0, s0, _ = run(eng, t, k, rows=rows, metric=metric)
        r1, s1, _ = run(eng, t, k, rows=rows, metric=metric)
        assert np.array_equal(r0, r1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
        perm = np.random.default_rng(3).permutation(len(rows))
        r2, s2, _ = run(eng, t, k, rows=rows[perm], metric=metric)
        assert np.array_equal(r0[perm], r2) and np.array_equal(s0[perm].view(np.uint32), s2.view(np.uint32))
        ra, sa, _ = run(eng, t, k, rows=rows[:23], metric=metric)
        rb, sb, _ = run(eng, t, k, rows=rows[23:], metric=metric)
        assert np.array_equal(r0, np.concatenate([ra, rb])) and np.array_equal(s0.view(np.uint32), np.concatenate([sa, sb]).view(np.uint32))
        rk, sk, _ = run(eng, t, 3, rows=rows, metric=metric)               # ... nor on k
        assert np.array_equal(r0[:, :3], rk) and np.array_equal(s0[:, :3].view(np.uint32), sk.view(np.uint32))


def test_offsets_beyond_2_to_the_31_elements(eng):
    free, _ = torch.cuda.mem_get_info(0)
    if free < 20 * 2**30:
        pytest.skip("needs 20 GB of free device memory (an 8.6 GB table and float64 chunks of it), %.1f GB are free" % (free / 2**30))
    D, n, k, chunk = 1024, 2**21 + 5, 8, 2**16
    assert n * D > 2**31
    gen = torch.Generator(device=DEV).manual_seed(4)
    table = torch.empty((n, D), dtype=torch.float32, device=DEV)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        table[a:b] = torch.randint(-4, 5, (b - a, D), generator=gen, device=DEV, dtype=torch.int32)
    q = torch.randint(-4, 5, (3, D), generator=gen, device=DEV, dtype=torch.int32).float()
    best = torch.where(q >= 0, 4.0, -4.0)                                  # the rows no other can beat: 4 sum |q|
    table[n - 5:n - 2] = best
    table[n - 2:] = best[0]                                                # query 0's best three times over, the last two rows among them
    cand = [[], [], []]
    for a in range(0, n, chunk):                                           # float64, exact for these integers
        sc = table[a:a + chunk].double() @ q.double().T
        for j in range(3):
            v = sc[:, j]
            idx = torch.nonzero(v >= torch.topk(v, min(k, v.numel())).values[-1]).flatten()
            cand[j] += list(zip((-v[idx]).tolist(), (idx + a).tolist()))
        del sc
    want = [sorted(c)[:k] for c in cand]
    r, s, skipped = eng.topk_rows(table, k, vectors=q, metric="dot")
    r, s = r.cpu().numpy(), s.cpu().numpy()
    assert skipped == 0
    for j in range(3):
        assert r[j].tolist() == [row for _, row in want[j]], (j, r[j], want[j])
        assert s[j].astype(np.float64).tolist() == [-v for v, _ in want[j]], (j, s[j], want[j])
    assert r[0, :3].tolist() == [n - 5, n - 2, n - 1] and r[1, 0] == n - 4 and r[2, 0] == n - 3
    del table


# ---- ids to rows ----------------------------------------------------------------------------------------------------------------------------
def test_rows_of_on_karate_and_on_a_sparse_id_space():
    P = pkg()
    with P.Engine(device=0) as e:
        e.load_edgelist(KARATE, directed=False)
        V = e.vertices()
        ids = np.array([1, 34, 17, 0, 35, -1, 2**31 - 1, -2**31, 5, 5], dtype=np.int32)
        rows, unknown = e.rows_of(i32(ids), return_unknown=True)
        assert rows.dtype == torch.int32 and rows.is_cuda
        assert rows.cpu().tolist() == [0, 33, 16, -1, -1, -1, -1, -1, 4, 4] and unknown == 5
        assert e.rows_of(ids.tolist()).cpu().tolist() == rows.cpu().tolist() and e.rows_of(ids).cpu().tolist() == rows.cpu().tolist()
        assert e.rows_of(torch.empty((0,), dtype=torch.int32, device=DEV), return_unknown=True)[1] == 0
    present = np.array([-70000, -3, 5, 6, 900, 1000, 70000, 2**30], dtype=np.int32)
    src, dst = present, np.roll(present, 1)
    with P.Engine(device=0, compact_ids=True) as e:                        # ids resolved by search over the compacted list
        e.load_coo(src, dst, np.ones(len(src), dtype=np.float32))
        V = e.vertices()
        assert V.tolist() == sorted(present.tolist())
        ids = np.concatenate([V, [-70001, -2**31, 2**30 + 1, 2**31 - 1, 0, 7, 899, 901, 69999], V[::-1]]).astype(np.int32)
        rows, unknown = e.rows_of(i32(ids), return_unknown=True)
        at = np.searchsorted(V, ids)
        want = np.where((at < len(V)) & (V[np.minimum(at, len(V) - 1)] == ids), at, -1)
        assert rows.cpu().tolist() == want.tolist() and unknown == 9 == int((want < 0).sum())


GAP_IDS = [3, 4, 5, 7, 8, 9, 10, 12]                                       # vmin 3, vmax 12, gaps at 6 and 11 (dense ids)


def test_rows_of_with_gaps_in_a_dense_id_space():
    with pkg().Engine(device=0) as e:
        src = np.array(GAP_IDS, dtype=np.int32)
        e.load_coo(src, np.roll(src, 1), np.ones(len(src), dtype=np.float32))
        assert e.vertices().tolist() == GAP_IDS
        rows, unknown = e.rows_of(list(range(0, 16)), return_unknown=True)
        assert rows.cpu().tolist() == [GAP_IDS.index(v) if v in GAP_IDS else -1 for v in range(16)] and unknown == 8


# ---- most_similar ---------------------------------------------------------------------------------------------------------------------------
def test_most_similar_on_a_trained_karate_table():
    with pkg().Engine(device=0) as e:
        e.load_edgelist(KARATE, directed=False)
        V = e.vertices()
        emb_in, _, _ = e.train_sgns(64, 5, 5, 5, 34, walk_length=20)        # the call tests/test_gpu_sgns.py makes
        table = emb_in.cpu().numpy()
        ids = np.concatenate([V, [0, 99]]).astype(np.int32)
        for metric in tref.METRICS:
            nb, sc = e.most_similar(emb_in, i32(ids), k=5, metric=metric)
            assert nb.dtype == torch.int32 and tuple(nb.shape) == (36, 5) and sc.dtype == torch.float32
            nb, sc = nb.cpu().numpy(), sc.cpu().numpy()
            assert (nb[34:] == -1).all() and (sc[34:] == -np.inf).all()    # an id that is no vertex: a row of padding
            ref = tref.topk(table, 5, rows=np.concatenate([np.arange(34), [-1, -1]]), metric=metric)
            rows = np.where(nb >= 0, np.searchsorted(V, np.maximum(nb, V[0])), -1)
            assert np.array_equal(np.where(rows >= 0, V[np.maximum(rows, 0)], -1), nb)      # neighbour ids are vertices()[rows]
            WORST["most_similar, " + metric] = tref.check(ref, rows, sc)
            r2, s2, _ = e.topk_rows(emb_in, 5, rows=e.rows_of(i32(ids)), metric=metric)
            assert np.array_equal(r2.cpu().numpy(), rows) and np.array_equal(s2.cpu().numpy().view(np.uint32), sc.view(np.uint32))
            hits = sum(int(x in set(e.neighbors(int(v))[0].tolist())) for v, row in zip(V, nb[:34]) for x in row)
            print("most_similar %s: %.3f of the top-5 neighbours are graph neighbours (not asserted); worst score error / eps %.4f"
                  % (metric, hits / (34 * 5), WORST["most_similar, " + metric]))
        nb10, _ = e.most_similar(emb_in, [1, 34])                          # the defaults: k = 10, cosine; a list is uploaded
        assert tuple(nb10.shape) == (2, 10) and 1 not in nb10[0].tolist() and 34 not in nb10[1].tolist()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def raw_topk(e, table, n_rows, qvec, qrow, Q, dim, k, metric, out_rows, out_scores, reserved=0):
    P = pkg()
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())      # noqa: E731
    tp, n = P.TopkParams(dim, k, metric, reserved), C.c_int64(-7)
    torch.cuda.synchronize()
    rc = P.lib().srw_topk_rows(e.h, ptr(table), n_rows, ptr(qvec), ptr(qrow), Q, C.byref(tp), ptr(out_rows), ptr(out_scores), C.byref(n))
    return rc, n.value


def test_topk_refusals_leave_the_outputs_untouched(eng):
    P = pkg()
    n, D, Q, k = 50, 8, 4, 3
    big = torch.full((n * D + Q * D + Q + 4 * Q * k + 64,), 0x40E00000, dtype=torch.int32, device=DEV)      # (7.0f; compared as integers)
    table = big[:n * D].view(torch.float32).view(n, D)
    qvec = big[n * D:n * D + Q * D].view(torch.float32).view(Q, D)
    qrow = big[n * D + Q * D:n * D + Q * D + Q]
    o = n * D + Q * D + Q
    out_rows, out_scores = big[o:o + Q * k], big[o + Q * k:o + 2 * Q * k].view(torch.float32)
    table.copy_(f32(tref.integer_table(n, D, 1))); qvec.copy_(f32(int_queries(Q, D, 2))); qrow.copy_(i32([0, 1, 2, 3]))
    saved = big.clone()
    ok = dict(table=table, n_rows=n, qvec=qvec, qrow=qrow, Q=Q, dim=D, k=k, metric=1, out_rows=out_rows, out_scores=out_scores)
    refused = [
        dict(dim=0), dict(dim=1025), dict(dim=-8), dict(k=0), dict(k=65), dict(k=-1), dict(metric=2), dict(metric=-1), dict(reserved=1),
        dict(n_rows=-1), dict(n_rows=2**31), dict(Q=-1),
        dict(table=None), dict(out_rows=None), dict(out_scores=None), dict(qvec=None, qrow=None),
        dict(table=table.data_ptr() + 2), dict(qvec=qvec.data_ptr() + 1), dict(qrow=qrow.data_ptr() + 2),
        dict(out_rows=out_rows.data_ptr() + 2), dict(out_scores=out_scores.data_ptr() + 3),
        dict(out_scores=out_rows), dict(out_scores=out_rows.data_ptr() + 4 * (Q * k - 1)),      # the outputs over each other
        dict(out_rows=out_scores.data_ptr() + 4 * (Q * k - 1), out_scores=out_scores),
        dict(out_rows=table), dict(out_scores=table.data_ptr() + 4 * (n * D - 1)),              # an output over the table
        dict(out_rows=qvec), dict(out_scores=qvec.data_ptr() + 4 * (Q * D - 1)),                # ... over the vectors
        dict(out_rows=qrow), dict(out_scores=qrow.data_ptr() + 4 * (Q - 1)),                    # ... over the query rows
        dict(out_rows=qrow.data_ptr() - 4 * (Q * k - 1)),                                       # ending inside the query rows
    ]
    for change in refused:
        rc, skipped = raw_topk(eng, **{**ok, **change})
        assert rc == P.ERR_INVALID and skipped == -7, change
        assert torch.equal(big, saved), change
        assert P.lib().srw_last_error(eng.h).decode().startswith("srw_topk_rows"), change
    # ... and what is allowed: nothing to do whatever the pointers are, an empty table, the call the refusals were cut from
    assert raw_topk(eng, **{**ok, "Q": 0, "table": None, "qvec": None, "qrow": None, "out_rows": None, "out_scores": None}) == (P.OK, 0)
    assert torch.equal(big, saved)
    assert raw_topk(eng, **{**ok, "n_rows": 0, "table": None}) == (P.OK, 4)            # by vector with rows 0 .. 3 of no table: all skipped
    assert (out_rows == -1).all() and (out_scores == -np.inf).all()
    assert raw_topk(eng, **{**ok, "n_rows": 0, "table": None, "qrow": None}) == (P.OK, 0)
    assert (out_rows == -1).all() and (out_scores == -np.inf).all()
    assert raw_topk(eng, **ok) == (P.OK, 0)
    ref = tref.topk(table.cpu().numpy(), k, vectors=qvec.cpu().numpy(), rows=[0, 1, 2, 3], metric="dot")
    tref.check_exact(ref, out_rows.view(Q, k).cpu().numpy(), out_scores.view(Q, k).cpu().numpy())
    assert torch.equal(big[:o], saved[:o]) and torch.equal(big[o + 2 * Q * k:], saved[o + 2 * Q * k:])     # nothing but the outputs is written
    with pytest.raises(ValueError, match="metric"):
        eng.topk_rows(table, k, rows=qrow, metric="euclid")
    with pytest.raises(TypeError, match="in device memory"):
        eng.topk_rows(table.cpu(), k, rows=qrow)
    empty = eng.topk_rows(table, k, rows=torch.empty((0,), dtype=torch.int32, device=DEV))
    assert tuple(empty[0].shape) == (0, k) and empty[2] == 0
    # a sharded handle serves as well: the search is the table's business alone
    with P.Engine(device=0, rank=0, world=2) as shard:
        r, s, _ = shard.topk_rows(table, k, vectors=qvec, rows=qrow, metric="dot")
        tref.check_exact(ref, r.cpu().numpy(), s.cpu().numpy())


def test_vertex_rows_refusals():
    P = pkg()
    L = P.lib()
    ids = i32([1, 2, 99, 3])
    out = torch.full((8,), -5, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def raw(e, d_ids, n, d_rows):
        unknown = C.c_int64(-7)
        ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())      # noqa: E731
        return L.srw_vertex_rows(e.h, ptr(d_ids), n, ptr(d_rows), C.byref(unknown)), unknown.value

    with P.Engine(device=0) as e:
        assert raw(e, ids, 4, out)[0] == P.ERR_INVALID and "no graph" in L.srw_last_error(e.h).decode()
        e.load_edgelist(KARATE, directed=False)
        for args in ((None, 4, out), (ids, 4, None), (ids, -1, out), (ids.data_ptr() + 2, 3, out), (ids, 4, out.data_ptr() + 1)):
            assert raw(e, *args) == (P.ERR_INVALID, -7), args
            assert L.srw_last_error(e.h).decode().startswith("srw_vertex_rows")
        e._ck(L.srw_shard_select(e.h, 1))
        assert raw(e, ids, 4, out)[0] == P.ERR_INVALID and "population 1" in L.srw_last_error(e.h).decode()
        e._ck(L.srw_shard_select(e.h, 0))
        assert (out == -5).all()
        assert raw(e, None, 0, None) == (P.OK, 0)
        assert raw(e, ids, 4, out) == (P.OK, 1) and out.cpu().tolist() == [0, 1, -1, 2, -5, -5, -5, -5]
        assert L.srw_vertex_rows(e.h, C.c_void_p(ids.data_ptr()), 4, C.c_void_p(out.data_ptr()), None) == P.OK     # n_unknown may be NULL
    with P.Engine(device=0, rank=0, world=2) as shard:
        assert raw(shard, ids, 4, out)[0] == P.ERR_INVALID and "world == 1" in L.srw_last_error(shard.h).decode()


def test_zz_the_worst_score_error_of_the_file():
    """printed, for DESIGN 7f; every entry was asserted <= 1 where it was measured"""
    cos = max([v for k, v in WORST.items() if "cosine" in k] + [0.0])
    dot = max([v for k, v in WORST.items() if "dot" in k] + [0.0])
    print("worst score error / eps over the file: cosine %.4f, dot %.4f, over %d checks" % (cos, dot, len(WORST)))
    assert max(list(WORST.values()) + [0.0]) <= 1
