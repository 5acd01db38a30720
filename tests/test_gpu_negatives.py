"""srw_skipgram_batch / srw_negative_weights_set / srw_path_vertex_counts / srw_graph_degrees_device and their Engine methods against
the numpy restatement of their specification (tests/negatives_ref.py; its footing: tests/test_negatives_cpu.py): every element of neg
under a weight table and under exclusion, at the smallest shapes at which each piece of the kernels can go wrong; the counts against
np.bincount; the weights' quantisation and the refusals.
Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import negatives_ref as nref
import skipgram_ref as ref
from conftest import KARATE
from helpers import pkg, random_multigraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -77
U32 = 2**32 - 1


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


def rawb(e, paths, lens, C_, K, seed, epoch, excl, md, pos, neg, cap):
    """srw_skipgram_batch itself: (status, *n_windows)"""
    P = pkg()
    bp = P.SkipgramBatchParams(C_, K, seed, epoch, excl, md)
    w = C.c_int64(-5)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
    torch.cuda.synchronize()
    n, stride = (0, 1) if paths is None else (paths.shape[0], paths.shape[1])
    rc = P.lib().srw_skipgram_batch(e.h, ptr(paths), ptr(lens), n, stride, C.byref(bp), ptr(pos), ptr(neg), cap, C.byref(w))
    return rc, w.value


def wnp(q):
    """the tensor set_negative_weights returned -> what the restatement is fed"""
    return None if q is None else q.cpu().numpy().astype(np.uint64)


def check(e, C_, K, q=None, seed=1, epoch=0, exclude=False, max_draws=8, explicit=False, want=None):
    """Engine.skipgram_batch over the last walk against the restatement on the fetched result (want: the restatement's triple when the
    caller has computed it already) -> (neg, redraws, exhausted, pos)"""
    tp, tl = e.paths_tensor()
    paths, lens = tp.cpu().numpy(), tl.cpu().numpy()
    kw = dict(paths=tp, lens=tl) if explicit else {}
    pos, neg = e.skipgram_batch(C_, K, seed=seed, epoch=epoch, exclude_window=exclude, max_draws=max_draws, **kw)
    W = int(ref.counts(lens, C_).sum())
    assert pos.dtype == torch.int32 and tuple(pos.shape) == (W, C_) and neg.dtype == torch.int32 and tuple(neg.shape) == (W, K)
    assert np.array_equal(pos.cpu().numpy(), ref.windows_fast(paths, lens, C_))
    want, redraws, exhausted = want or nref.negatives(lens, C_, K, seed, epoch, e.vertices(), w=wnp(q), paths=paths, exclude=exclude,
                                                      max_draws=max_draws)
    got = neg.cpu().numpy()
    assert np.array_equal(got, want), "neg differs at window %d" % np.nonzero((got != want).any(axis=1))[0][:1]
    return got, redraws, exhausted, pos.cpu().numpy()


# ---- karate, degree weights: odd K, the vector store, the scalar store, an unaligned neg ------------------------------------------------
@pytest.fixture(scope="module")
def karate(eng):
    eng.load_edgelist(KARATE, directed=False)
    eng.walk(fetch=False, walk_length=20, num_walks=2, seed=5, p=0.5, q=2.0)
    q = eng.set_negative_weights(eng.degrees_tensor())
    assert q.dtype == torch.int64 and torch.equal(q, eng.degrees_tensor()) and int(q.sum()) == 156
    yield eng, q
    eng.set_negative_weights(None)


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_karate_degree_weights(karate, C_, K):
    e, q = karate
    neg, _, _, _ = check(e, C_, K, q, seed=3, epoch=K)
    W = neg.shape[0]
    # neg 4 bytes past an aligned address: neither 8 nor 16 bytes aligned, every store goes element by element
    buf = torch.full((W * K + 5,), POISON, dtype=torch.int32, device=DEV)
    pos = torch.empty((W * C_,), dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    assert rawb(e, None, None, C_, K, 3, K, 0, 8, pos, buf[1:], W) == (pkg().OK, W)
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:1 + W * K].reshape(W, K), neg) and got[0] == POISON and (got[1 + W * K:] == POISON).all()


def test_degree_weights_follow_the_degrees(karate):
    e, q = karate
    neg, _, _, _ = check(e, 3, 8, q, seed=9)
    V, deg = e.vertices(), q.cpu().numpy()
    freq = np.array([(neg == v).sum() for v in V]) / neg.size
    assert abs(freq[np.argmax(deg)] - deg.max() / 156) < 0.02 and freq[np.argmax(deg)] > 3 * freq[np.argmin(deg)]


def test_all_the_weight_on_one_vertex(karate):
    e, q = karate
    V = e.vertices()
    try:
        for at in (0, 33):
            w = torch.zeros(34, dtype=torch.int64, device=DEV)
            w[at] = 7
            qq = e.set_negative_weights(w)
            neg, _, _, _ = check(e, 2, 5, qq)
            assert (neg == V[at]).all()
    finally:
        e.set_negative_weights(q)


def test_no_table_and_no_exclusion_is_skipgram_bit_for_bit(karate):
    e, q = karate
    e.set_negative_weights(None)
    try:
        for C_, K in ((3, 3), (10, 8), (1, 4), (22, 1)):
            pos, neg = e.skipgram(C_, K, seed=4, epoch=2)
            bpos, bneg = e.skipgram_batch(C_, K, seed=4, epoch=2)
            assert torch.equal(pos, bpos) and torch.equal(neg, bneg)
            check(e, C_, K, None, seed=4, epoch=2)
        bpos, bneg = e.skipgram_batch(5)
        assert bneg is None and torch.equal(bpos, e.skipgram(5)[0])
    finally:
        e.set_negative_weights(q)


def test_keying_and_set_then_clear(karate):
    e, q = karate
    tp, tl = e.paths_tensor()
    a, b = 11, 40
    pos_s, neg_s = e.skipgram_batch(4, 6, seed=4, paths=tp[a:b], lens=tl[a:b])
    lens = tl[a:b].cpu().numpy()
    want, _, _ = nref.negatives(lens, 4, 6, 4, 0, e.vertices(), w=wnp(q))             # keyed from row 0
    assert np.array_equal(neg_s.cpu().numpy(), want)
    assert np.array_equal(pos_s.cpu().numpy(), ref.windows_loop(tp[a:b].cpu().numpy(), lens, 4))
    _, full = e.skipgram_batch(4, 6, seed=4)
    _, epoch1 = e.skipgram_batch(4, 6, seed=4, epoch=1)
    _, seed5 = e.skipgram_batch(4, 6, seed=5)
    assert torch.equal(full[:(b - a) * 19], neg_s) and not torch.equal(full[a * 19:b * 19], neg_s)
    assert not torch.equal(epoch1, full) and not torch.equal(seed5, full)
    _, uniform = e.skipgram(4, 6, seed=4)
    assert not torch.equal(full, uniform)
    assert e.set_negative_weights(None) is None
    assert torch.equal(e.skipgram_batch(4, 6, seed=4)[1], uniform)
    assert torch.equal(e.set_negative_weights(q), q)
    assert torch.equal(e.skipgram_batch(4, 6, seed=4)[1], full)


def test_walk_skipgram_batch_is_walk_then_batch(karate):
    e, q = karate
    wkw = dict(walk_length=20, num_walks=2, seed=5, p=0.5, q=2.0)
    src = torch.tensor([3, 34, 3, 1], dtype=torch.int32, device=DEV)
    pos, neg = e.walk_skipgram_batch(src, 5, 4, sg_seed=6, epoch=3, exclude_window=True, max_draws=4, **wkw)
    paths, lens, _ = e.walk(sources=src.cpu().numpy(), **wkw)
    want, _, _ = nref.negatives(lens, 5, 4, 6, 3, e.vertices(), w=wnp(q), paths=paths, exclude=True, max_draws=4)
    assert np.array_equal(pos.cpu().numpy(), ref.windows_loop(paths, lens, 5)) and np.array_equal(neg.cpu().numpy(), want)
    e.walk(fetch=False, **wkw)                                                  # (the module's karate walk again)


# ---- exclusion -------------------------------------------------------------------------------------------------------------------
def test_exclusion_on_karate(karate):
    e, q = karate
    tp, tl = e.paths_tensor()
    paths, lens = tp.cpu().numpy(), tl.cpu().numpy()
    V = e.vertices()
    for w in (q, None):
        e.set_negative_weights(w)
        # the restatement alone first: something is redrawn, nothing runs out of attempts ((5/34)^16 per entry; a failure here asks
        # for another seed, not another cap)
        want = nref.negatives(lens, 5, 8, 2, 1, V, w=wnp(w), paths=paths, exclude=True, max_draws=16)
        assert want[1] > 0 and want[2] == 0
        neg, _, _, pos = check(e, 5, 8, w, seed=2, epoch=1, exclude=True, max_draws=16, want=want)
        assert not (neg[:, :, None] == pos[:, None, :]).any()
        plain, _, _, _ = check(e, 5, 8, w, seed=2, epoch=1)
        assert (plain[:, :, None] == pos[:, None, :]).any() and (plain != neg).any()
        assert ((plain != neg).any(axis=1) <= (plain[:, :, None] == pos[:, None, :]).any(axis=(1, 2))).all()
    e.set_negative_weights(q)
    _, _, exhausted, _ = check(e, 5, 4, q, seed=2, epoch=1, exclude=True, max_draws=2)   # a cap that binds: some last attempts stand
    assert exhausted > 0
    # max_draws outside 1 .. 16 with exclusion on; ignored with exclusion off
    P = pkg()
    for md in (0, 17, -1):
        assert rawb(e, None, None, 5, 0, 1, 0, 1, md, None, None, 0)[0] == P.ERR_INVALID
        assert "max_draws" in P.lib().srw_last_error(e.h).decode()
        assert rawb(e, None, None, 5, 0, 1, 0, 0, md, None, None, 0) == (P.OK, 68 * 18)
        with pytest.raises(P.SrwError):
            e.skipgram_batch(5, 2, exclude_window=True, max_draws=md)


@pytest.mark.parametrize("md", [1, 2, 16])
def test_every_attempt_rejected_the_last_one_stands(md):
    with pkg().Engine(device=0) as e:
        e.load_coo(np.array([4], dtype=np.int32), np.array([9], dtype=np.int32))
        e.walk(fetch=False, walk_length=5, num_walks=1, seed=1)
        tp, tl = e.paths_tensor()
        assert tuple(tp.shape) == (2, 7) and bool((tl == 7).all())
        for w in (None, torch.tensor([3, 1], dtype=torch.int32, device=DEV)):
            q = e.set_negative_weights(w)
            neg, redraws, exhausted, _ = check(e, 2, 3, q, seed=8, exclude=True, max_draws=md)
            assert exhausted == neg.size == 36 and redraws == 36 * (md - 1)
            r, j = ref.window_keys(tl.cpu().numpy(), 2)
            cdf = None if q is None else nref.cdf_of(wnp(q))
            for k in range(3):
                assert np.array_equal(neg[:, k], nref.draw(r, j, k, md - 1, 8, 0, e.vertices(), cdf))


def test_rows_beyond_the_lds_staging_with_exclusion(karate):
    e, q = karate
    e.walk(fetch=False, sources=[1, 34], walk_length=2047, num_walks=1, seed=8)
    assert tuple(e.paths_tensor()[0].shape) == (2, 2049)
    _, redraws, _, _ = check(e, 3, 2, q, seed=5, exclude=True, max_draws=8)
    assert redraws > 0
    check(e, 3, 2, q, seed=5)
    e.set_negative_weights(None)
    check(e, 3, 4, None, seed=5, exclude=True, max_draws=8)
    e.set_negative_weights(q)
    e.walk(fetch=False, walk_length=20, num_walks=2, seed=5, p=0.5, q=2.0)      # (the module's karate walk again)


# ---- the group widths of the row-ownership rule -----------------------------------------------------------------------------------------
def test_group_widths_4_16_64():
    """k_skipgram_fill's rule, (stride - C + 1) * C ints of a full row: up to 16 -> 4 lanes, up to 128 -> 16, else a wave.  Stride 8:
    C = 1 gives 8 (4 lanes), C = 3 gives 18 (16 lanes); stride 42, C = 10 gives 330 (a wave).  Ragged rows: a directed graph."""
    with pkg().Engine(device=0) as e:
        e.generate_rmat(10, directed=True)
        q = e.set_negative_weights(e.degrees_tensor() + 1)
        for wl, C_ in ((6, 1), (6, 3), (40, 10)):
            e.walk(fetch=False, walk_length=wl, num_walks=2, seed=4)
            tp, tl = e.paths_tensor()
            assert tp.shape[1] == wl + 2 and int(tl.min()) == 1 and int(tl.max()) >= C_
            for K in (3, 4):
                check(e, C_, K, q, seed=K)
                check(e, C_, K, q, seed=K, exclude=True, max_draws=3)
        e.set_negative_weights(None)
        e.walk(fetch=False, walk_length=6, num_walks=1, seed=4)
        check(e, 3, 5, None, exclude=True, max_draws=3)


# ---- tables that strain the guide and the search ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rmat12():
    with pkg().Engine(device=0) as e:
        e.generate_rmat(12)
        e.walk(fetch=False, walk_length=10, num_walks=1, seed=2)
        yield e


def test_zero_weights_first_last_and_in_a_run(rmat12):
    e = rmat12
    V = e.vertices()
    nV = len(V)
    w = e.degrees_tensor().clone()
    assert nV > 2000 and int(w.min()) > 0
    mid = nV // 2
    w[0] = 0; w[-1] = 0; w[mid:mid + 100] = 0
    q = e.set_negative_weights(w)
    assert torch.equal(q, w)
    neg, _, _, _ = check(e, 3, 6, q, seed=7)
    dead = set(V[[0, nV - 1]].tolist()) | set(V[mid:mid + 100].tolist())
    seen = set(np.unique(neg).tolist())
    assert not (seen & dead) and len(seen) > nV // 2


def test_one_guide_bucket_holds_almost_every_vertex(rmat12):
    e = rmat12
    nV = e.num_vertices
    w = torch.ones(nV, dtype=torch.int64, device=DEV)
    w[0] = U32
    q = e.set_negative_weights(w)
    neg, _, _, _ = check(e, 3, 6, q, seed=1)
    V = e.vertices()
    assert (neg == V[0]).mean() > 0.99
    # ... and the mirror image: the huge value last, so that the first bucket is the long one
    w = torch.ones(nV, dtype=torch.int64, device=DEV)
    w[-1] = U32
    check(e, 2, 4, e.set_negative_weights(w), seed=1)
    # a table whose tail weighs 2^-32 of the whole: a few draws in 8e5 land there
    w = torch.full((nV,), U32, dtype=torch.int64, device=DEV)
    w[nV // 3:] = 1
    check(e, 1, 8, e.set_negative_weights(w), seed=3)


def test_full_weights_on_rmat17_exceed_2_48():
    with pkg().Engine(device=0) as e:
        e.generate_rmat(17)
        nV = e.num_vertices
        assert 8e4 < nV < 1.2e5
        q = e.set_negative_weights(torch.full((nV,), U32, dtype=torch.int64, device=DEV))
        assert int(q.sum()) > 2**48 and bool((q == U32).all())
        e.walk(fetch=False, sources=np.arange(0, 4096, dtype=np.int32)[np.isin(np.arange(4096), e.vertices())], walk_length=10, seed=3)
        neg, _, _, _ = check(e, 4, 6, q, seed=2)
        # an even table: the draw is the uniform index map of the 64-bit word
        assert len(np.unique(neg)) > 0.5 * min(neg.size, nV)
        check(e, 4, 6, q, seed=2, exclude=True, max_draws=2)


def test_a_single_vertex():
    with pkg().Engine(device=0) as e:
        e.load_coo(np.array([7], dtype=np.int32), np.array([7], dtype=np.int32))
        assert e.num_vertices == 1
        e.walk(fetch=False, walk_length=4, num_walks=3, seed=1)
        for w in (None, torch.tensor([5], dtype=torch.int64, device=DEV), torch.tensor([U32], dtype=torch.int64, device=DEV)):
            q = e.set_negative_weights(w)
            neg, _, _, _ = check(e, 2, 3, q)
            assert (neg == 7).all() and neg.shape == (15, 3)
            neg, _, exhausted, _ = check(e, 2, 3, q, exclude=True, max_draws=3)
            assert (neg == 7).all() and exhausted == 45


@pytest.mark.parametrize("compact", [True, False])
def test_a_sparse_id_space_gives_input_ids(compact):
    k = 40
    rng = np.random.default_rng(21)
    s, d, _ = random_multigraph(rng, 45, 300, False, id_lo=2_000_000_000 - k)
    with pkg().Engine(device=0, compact_ids=compact) as e:
        e.load_coo(s, d, directed=True)
        e.walk(fetch=False, walk_length=9, num_walks=2, seed=2)
        V = e.vertices()
        deg = e.degrees_tensor()
        assert deg.cpu().tolist() == [len(e.neighbors(int(v))[0]) for v in V]
        q = e.set_negative_weights(deg)                                         # destination-only vertices: weight 0
        neg, _, _, pos = check(e, 3, 5, q, seed=7)
        assert V.min() >= 2_000_000_000 - k and neg.min() >= 2_000_000_000 - k
        assert set(np.unique(neg).tolist()) <= set(V[deg.cpu().numpy() > 0].tolist())
        neg, _, _, _ = check(e, 3, 5, q, seed=7, exclude=True, max_draws=6)
        paths, lens = [x.cpu().numpy() for x in e.paths_tensor()]
        cnt = e.visit_counts().cpu().numpy()
        assert e.last_unknown_ids == 0
        assert np.array_equal(cnt, [(paths[np.arange(paths.shape[1])[None, :] < lens[:, None]] == v).sum() for v in V])


# ---- counts and degrees --------------------------------------------------------------------------------------------------------------
def bincount_ref(paths, lens, V):
    tok = paths[np.arange(paths.shape[1])[None, :] < lens[:, None]].astype(np.int64)
    lo = int(V.min())
    bc = np.bincount(tok - lo, minlength=int(V.max()) - lo + 1)
    return bc[V.astype(np.int64) - lo]


def test_visit_counts_on_karate_and_degrees(karate):
    e, _ = karate
    tp, tl = e.paths_tensor()
    V = e.vertices()
    cnt = e.visit_counts()
    assert cnt.dtype == torch.int64 and cnt.is_cuda and tuple(cnt.shape) == (34,)
    want = bincount_ref(tp.cpu().numpy(), tl.cpu().numpy(), V)
    assert np.array_equal(cnt.cpu().numpy(), want) and int(cnt.sum()) == 68 * 22 and e.last_unknown_ids == 0
    assert torch.equal(e.visit_counts(paths=tp, lens=tl), cnt)
    assert np.array_equal(e.visit_counts(paths=tp[5:9], lens=tl[5:9]).cpu().numpy(), bincount_ref(tp[5:9].cpu().numpy(), tl[5:9].cpu().numpy(), V))
    deg = e.degrees_tensor()
    assert deg.dtype == torch.int64 and deg.cpu().tolist() == [len(e.neighbors(int(v))[0]) for v in V]
    # a caller's array with ids that are no vertices (0, 35, a huge one, a negative one) and lens beyond the stride
    own = torch.tensor([[1, 0, 34, 35], [2_000_000_000, 2, 2, -5], [3, 3, 3, 3]], dtype=torch.int32, device=DEV)
    ln = torch.tensor([4, 4, 9], dtype=torch.int32, device=DEV)
    buf = torch.full((34,), POISON, dtype=torch.int64, device=DEV)
    unknown = C.c_int64(-1)
    L = pkg().lib()
    for _ in range(2):                                                         # overwritten, not accumulated
        torch.cuda.synchronize()
        e._ck(L.srw_path_vertex_counts(e.h, C.c_void_p(own.data_ptr()), C.c_void_p(ln.data_ptr()), 3, 4, C.c_void_p(buf.data_ptr()), C.byref(unknown)))
        got = buf.cpu().numpy()
        assert unknown.value == 4 and got.sum() == 8 and (got[0], got[1], got[2], got[33]) == (1, 2, 4, 1)
    assert np.array_equal(e.visit_counts(paths=own, lens=ln).cpu().numpy(), got) and e.last_unknown_ids == 4
    assert int(e.visit_counts(paths=own[:0], lens=ln[:0]).sum()) == 0
    P = pkg()
    assert L.srw_path_vertex_counts(e.h, None, None, 0, 0, None, C.byref(unknown)) == P.ERR_INVALID          # d_counts == NULL
    assert L.srw_path_vertex_counts(e.h, C.c_void_p(own.data_ptr()), None, 3, 4, C.c_void_p(buf.data_ptr()), C.byref(unknown)) == P.ERR_INVALID
    assert L.srw_graph_degrees_device(e.h, None) == P.ERR_INVALID


def test_visit_counts_on_a_directed_graph_with_dead_ends():
    with pkg().Engine(device=0) as e:
        e.generate_rmat(10, directed=True)
        e.walk(fetch=False, walk_length=12, num_walks=3, seed=6)
        tp, tl = e.paths_tensor()
        paths, lens = tp.cpu().numpy(), tl.cpu().numpy()
        assert paths.shape[1] == 14 and lens.min() == 1 and lens.max() > 1
        V = e.vertices()
        assert np.array_equal(e.visit_counts().cpu().numpy(), bincount_ref(paths, lens, V)) and e.last_unknown_ids == 0
        deg = e.degrees_tensor().cpu().numpy()
        assert deg.tolist() == [len(e.neighbors(int(v))[0]) for v in V] and (deg == 0).any() and deg.sum() == e.num_entries
        with pytest.raises(pkg().SrwError):
            e.skipgram_batch(15)                                                # context > stride, as skipgram


def test_visit_counts_on_a_star_the_single_hot_counter():
    leaves = 4096
    with pkg().Engine(device=0) as e:
        e.load_coo(np.zeros(leaves, dtype=np.int32), np.arange(1, leaves + 1, dtype=np.int32))
        e.walk(fetch=False, walk_length=20, num_walks=1, seed=3)
        tp, tl = e.paths_tensor()
        paths, lens = tp.cpu().numpy(), tl.cpu().numpy()
        cnt = e.visit_counts().cpu().numpy()
        assert np.array_equal(cnt, bincount_ref(paths, lens, e.vertices()))
        assert cnt.sum() == (leaves + 1) * 22 and cnt[0] == (leaves + 1) * 11   # every other token is the hub


# ---- weights ----------------------------------------------------------------------------------------------------------------------
def test_float_weights_are_quantised_in_torch_and_fed_as_returned(karate):
    e, q0 = karate
    try:
        w = e.visit_counts().double().pow(0.75)
        w[3] = 0.0
        w[4] = 1e-30                                                            # positive and far below max / 2^32
        q = e.set_negative_weights(w)
        assert q.dtype == torch.int64 and int(q.max()) == U32 and int(q[3]) == 0 and int(q[4]) == 1
        assert bool((q[w > 0] >= 1).all()) and bool((q[w == 0] == 0).all())
        neg, _, _, _ = check(e, 3, 5, q, seed=6)                                # the restatement is fed q as returned
        assert e.vertices()[3] not in neg
        q32 = e.set_negative_weights(w.float())
        assert bool((q32[w > 0] >= 1).all()) and int(q32[3]) == 0
        check(e, 3, 5, q32, seed=6)
        for dt in (torch.int32, torch.int64, torch.uint8, torch.int16):
            wi = (torch.arange(34, device=DEV) % 5).to(dt)
            qi = e.set_negative_weights(wi)
            assert qi.dtype == torch.int64 and torch.equal(qi, wi.to(torch.int64))
        big = torch.full((34,), U32, dtype=torch.int64, device=DEV)
        big[::2] = 2**31
        assert torch.equal(e.set_negative_weights(big), big)
        check(e, 3, 2, big, seed=6)
    finally:
        e.set_negative_weights(q0)


def test_weight_errors_leave_the_table_in_force(karate):
    P = pkg()
    e, q = karate
    _, before = e.skipgram_batch(3, 4, seed=2)
    ones = torch.ones(34, dtype=torch.int64, device=DEV)
    for w in (ones[:33], torch.ones(35, dtype=torch.int64, device=DEV), ones[:0], ones * 0, torch.zeros(34, device=DEV)):
        with pytest.raises(P.SrwError) as ei:
            e.set_negative_weights(w)
        assert ei.value.code == P.ERR_INVALID
    bad = ones.clone().double()
    for val, exc in ((-1.0, ValueError), (float("nan"), ValueError), (float("inf"), ValueError)):
        bad[7] = val
        with pytest.raises(exc):
            e.set_negative_weights(bad)
    for val in (-1, 2**32):
        wi = ones.clone()
        wi[7] = val
        with pytest.raises(ValueError):
            e.set_negative_weights(wi)
    with pytest.raises(TypeError, match="in device memory"):
        e.set_negative_weights(torch.ones(34))
    assert torch.equal(e.skipgram_batch(3, 4, seed=2)[1], before)               # the degree table is still in force
    with P.Engine(device=0, rank=0, world=2) as shard:
        with pytest.raises(P.SrwError) as ei:
            shard.set_negative_weights(ones)
        assert ei.value.code == P.ERR_INVALID and "world == 1" in str(ei.value)
        for call in (shard.degrees_tensor, shard.visit_counts, lambda: shard.skipgram_batch(2)):
            with pytest.raises(P.SrwError):
                call()
    with P.Engine(device=0) as fresh:
        with pytest.raises(P.SrwError):
            fresh.set_negative_weights(ones)                                    # no graph loaded
        assert fresh.set_negative_weights(None) is None
        fresh._ck(P.lib().srw_shard_select(fresh.h, 1))
        with pytest.raises(P.SrwError, match="population 1"):
            fresh.set_negative_weights(None)
        fresh._ck(P.lib().srw_shard_select(fresh.h, 0))


def test_a_reload_drops_the_table():
    with pkg().Engine(device=0) as e:
        e.load_edgelist(KARATE, directed=False)
        e.walk(fetch=False, walk_length=10, num_walks=1, seed=1)
        _, uniform = e.skipgram_batch(3, 4)
        e.set_negative_weights(e.degrees_tensor())
        _, weighted = e.skipgram_batch(3, 4)
        assert not torch.equal(weighted, uniform)
        e.load_edgelist(KARATE, directed=False)
        e.walk(fetch=False, walk_length=10, num_walks=1, seed=1)
        assert torch.equal(e.skipgram_batch(3, 4)[1], uniform) and torch.equal(e.skipgram(3, 4)[1], uniform)
