"""srw_skipgram_windows / Engine.skipgram / Engine.walk_skipgram against the numpy restatement of their specification
(tests/skipgram_ref.py, pinned to the oracle's Philox by tests/test_skipgram_cpu.py): every element of pos and neg, on ragged rows of
every length, rows longer than one pass of a wave, stretches that start on every residue mod 16 bytes, a scan across blocks, offsets
beyond 2^31 elements, a sparse id space; the keying of the negatives; capacity and edge cases.
Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import skipgram_ref as ref
from conftest import KARATE
from helpers import pkg, random_multigraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -77


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


def raw(e, paths, lens, C_, K, seed, epoch, pos, neg, cap):
    """srw_skipgram_windows itself: (status, *n_windows)"""
    P = pkg()
    sp = P.SkipgramParams(C_, K, seed, epoch)
    w = C.c_int64(-5)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
    torch.cuda.synchronize()
    n, stride = (0, 1) if paths is None else (paths.shape[0], paths.shape[1])
    rc = P.lib().srw_skipgram_windows(e.h, ptr(paths), ptr(lens), n, stride, C.byref(sp), ptr(pos), ptr(neg), cap, C.byref(w))
    return rc, w.value


def check(e, C_, K, seed=1, epoch=0, fast=False, explicit=False):
    """Engine.skipgram over the last walk against the restatement on the fetched result -> (pos, neg, paths, lens) as numpy"""
    tp, tl = e.paths_tensor()
    paths, lens = tp.cpu().numpy(), tl.cpu().numpy()
    kw = dict(paths=tp, lens=tl) if explicit else {}
    pos, neg = e.skipgram(C_, K, seed=seed, epoch=epoch, **kw)
    W = int(ref.counts(lens, C_).sum())
    assert pos.dtype == torch.int32 and pos.is_cuda and tuple(pos.shape) == (W, C_)
    want = (ref.windows_fast if fast else ref.windows_loop)(paths, lens, C_)
    got = pos.cpu().numpy()
    assert np.array_equal(got, want), "pos differs at window %d" % np.nonzero((got != want).any(axis=1))[0][:1]
    if K == 0:
        assert neg is None
        return got, None, paths, lens
    assert neg.dtype == torch.int32 and neg.is_cuda and tuple(neg.shape) == (W, K)
    nwant = ref.negatives(lens, C_, K, seed, epoch, e.vertices())
    ngot = neg.cpu().numpy()
    assert np.array_equal(ngot, nwant), "neg differs at window %d" % np.nonzero((ngot != nwant).any(axis=1))[0][:1]
    return got, ngot, paths, lens


# ---- ragged rows, every length ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(eng):
    """0 -> 1 -> ... -> 19, directed: a walker from v has lens = min(12, 20 - v) whatever it draws"""
    eng.load_coo(np.arange(19, dtype=np.int32), np.arange(1, 20, dtype=np.int32), directed=True)
    eng.walk(fetch=False, walk_length=10, num_walks=2, seed=3)
    tl = eng.paths_tensor()[1].cpu().numpy()
    assert np.array_equal(tl, np.tile(np.minimum(12, 20 - np.arange(20)), 2)) and set(tl.tolist()) == set(range(1, 13))
    return eng


@pytest.mark.parametrize("C_", [1, 2, 5, 12])
def test_ragged_rows_of_every_length(chain, C_):
    e = chain
    tp, tl = e.paths_tensor()
    assert tuple(tp.shape) == (40, 12)
    lens = tl.cpu().numpy()
    W = int(np.maximum(0, lens.astype(np.int64) - C_ + 1).sum())
    for K in (0, 1, 4, 5):
        pos, _, _, _ = check(e, C_, K, seed=11, epoch=K)
        assert pos.shape[0] == W and (pos >= 0).all()
        # count only: the same W, and nothing is written (a poisoned neg buffer rides along; d_pos == NULL is what asks for the count)
        poison = torch.full((max(W * max(K, 1), 1),), POISON, dtype=torch.int32, device=DEV)
        rc, w = raw(e, None, None, C_, K, 11, K, None, poison, 0)
        assert (rc, w) == (pkg().OK, W)
        assert bool((poison == POISON).all())
    if C_ == 12:
        assert W == 2 * 9                                      # only the full rows, one window each
    if C_ == 5:
        c = ref.counts(lens, 5)
        assert (c[:20] == 0).any() and c[0] > 0 and c[20] > 0  # rows with no window between rows with some


# ---- no dead ends: rows longer than a wave's pass, stretches on every residue mod 16 bytes ---------------------------------------------
@pytest.fixture(scope="module")
def karate_walk(eng, chain):
    eng.load_edgelist(KARATE, directed=False)
    eng.walk(fetch=False, walk_length=80, num_walks=3, seed=5, p=0.5, q=2.0)
    return eng


def test_no_dead_ends(karate_walk):
    e = karate_walk
    pos, neg, paths, lens = check(e, 10, 8, seed=2, epoch=1)
    assert paths.shape == (102, 82) and (lens == 82).all() and pos.shape[0] == 102 * 73
    pos2, neg2, _, _ = check(e, 10, 8, seed=2, epoch=1, explicit=True)          # the same result through paths= / lens=
    assert np.array_equal(pos, pos2) and np.array_equal(neg, neg2)


@pytest.mark.parametrize("C_,K", [(3, 0), (7, 3), (82, 4), (81, 2)])
def test_unaligned_stretches(karate_walk, C_, K):
    """80 * 3, 76 * 7, 1 * 82, 2 * 81 output ints per row, written to destinations at 0, 4, 8 and 12 bytes past a 16-byte boundary:
    head and tail of the vector stores on every residue.  C = stride: one window per row."""
    pos, _, _, _ = check(karate_walk, C_, K)
    # a full row of stride 82 holds an even number of output ints whatever C is: the odd residues come from a destination that is
    # itself off the 16-byte boundary (and from the ragged rows of the chain and RMAT cases)
    e = karate_walk
    W = pos.shape[0]
    for shift in (1, 2, 3):
        buf = torch.full((W * C_ + 8,), POISON, dtype=torch.int32, device=DEV)
        rc, w = raw(e, None, None, C_, 0, 1, 0, buf[shift:], None, W)
        assert (rc, w) == (pkg().OK, W)
        got = buf.cpu().numpy()
        assert np.array_equal(got[shift:shift + W * C_].reshape(W, C_), pos), shift
        assert (got[:shift] == POISON).all() and (got[shift + W * C_:] == POISON).all(), shift


def test_rows_beyond_the_lds_staging(eng, karate_walk):
    """stride 2102: the kernel reads such rows from global memory instead of staging them"""
    eng.walk(fetch=False, walk_length=2100, num_walks=1, seed=8)
    check(eng, 5, 4, fast=True)
    check(eng, 2102, 1, fast=True)
    eng.walk(fetch=False, walk_length=80, num_walks=3, seed=5, p=0.5, q=2.0)    # (the module's karate walk again)


# ---- the scan across blocks -------------------------------------------------------------------------------------------------------
def test_ragged_rows_across_many_blocks():
    with pkg().Engine(device=0) as e:
        e.generate_rmat(14, directed=True)
        e.walk(fetch=False, walk_length=6, num_walks=5, seed=4)
        pos, neg, paths, lens = check(e, 3, 4, seed=9, epoch=2, fast=True)
        assert paths.shape[0] > 50000 and paths.shape[1] == 8 and lens.min() == 1 and lens.max() == 8
        assert set(np.unique(neg).tolist()) <= set(e.vertices().tolist())
        check(e, 1, 2, fast=True)                                               # every entry its own window
        check(e, 8, 0, fast=True)


# ---- offsets beyond 2^31 elements ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_walks", [10, 14])
def test_offsets_beyond_2_31_elements(num_walks):
    """RMAT-17, undirected, walk_length 80, C = 41: 42 windows of 41 ints per row.  90 127 of the 131 072 ids are present in the default
    graph, so 10 walks give 1.55e9 ints — below 2^31, that case proves nothing and skips — and 14 walks give 2.17e9."""
    Cw = 41
    with pkg().Engine(device=0) as e:
        e.generate_rmat(17)
        n = e.num_vertices * num_walks
        if n * 42 * Cw <= 2**31:
            pytest.skip("W * C = %d <= 2^31" % (n * 42 * Cw))
        st = e.walk(fetch=False, walk_length=80, num_walks=num_walks, seed=6)
        assert st["dead_ends"] == 0 and st["n_walkers"] == n
        pos, neg = e.skipgram(Cw)
        tp, tl = e.paths_tensor()
        assert neg is None and tuple(pos.shape) == (n * 42, Cw) and pos.numel() > 2**31 and bool((tl == 82).all())
        rows = 2**28 // (42 * Cw)
        for r0 in range(0, n, rows):
            r1 = min(n, r0 + rows)
            assert torch.equal(pos[r0 * 42:r1 * 42], tp[r0:r1].unfold(1, Cw, 1).reshape(-1, Cw)), (r0, r1)
        del pos
        pos, neg = e.skipgram(80, 4, seed=3, epoch=5)                           # three windows per row
        lens = tl.cpu().numpy()
        assert tuple(pos.shape) == (n * 3, 80) and tuple(neg.shape) == (n * 3, 4)
        assert torch.equal(pos, tp.unfold(1, 80, 1).reshape(-1, 80))
        assert np.array_equal(neg.cpu().numpy(), ref.negatives(lens, 80, 4, 3, 5, e.vertices()))


# ---- keying ---------------------------------------------------------------------------------------------------------------------
def test_negatives_are_keyed_by_row_window_and_k(karate_walk):
    e = karate_walk
    tp, tl = e.paths_tensor()
    V = e.vertices()
    _, full = e.skipgram(10, 6, seed=4, epoch=0)
    a, b = 17, 60
    pos_s, neg_s = e.skipgram(10, 6, seed=4, epoch=0, paths=tp[a:b], lens=tl[a:b])
    # a call over rows [a, b): the key is the row index within the call — the negatives of the first b - a rows of the whole result
    assert torch.equal(neg_s, full[:(b - a) * 73])
    assert not torch.equal(neg_s, full[a * 73:b * 73])
    assert np.array_equal(pos_s.cpu().numpy(), ref.windows_loop(tp[a:b].cpu().numpy(), tl[a:b].cpu().numpy(), 10))
    assert np.array_equal(neg_s.cpu().numpy(), ref.negatives(tl[a:b].cpu().numpy(), 10, 6, 4, 0, V))
    _, again = e.skipgram(10, 6, seed=4, epoch=0)
    _, epoch1 = e.skipgram(10, 6, seed=4, epoch=1)
    _, seed5 = e.skipgram(10, 6, seed=5, epoch=0)
    assert torch.equal(again, full)
    assert not torch.equal(epoch1, full) and not torch.equal(seed5, full) and not torch.equal(seed5, epoch1)
    assert set(np.unique(full.cpu().numpy()).tolist()) <= set(V.tolist())
    assert len(np.unique(full.cpu().numpy())) == 34                             # 44 676 uniform draws over 34 vertices: all occur


@pytest.mark.parametrize("compact", [True, False])
def test_a_sparse_id_space_gives_input_ids(compact):
    k = 40
    rng = np.random.default_rng(21)
    s, d, _ = random_multigraph(rng, 45, 300, False, id_lo=2_000_000_000 - k)
    with pkg().Engine(device=0, compact_ids=compact) as e:
        e.load_coo(s, d, directed=True)
        e.walk(fetch=False, walk_length=9, num_walks=2, seed=2)
        pos, neg, paths, lens = check(e, 3, 5, seed=7)
        V = e.vertices()
        assert V.min() >= 2_000_000_000 - k and pos.min() >= 2_000_000_000 - k
        assert set(np.unique(neg).tolist()) <= set(V.tolist())


# ---- capacity and edge cases ------------------------------------------------------------------------------------------------------------
def test_capacity_and_argument_errors(karate_walk):
    P = pkg()
    e = karate_walk
    tp, tl = e.paths_tensor()
    W = 102 * 73
    pos = torch.full((W * 10,), POISON, dtype=torch.int32, device=DEV)
    neg = torch.full((W * 4,), POISON, dtype=torch.int32, device=DEV)
    rc, w = raw(e, None, None, 10, 4, 1, 0, pos, neg, W - 1)
    assert (rc, w) == (P.ERR_INVALID, W)
    msg = P.lib().srw_last_error(e.h).decode()
    assert str(W) in msg and str(W - 1) in msg, msg
    assert bool((pos == POISON).all()) and bool((neg == POISON).all())
    assert raw(e, None, None, 10, 4, 1, 0, pos, neg, W) == (P.OK, W)            # ... and it fits exactly
    assert not bool((pos == POISON).any())
    # argument errors: SRW_ERR_INVALID, nothing written
    pos.fill_(POISON); neg.fill_(POISON)
    L = P.lib()
    sp, wv = P.SkipgramParams(10, 4, 1, 0), C.c_int64(0)
    vp = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    assert L.srw_skipgram_windows(e.h, None, None, 0, 0, None, vp(pos), vp(neg), W, C.byref(wv)) == P.ERR_INVALID      # sp == NULL
    assert L.srw_skipgram_windows(e.h, None, None, 0, 0, C.byref(sp), vp(pos), vp(neg), W, None) == P.ERR_INVALID      # n_windows == NULL
    for C_, K, paths, lens, p_, n_ in ((0, 0, None, None, pos, neg), (83, 0, None, None, pos, neg), (-1, 0, None, None, pos, neg),
                                       (10, -1, None, None, pos, neg), (10, 4, None, None, pos, None),
                                       (10, 0, tp, None, pos, None)):
        rc, _ = raw(e, paths, lens, C_, K, 1, 0, p_, n_, W)
        assert rc == P.ERR_INVALID, (C_, K)
    sp = P.SkipgramParams(10, 0, 1, 0)
    assert L.srw_skipgram_windows(e.h, None, vp(tl), 102, 82, C.byref(sp), vp(pos), None, W, C.byref(wv)) == P.ERR_INVALID    # lens alone
    # n == 0 with a pointer given: a valid, empty result whatever stride and the other pointer are
    for pp, pl, stride in ((vp(tp), vp(tl), 82), (vp(tp), vp(tl), 0), (vp(tp), None, 0), (None, vp(tl), 5)):
        wv.value = -3
        assert L.srw_skipgram_windows(e.h, pp, pl, 0, stride, C.byref(sp), vp(pos), None, W, C.byref(wv)) == P.OK and wv.value == 0
    assert L.srw_skipgram_windows(e.h, vp(tp), vp(tl), -1, 82, C.byref(sp), vp(pos), None, W, C.byref(wv)) == P.ERR_INVALID   # n < 0
    assert L.srw_skipgram_windows(e.h, vp(tp), vp(tl), 102, 9, C.byref(sp), vp(pos), None, W, C.byref(wv)) == P.ERR_INVALID   # context > stride
    torch.cuda.synchronize()
    assert bool((pos == POISON).all()) and bool((neg == POISON).all())
    with pytest.raises(P.SrwError):
        e.skipgram(83)
    assert raw(e, None, None, 10, 0, 1, 0, None, None, 0) == (P.OK, W)
    # population 1 selected
    with P.Engine(device=0) as two:
        two._ck(L.srw_shard_select(two.h, 1))
        assert raw(two, None, None, 10, 0, 1, 0, None, None, 0)[0] == P.ERR_INVALID
        assert "population 1" in L.srw_last_error(two.h).decode()
        two._ck(L.srw_shard_select(two.h, 0))
        assert raw(two, None, None, 10, 0, 1, 0, None, None, 0)[0] == P.ERR_INVALID
        assert "no walk result" in L.srw_last_error(two.h).decode()


def test_empty_results_and_handles_without_a_result(karate_walk):
    P = pkg()
    e = karate_walk
    e.walk(fetch=False, sources=[], walk_length=80)
    pos, neg = e.skipgram(10, 3)
    assert tuple(pos.shape) == (0, 10) and tuple(neg.shape) == (0, 3) and pos.dtype == torch.int32
    tp, tl = e.paths_tensor()
    pos, neg = e.skipgram(4, paths=tp, lens=tl)                                 # explicit empty tensors
    assert tuple(pos.shape) == (0, 4) and neg is None
    e.walk(fetch=False, walk_length=80, num_walks=3, seed=5, p=0.5, q=2.0)      # (the module's karate walk again)
    with P.Engine(device=0) as fresh:
        with pytest.raises(P.SrwError) as ei:
            fresh.skipgram(2)
        assert ei.value.code == P.ERR_INVALID
        # caller-supplied paths need no graph — unless negatives are asked for
        paths = torch.tensor([[5, 6, 7, -1], [8, -1, -1, -1], [1, 2, 3, 4]], dtype=torch.int32, device=DEV)
        lens = torch.tensor([3, 1, 4], dtype=torch.int32, device=DEV)
        pos, neg = fresh.skipgram(2, paths=paths, lens=lens)
        assert pos.cpu().tolist() == [[5, 6], [6, 7], [1, 2], [2, 3], [3, 4]] and neg is None
        pos, _ = fresh.skipgram(4, paths=paths, lens=lens)
        assert pos.cpu().tolist() == [[1, 2, 3, 4]]
        pos, _ = fresh.skipgram(4, paths=paths[:2], lens=lens[:2])              # W == 0
        assert tuple(pos.shape) == (0, 4)
        with pytest.raises(P.SrwError):
            fresh.skipgram(2, 1, paths=paths, lens=lens)
    with P.Engine(device=0, rank=0, world=2) as shard:
        with pytest.raises(P.SrwError) as ei:
            shard.skipgram(2)
        assert ei.value.code == P.ERR_INVALID


# ---- walk_skipgram ------------------------------------------------------------------------------------------------------------------
def test_walk_skipgram_is_walk_then_skipgram(karate_walk):
    e = karate_walk
    src = torch.tensor([3, 34, 3, 1, 17, 34, 34], dtype=torch.int32, device=DEV)
    wkw = dict(walk_length=20, num_walks=2, seed=12, p=0.25, q=4.0)
    pos, neg = e.walk_skipgram(src, 5, 7, sg_seed=6, epoch=3, **wkw)
    keep_p, keep_n = pos.clone(), neg.clone()
    assert e.sources_len() is None                                              # the list was for that call only
    paths, lens, st = e.walk(sources=src.cpu().numpy(), **wkw)
    assert st["n_walkers"] == 14 and (paths[:, 0] == np.tile(src.cpu().numpy(), 2)).all()
    assert np.array_equal(pos.cpu().numpy(), ref.windows_loop(paths, lens, 5))
    assert np.array_equal(neg.cpu().numpy(), ref.negatives(lens, 5, 7, 6, 3, e.vertices()))
    # the tensors are the caller's: another walk on the handle leaves them alone
    e.walk(fetch=False, walk_length=80, num_walks=3, seed=5, p=0.5, q=2.0)
    e.skipgram(9, 2)
    assert torch.equal(pos, keep_p) and torch.equal(neg, keep_n)
    assert pos.data_ptr() != e.paths_tensor()[0].data_ptr()
