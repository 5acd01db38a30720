"""srw_sgns_step and Engine.sgns_step / sgns_grad / train_sgns against the float64 restatement of the header (tests/sgns_ref.py; its
footing: tests/test_sgns_cpu.py): EVERY element of both new tables and of loss, under the tolerance derived there from the number
formats — u (D + m + 8) max(1, S) (|old| + A) per table element, u (D + T + 8) max(1, S) sum (1 + |f|) per window's loss — at the
smallest shapes at which each piece of the kernel can go wrong.  Each check prints its worst error / tolerance ratio before it asserts.
Run on the MI355X box with `pytest -m gpu`."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sgns_ref as sref
from conftest import KARATE
from helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = sref.LR


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def karate(eng):
    eng.load_edgelist(KARATE, directed=False)
    eng.walk(fetch=False, **sref.KARATE_WALK)
    V = eng.vertices()
    assert V.tolist() == list(range(1, 35))                                # the ids as they are: vmin = 1
    return eng, V


def karate_batch(e, C_, K):
    pos, neg = e.skipgram_batch(C_, K, **sref.KARATE_SG)
    assert pos.shape[0] >= sref.KARATE_W
    return pos[:sref.KARATE_W].contiguous(), None if neg is None else neg[:sref.KARATE_W].contiguous()


def cpu(t):
    return None if t is None else t.cpu().numpy()


def hold(what, got_in, got_out, got_loss, want, old_in, old_out):
    """every element of the two new tables and of loss against the restatement"""
    one = want.new_in is want.new_out
    r_in = sref.worst(cpu(got_in), want.new_in, sref.table_bound(want, "in", old_in))
    r_out = 0.0 if one else sref.worst(cpu(got_out), want.new_out, sref.table_bound(want, "out", old_out))
    r_loss = sref.worst(cpu(got_loss), want.loss, sref.loss_bound(want)) if got_loss is not None else 0.0
    print("%s: worst error / tolerance  in %.4f  out %.4f  loss %.4f  (S = %.3g, m up to %d)"
          % (what, r_in, r_out, r_loss, want.S, max(want.m_in.max(), want.m_out.max())))
    assert np.isfinite(cpu(got_in)).all() and np.isfinite(cpu(got_out)).all()
    assert r_in <= 1 and r_out <= 1 and r_loss <= 1, what


def exact_both_forms(e, V, pos, neg, tin, tout, center, what):
    """the exact step into clones, and into zeros with lr = -1 (sgns_grad); pos / neg are device tensors, the tables numpy"""
    a, b = dev(tin), dev(tout)
    na, nb = a.clone(), b.clone()
    loss, skipped = e.sgns_step(pos, neg, a, b, LR, center=center, into=(na, nb), loss=True)
    want = sref.step(V, cpu(pos), cpu(neg), tin, tout, LR, center, tin, tout)
    assert skipped == want.skipped
    assert torch.equal(a, dev(tin)) and torch.equal(b, dev(tout))          # the old tables are only read
    hold(what + " clones", na, nb, loss, want, tin, tout)
    ga, gb, gloss = e.sgns_grad(pos, neg, a, b, center=center)
    z = np.zeros_like(tin)
    want = sref.step(V, cpu(pos), cpu(neg), tin, tout, -1.0, center, z, np.zeros_like(tin))
    hold(what + " grad", ga, gb, gloss, want, z, z)


# ---- the exact form on karate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", sref.KARATE_DIMS)
@pytest.mark.parametrize("C_,K", sref.KARATE_SHAPES)
def test_exact_form_on_karate(karate, C_, K, D):
    e, V = karate
    pos, neg = karate_batch(e, C_, K)
    tin, tout = sref.tables_for(V.size, D, 7)
    for center in sref.centers(C_):
        exact_both_forms(e, V, pos, neg, tin, tout, center, "karate C %d K %d D %d center %d" % (C_, K, D, center))


# ---- heavy collisions: thousands of terms per element ------------------------------------------------------------------------------
def test_heavy_collisions():
    V, pos, neg = sref.heavy_windows()
    with pkg().Engine(device=0) as e:
        e.load_adjacency(sref.heavy_graph())
        assert np.array_equal(e.vertices(), V)
        for D, center in ((64, 0), (128, 1)):
            tin, tout = sref.tables(sref.HEAVY_NV, D, 3, 0.5, 0.5)
            exact_both_forms(e, V, dev(pos), dev(neg), tin, tout, center, "heavy D %d center %d" % (D, center))
        tin, tout = sref.tables(sref.HEAVY_NV, 64, 4, 0.1, 0.1)
        exact_both_forms(e, V, dev(pos), dev(neg), tin, tout, 0, "heavy +-0.1")


# ---- more windows than waves in flight ------------------------------------------------------------------------------------------------
def test_grid_stride():
    with pkg().Engine(device=0) as e:
        e.generate_rmat(12)
        V = e.vertices()
        rng = np.random.default_rng(12)
        W = 70000
        pos, neg = V[rng.integers(0, V.size, size=(W, 2))], V[rng.integers(0, V.size, size=(W, 1))]
        tin, tout = sref.tables(V.size, 64, 5)
        a, b = dev(tin), dev(tout)
        na, nb = a.clone(), b.clone()
        loss, skipped = e.sgns_step(dev(pos), dev(neg), a, b, LR, into=(na, nb), loss=True)
        want = sref.step(V, pos, neg, tin, tout, LR, 0, tin, tout)
        assert skipped == 0
        hold("rmat-12, 70 000 windows", na, nb, loss, want, tin, tout)


# ---- one table for both roles -------------------------------------------------------------------------------------------------------
def test_one_table_for_both_roles(karate):
    e, V = karate
    pos, neg = karate_batch(e, 3, 2)
    for center in (0, 1):
        neg[0, 0] = pos[0, center]                                         # a negative equal to its own centre
        neg[1, 1] = pos[1, center]
        tab, _ = sref.tables_for(V.size, 128, 9)
        a = dev(tab)
        n = a.clone()
        loss, skipped = e.sgns_step(pos, neg, a, a, LR, center=center, into=(n, n), loss=True)
        want = sref.step(V, cpu(pos), cpu(neg), tab, tab, LR, center, tab, tab)
        assert want.new_in is want.new_out and skipped == 0
        hold("one table, center %d" % center, n, n, loss, want, tab, tab)
        g_in, g_out, gloss = e.sgns_grad(pos, neg, a, a, center=center)
        assert g_in is g_out
        z = np.zeros_like(tab)
        want = sref.step(V, cpu(pos), cpu(neg), tab, tab, -1.0, center, z, z)
        hold("one table grad, center %d" % center, g_in, g_in, gloss, want, z, z)


# ---- compacted ids --------------------------------------------------------------------------------------------------------------------
def test_compacted_ids():
    from test_sparse_ids import sparse_multigraph
    s, d, w = sparse_multigraph(4, weighted=False)
    with pkg().Engine(device=0) as e:
        e.load_coo(s, d, w)
        V = e.vertices()
        assert V[0] == -2**31 and V[-1] == 2**31 - 1 and -1 in V            # the extremes, and -1 as an ordinary vertex
        rng = np.random.default_rng(8)
        W = 300
        pos, neg = V[rng.integers(0, V.size, size=(W, 3))], V[rng.integers(0, V.size, size=(W, 2))]
        pos[0], neg[0] = [-2**31, 2**31 - 1, -1], [2**31 - 1, -2**31]
        absent = [x for x in (5, -2, 123456789, 2**31 - 2, -2**31 + 1) if x not in set(V.tolist())]
        for k, x in enumerate(absent):                                     # ids between the ranks: those windows are skipped
            (pos if k % 2 else neg)[10 + k, k % 2] = x
        tin, tout = sref.tables(V.size, 64, 6)
        a, b = dev(tin), dev(tout)
        na, nb = a.clone(), b.clone()
        loss, skipped = e.sgns_step(dev(pos), dev(neg), a, b, LR, center=1, into=(na, nb), loss=True)
        want = sref.step(V, pos, neg, tin, tout, LR, 1, tin, tout)
        assert skipped == want.skipped == len(absent) > 0
        hold("compacted ids", na, nb, loss, want, tin, tout)
        assert bool((loss[10:10 + len(absent)] == 0).all())


# ---- ids that are no vertex: skipped whole, nothing outside the tables is touched ---------------------------------------------------
GAP_IDS = [3, 4, 5, 7, 8, 9, 10, 12]                                     # vmin 3, vmax 12, gaps at 6 and 11


def test_unknown_ids_are_skipped_and_the_margins_stay():
    rows = [(v, [(GAP_IDS[(i + 1) % 8], 1.0), (GAP_IDS[(i - 1) % 8], 1.0)]) for i, v in enumerate(GAP_IDS)]
    with pkg().Engine(device=0) as e:
        e.load_adjacency(rows)
        V = e.vertices()
        assert V.tolist() == GAP_IDS
        rng = np.random.default_rng(2)
        W, D, M = 64, 64, 4096
        pos, neg = V[rng.integers(0, 8, size=(W, 3))], V[rng.integers(0, 8, size=(W, 2))]
        # every kind — below vmin, above vmax, in a gap (6 and 11), -1, the ends of int32 — in pos and in neg, one per window, the
        # centre and the last lane among the places: windows 1 .. 14
        UNKNOWN = [2, 13, 6, 11, -1, 2**31 - 1, -2**31]
        NB = 2 * len(UNKNOWN)
        for k, x in enumerate(UNKNOWN):
            pos[1 + 2 * k, k % 3] = x
            neg[2 + 2 * k, k % 2] = x
        tin, tout = sref.tables(8, D, 3)
        a, b = dev(tin), dev(tout)
        POISON = 12345.0
        bufs = [torch.full((M + 8 * D + M,), POISON, dtype=torch.float32, device=DEV) for _ in range(2)]
        news = [buf[M:M + 8 * D].view(8, D) for buf in bufs]
        news[0].copy_(a)
        news[1].copy_(b)
        loss, skipped = e.sgns_step(dev(pos), dev(neg), a, b, LR, into=tuple(news), loss=True)
        want = sref.step(V, pos, neg, tin, tout, LR, 0, tin, tout)
        assert skipped == want.skipped == NB
        assert bool((loss[1:1 + NB] == 0).all()) and bool((loss[1 + NB:] > 0).all()) and float(loss[0]) > 0
        hold("unknown ids", news[0], news[1], loss, want, tin, tout)
        for buf in bufs:
            assert bool((buf[:M] == POISON).all()) and bool((buf[M + 8 * D:] == POISON).all())
        # a call of nothing but such windows changes nothing at all
        before = [n.clone() for n in news]
        loss, skipped = e.sgns_step(dev(pos[1:1 + NB]), dev(neg[1:1 + NB]), a, b, LR, into=tuple(news), loss=True)
        assert skipped == NB and bool((loss == 0).all()) and torch.equal(news[0], before[0]) and torch.equal(news[1], before[1])


# ---- saturation -----------------------------------------------------------------------------------------------------------------------
def test_saturation(karate):
    """rows that are +-0.79 times one sign pattern: every |f| is near 64 * 0.79^2 = 40"""
    e, V = karate
    pos, neg = karate_batch(e, 3, 2)
    rng = np.random.default_rng(4)
    D = 64
    pattern = rng.choice([-1.0, 1.0], size=D)
    mk = lambda: (0.79 * rng.choice([-1.0, 1.0], size=(V.size, 1)) * pattern * (1 + 0.01 * rng.uniform(-1, 1, size=(V.size, D)))).astype(np.float32)  # noqa: E731
    tin, tout = mk(), mk()
    a, b = dev(tin), dev(tout)
    na, nb = a.clone(), b.clone()
    loss, _ = e.sgns_step(pos, neg, a, b, LR, into=(na, nb), loss=True)
    want = sref.step(V, cpu(pos), cpu(neg), tin, tout, LR, 0, tin, tout)
    assert 39 < np.abs(want.f).min() and np.abs(want.f).max() < 41
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(na).all()) and bool(torch.isfinite(nb).all())
    hold("saturation", na, nb, loss, want, tin, tout)
    sign = np.array([1.0, 1.0, -1.0, -1.0])                                # labels 1, 1, 0, 0
    assert np.allclose(cpu(loss), np.maximum(-sign * want.f, 0).sum(axis=1), rtol=1e-5, atol=1e-12)     # loss = |f| of the wrong-signed targets
    assert float(loss.max()) > 39
    ga, gb, gloss = e.sgns_grad(pos, neg, a, b)
    z = np.zeros_like(tin)
    hold("saturation grad", ga, gb, gloss, sref.step(V, cpu(pos), cpu(neg), tin, tout, -1.0, 0, z, np.zeros_like(tin)), z, z)


# ---- in place -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_in_place_without_collisions_is_the_exact_step(karate, D):
    e, V = karate
    rng = np.random.default_rng(D)
    C_, K = 3, 2
    for W in (1, V.size // (C_ + K)):
        ids = rng.permutation(V)[:W * (C_ + K)].reshape(W, C_ + K).astype(np.int32)     # every vertex at most once in the call
        pos, neg = ids[:, :C_].copy(), ids[:, C_:].copy()
        tin, tout = sref.tables_for(V.size, D, 11)
        for center in (0, 1):
            a, b = dev(tin), dev(tout)
            loss, skipped = e.sgns_step(dev(pos), dev(neg), a, b, LR, center=center, loss=True)
            want = sref.step(V, pos, neg, tin, tout, LR, center, tin, tout)
            assert skipped == 0
            hold("in place, W %d D %d center %d" % (W, D, center), a, b, loss, want, tin, tout)
            sl = sref.slots_of(V, ids)
            rest_in = np.setdiff1d(np.arange(V.size), sl[:, center])
            rest_out = np.setdiff1d(np.arange(V.size), np.delete(sl, center, axis=1))
            assert np.array_equal(cpu(a)[rest_in], tin[rest_in]) and np.array_equal(cpu(b)[rest_out], tout[rest_out])
            assert not np.array_equal(cpu(a)[sl[:, center]], tin[sl[:, center]])


def test_in_place_with_collisions(karate):
    e, V = karate
    pos, neg = karate_batch(e, 5, 5)
    tin, tout = sref.tables_for(V.size, 64, 13)
    pos, neg = pos[:6].contiguous(), neg[:6].contiguous()                  # few windows of a real walk: rows repeat, and some are not named
    sl = sref.slots_of(V, np.concatenate([cpu(pos), cpu(neg)], axis=1))
    rest_in = np.setdiff1d(np.arange(V.size), sl[:, 0])
    rest_out = np.setdiff1d(np.arange(V.size), sl[:, 1:])
    assert rest_in.size and rest_out.size and np.unique(sl[:, 1:]).size < sl[:, 1:].size
    a, b = dev(tin), dev(tout)
    loss, skipped = e.sgns_step(pos, neg, a, b, LR, loss=True)
    assert skipped == 0 and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and bool(torch.isfinite(loss).all())
    assert np.array_equal(cpu(a)[rest_in], tin[rest_in]) and np.array_equal(cpu(b)[rest_out], tout[rest_out])    # only named rows change
    named_in, named_out = np.unique(sl[:, 0]), np.unique(sl[:, 1:])
    assert (cpu(a)[named_in] != tin[named_in]).any(axis=1).all() and (cpu(b)[named_out] != tout[named_out]).any(axis=1).all()
    # lr = 0 (a whole batch): both tables bit-identical afterwards, loss is the exact form's
    pos, neg = karate_batch(e, 5, 5)
    a, b = dev(tin), dev(tout)
    loss0, _ = e.sgns_step(pos, neg, a, b, 0.0, loss=True)
    assert torch.equal(a, dev(tin)) and torch.equal(b, dev(tout))
    na, nb = a.clone(), b.clone()
    loss_exact, _ = e.sgns_step(pos, neg, a, b, LR, into=(na, nb), loss=True)
    assert torch.equal(loss0, loss_exact)
    want = sref.step(V, cpu(pos), cpu(neg), tin, tout, 0.0, 0, tin, tout)
    hold("lr = 0", a, b, loss0, want, tin, tout)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw(e, pos, neg, W, C_, K, D, center, lr, tin, tout, nin, nout, n_rows, loss=None, reserved=0):
    """srw_sgns_step itself; a tensor, an address or None per pointer -> (status, *n_skipped)"""
    P = pkg()
    sp = P.SgnsParams(C_, K, D, center, lr, reserved)
    n = C.c_int64(-5)
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())      # noqa: E731
    torch.cuda.synchronize()
    rc = P.lib().srw_sgns_step(e.h, ptr(pos), ptr(neg), W, C.byref(sp), ptr(tin), ptr(tout), ptr(nin), ptr(nout), n_rows, ptr(loss),
                               C.byref(n))
    return rc, n.value


def test_refusals_leave_the_tables_untouched(karate):
    P = pkg()
    e, V = karate
    pos, neg = karate_batch(e, 3, 2)
    W, D, nV = pos.shape[0], 64, 34
    tin, tout = sref.tables(nV, D, 1)
    big = torch.zeros((6 * nV * D,), dtype=torch.float32, device=DEV)       # four tables and room to overlap them
    view = lambda k, off=0: big[k * nV * D + off:(k + 1) * nV * D + off].view(nV, D)      # noqa: E731
    a, b, na, nb = view(0), view(1), view(2), view(3)
    a.copy_(dev(tin)); b.copy_(dev(tout)); na.copy_(a); nb.copy_(b)
    saved = big.clone()
    ok = dict(pos=pos, neg=neg, W=W, C_=3, K=2, D=D, center=0, lr=LR, tin=a, tout=b, nin=na, nout=nb, n_rows=nV)
    nan, inf = float("nan"), float("inf")
    refused = [
        dict(n_rows=33), dict(n_rows=35), dict(n_rows=0),
        dict(D=0), dict(D=32), dict(D=96), dict(D=100), dict(D=576), dict(D=-64),
        dict(C_=0), dict(K=-1), dict(C_=1, K=0), dict(C_=5, K=60), dict(C_=65, K=0), dict(C_=1, K=64), dict(C_=2**31 - 1, K=2),
        dict(center=-1), dict(center=3), dict(center=64),
        dict(neg=None),
        dict(lr=nan), dict(lr=inf), dict(lr=-inf), dict(reserved=1),
        dict(nin=None), dict(nout=None),
        dict(W=-1), dict(pos=None), dict(tin=None), dict(tout=None),
        dict(pos=pos.data_ptr() + 2), dict(tin=a.data_ptr() + 2), dict(nout=nb.data_ptr() + 1),
        dict(nin=view(2, 64)),                                             # new in over new out's first bytes
        dict(nin=view(0, 64), nout=view(4)),                               # new in over part of the old in
        dict(nout=view(0, nV * D - 64), nin=view(4)),                      # new out over the ends of old in and old out
        dict(tout=view(0, 64), nout=view(4)),                              # the two old tables over each other
        dict(tout=a),                                                      # one table for both roles, two new tables
        dict(nout=na),                                                     # two tables, one new table
        dict(nin=b, nout=view(4)), dict(nout=a, nin=view(4)),              # a new table that is the other role's old table
        dict(loss=view(0)[0]), dict(loss=view(3)[nV - 1, D - 1:]), dict(loss=view(1).view(-1)[nV * D - W:]),     # the losses over a table
    ]
    for change in refused:
        rc, n = raw(e, **{**ok, **change})
        assert rc == P.ERR_INVALID, change
        assert torch.equal(big, saved), change
        assert e.h and P.lib().srw_last_error(e.h).decode().startswith("srw_sgns_step"), change
    # ... and what is allowed: the call itself, nothing to do, the in-place form by address, one table with one new table
    assert raw(e, **{**ok, "W": 0, "pos": None, "neg": None, "tin": None, "tout": None, "nin": None, "nout": None}) == (P.OK, 0)
    assert torch.equal(big, saved)
    empty = torch.empty((0, 3), dtype=torch.int32, device=DEV)
    assert e.sgns_step(empty, None, a, b, LR) == (None, 0) and torch.equal(big, saved)
    assert raw(e, **{**ok, "loss": view(4).view(-1)[:W]}) == (P.OK, 0)      # the losses right behind the last table
    want = sref.step(V, cpu(pos), cpu(neg), tin, tout, LR, 0, tin, tout)
    hold("the call the refusals were cut from", na, nb, None, want, tin, tout)
    assert torch.equal(a, dev(tin)) and torch.equal(b, dev(tout))
    assert raw(e, **{**ok, "nin": a, "nout": b})[0] == P.OK                # in place, spelled with the tables' own addresses
    assert raw(e, **{**ok, "tout": a, "nin": na, "nout": na})[0] == P.OK
    # the handle's state
    with P.Engine(device=0, rank=0, world=2) as shard:
        rc, _ = raw(shard, **ok)
        assert rc == P.ERR_INVALID and "world == 1" in P.lib().srw_last_error(shard.h).decode()
    with P.Engine(device=0) as fresh:
        rc, _ = raw(fresh, **ok)
        assert rc == P.ERR_INVALID and "no graph" in P.lib().srw_last_error(fresh.h).decode()
        fresh.load_edgelist(KARATE, directed=False)
        fresh._ck(P.lib().srw_shard_select(fresh.h, 1))
        rc, _ = raw(fresh, **ok)
        assert rc == P.ERR_INVALID and "population 1" in P.lib().srw_last_error(fresh.h).decode()
        fresh._ck(P.lib().srw_shard_select(fresh.h, 0))
        big.copy_(saved)
        assert raw(fresh, **ok) == (P.OK, 0)
    with pytest.raises(TypeError, match="in device memory"):
        e.sgns_step(pos.cpu(), neg, a, b, LR)


# ---- train_sgns -----------------------------------------------------------------------------------------------------------------------
def test_train_sgns_on_karate(oracle):
    """dim 64, C = 5, K = 5, 5 epochs, walk length 20, one batch of all 34 sources per epoch: the first epoch's mean loss is the first
    step's.  emb_out starts at zero, so at the OLD values every f of the first step is 0 and every window's loss is 9 ln 2: the exact
    form over the same batch is held to that under the loss tolerance.  train_sgns itself steps in place, and there the assertion
    cannot hold as it stands: a read of the first step may see adds of the same step (measured: 8e-5 from 9 ln 2, the tolerance is
    4e-5).  What such a read can see is bounded from the batch itself.  To first order in lr a row of emb_out is
    lr sum_j g_j emb_in[c_j] over the windows j that name it as a target and have added already, so for a pair (c, t)
        |f| <= lr g_max sum_c' N[t][c'] |<emb_in[c], emb_in[c']>|,      N[t][c'] = windows with centre c' and target t,
    with g_max = sigma(f_max) (|g| <= sigma(|f|): 1/2 at f = 0), and |softplus(+-f) - ln 2| <= |f| / 2 + f^2 / 8.  The mean over the
    windows of the sum over their targets of that, from f_max of every pair, is the first-order bound; it is doubled for what is
    second order in lr (the drift of the centre rows, themselves sums of lr g emb_out rows — an estimate, not a bound) and the loss
    tolerance is added."""
    from test_gpu_embedding import _cos_split
    dim, C_, K, T = 64, 5, 5, 9
    with pkg().Engine(device=0) as e:
        e.load_edgelist(KARATE, directed=False)
        V = e.vertices()
        emb_in, emb_out, means = e.train_sgns(dim, C_, K, 5, 34, walk_length=20)
        assert emb_in.shape == (34, dim) and emb_out.shape == (34, dim) and len(means) == 5
        assert bool(torch.isfinite(emb_in).all()) and bool(torch.isfinite(emb_out).all()) and np.isfinite(means).all()
        # the first step again, in the exact form: the same generator, the same shuffle, the same batch
        gen = torch.Generator().manual_seed(1)
        first_in = ((torch.rand((34, dim), generator=gen, dtype=torch.float32) - 0.5) / dim).to(DEV)
        order = torch.as_tensor(V, dtype=torch.int32)[torch.randperm(34, generator=gen)].to(DEV)
        pos, neg = e.walk_skipgram_batch(order, C_, K, sg_seed=1, epoch=0, walk_length=20)
        zero = torch.zeros_like(first_in)
        loss, skipped = e.sgns_step(pos, neg, first_in, zero, LR, into=(first_in.clone(), zero.clone()), loss=True)
        want = sref.step(V, cpu(pos), cpu(neg), cpu(first_in), cpu(zero), LR, 0, cpu(first_in), cpu(zero))
        tol = sref.loss_bound(want)
        assert skipped == 0 and want.S == 0 and np.allclose(want.loss, T * math.log(2.0), rtol=1e-15)
        print("first step, exact form: worst |loss - 9 ln 2| / tolerance %.4f" % sref.worst(cpu(loss), want.loss, tol))
        assert (np.abs(cpu(loss).astype(np.float64) - T * math.log(2.0)) <= tol).all()
        sl = sref.slots_of(V, np.concatenate([cpu(pos), cpu(neg)], axis=1))
        N = np.zeros((34, 34))
        np.add.at(N, (sl[:, 1:], np.broadcast_to(sl[:, :1], sl[:, 1:].shape)), 1.0)           # N[t][c']
        x = cpu(first_in).astype(np.float64)
        reach = N @ np.abs(x @ x.T)                                                     # [t][c]: sum_c' N[t][c'] |<in[c], in[c']>|
        f_max = 0.025 * float(sref.sigmoid(0.025 * reach.max())) * reach               # g_max = sigma of the largest f that |g| <= 1 allows
        per_pair = f_max / 2 + f_max ** 2 / 8
        first_order = float(per_pair[sl[:, 1:], sl[:, :1]].sum(axis=1).mean())
        allowance = 2 * first_order + float(tol.max())
        print("mean loss per epoch", means, " 9 ln 2 =", T * math.log(2.0), " in-place allowance %.3g (first order %.3g, largest f %.3g)"
              % (allowance, first_order, f_max.max()))
        assert abs(means[0] - T * math.log(2.0)) <= allowance
        assert means[-1] < means[0]
        nb, nn = _cos_split(oracle.Graph.load(KARATE, directed=False), V, cpu(emb_in))
        print("cosine of neighbours %.4f, of non-neighbours %.4f (not asserted)" % (nb, nn))
