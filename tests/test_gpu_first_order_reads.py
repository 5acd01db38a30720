"""CFO_GD_EDGE on the device: the compact-record pick loads ONE record per step on the buckets whose predecessor sits exactly on the
bucket's threshold (every such bucket of a unit-weight row), and picks what it picked before.

  * srw_cfo_pick (the pick itself, one draw per lane) on the rows and draws of tests/test_first_order_code_cpu.py, as stars: positions
    against the oracle's RandomSample.sample, loads against the numpy restatement, with and without SRW_NO_EDGE_CODE;
  * a star of 2^20 leaves: every walker of the compact walk against the 32-byte records' walk (fo_pick: untouched, independent), sampled
    sources against the oracle, and ent_reads = steps + the hub steps whose draw is the lowest of its bucket — counted with a numpy Philox;
  * RMAT-13: the oracle's paths, one record per step; under the switch the same paths and the loads of before.
"""
import contextlib
import os

import numpy as np
import pytest

import first_order_code_ref as ref
from helpers import pkg
from skipgram_ref import philox_np

pytestmark = pytest.mark.gpu

ROWS = ref.rows()


@contextlib.contextmanager
def _no_edge_code():
    """SRW_NO_EDGE_CODE for the statements inside: the switch is read when the compact tables are built, so the first pick or walk of
    an engine goes in here (tests/conftest.py: a test that needs a switch sets it itself and takes it away again)."""
    os.environ["SRW_NO_EDGE_CODE"] = "1"
    try:
        yield
    finally:
        del os.environ["SRW_NO_EDGE_CODE"]


@pytest.fixture(scope="module")
def stars():
    """One graph: row i of ROWS is the star of hub i, its leaves in the row's order.  (engine, engine with plain tables, {name: hub})."""
    src, dst, w = [], [], []
    nxt = len(ROWS)
    hubs = {}
    for i, (name, wr) in enumerate(ROWS):
        hubs[name] = i
        src.append(np.full(len(wr), i, np.int32)); dst.append(np.arange(nxt, nxt + len(wr), dtype=np.int32)); w.append(wr)
        nxt += len(wr)
    src, dst, w = np.concatenate(src), np.concatenate(dst), np.concatenate(w)
    engs = []
    for plain in (False, True):
        e = pkg().Engine(device=0)
        e.load_coo(src, dst, w, directed=False)
        if plain:
            with _no_edge_code():
                e.cfo_pick(0, [0])                       # builds the tables
        engs.append(e)
    yield engs[0], engs[1], hubs
    for e in engs:
        e.close()


@pytest.mark.parametrize("name", [n for n, _ in ROWS])
def test_hook_positions_and_reads(stars, oracle, name):
    eng, eng_plain, hubs = stars
    w = dict(ROWS)[name]
    deg = len(w)
    ids, wr = eng.neighbors(hubs[name])
    assert np.array_equal(wr, w)                         # the hub's row is the row, in its order
    c, code = ref.build(w)
    _, plain = ref.build(w, edge_code=False)
    m = ref.draws(w, c)
    pos, reads = eng.cfo_pick(hubs[name], m)
    pos_p, reads_p = eng_plain.cfo_pick(hubs[name], m)
    want = np.array([oracle.sample_index(w, np.float32(int(x)) * np.float32(2.0 ** -24)) for x in m])    # m * 2^-24 is exact in float32
    assert np.array_equal(pos, want), np.flatnonzero(pos != want)[:8]
    assert np.array_equal(pos_p, want), np.flatnonzero(pos_p != want)[:8]
    j = (m * deg) >> 24
    coded = code[j] == ref.EDGE
    lowest = (m >= 1) & ((((m - 1) * deg) >> 24) < j)
    one = coded & ~lowest & (c[j] >= m)
    print("%s: deg %d, %d draws, %d in coded buckets, %d of them lowest, %d served by the loaded record" %
          (name, deg, len(m), coded.sum(), (coded & lowest).sum(), one.sum()))
    assert np.all(reads[one] == 1)
    assert np.all(reads[coded & lowest] == 2)
    assert np.all(reads_p[one] == 3)                     # under the switch: j, j - 1, j again
    assert np.all(reads_p[coded & lowest] == 2)
    # and every draw loads what the restated pick loads
    model = np.array([ref.pick(c, code, int(x)) for x in m])
    model_p = np.array([ref.pick(c, plain, int(x), reload=True) for x in m])
    assert np.array_equal(pos, model[:, 0]) and np.array_equal(reads, model[:, 1]), np.flatnonzero(reads != model[:, 1])[:8]
    assert np.array_equal(reads_p, model_p[:, 1]), np.flatnonzero(reads_p != model_p[:, 1])[:8]


def test_hook_rejects_what_it_cannot_pick(stars):
    eng, _, hubs = stars
    with pytest.raises(pkg().SrwError):
        eng.cfo_pick(hubs["unit16"], [1 << 24])          # not a 24-bit draw
    with pytest.raises(pkg().SrwError):
        eng.cfo_pick(10 ** 8, [0])                       # no such vertex
    pos, reads = eng.cfo_pick(hubs["unit16"], [])
    assert len(pos) == 0 and len(reads) == 0


N_LEAVES = 1 << 20
STAR_L = 8


def _lowest_hub_draws(paths, seed, deg, hub=0):
    """(# hub steps, # hub steps whose draw is the lowest of a bucket j >= 1): walker of source v draws m = philox(ctr = (iteration 0,
    v, step, 0), key = (seed, 0))[0] >> 8 at step s (device_common.h:walk_bits24); it stands on the hub before step s iff paths[v][s - 1]
    is the hub."""
    n_hub = n_low = 0
    srcs = paths[:, 0].astype(np.uint64)
    for s in range(1, paths.shape[1]):
        at = paths[:, s - 1] == hub
        m = (philox_np(0, srcs[at], s, 0, seed, 0)[0] >> np.uint64(8)).astype(np.int64)
        j = (m * deg) >> 24
        low = (m >= 1) & ((((m - 1) * deg) >> 24) < j) & (j >= 1)
        n_hub += int(at.sum()); n_low += int(low.sum())
    return n_hub, n_low


@pytest.mark.parametrize("pattern", ["unit", "1.5_0.5"])
def test_star_walk(oracle, pattern):
    src = np.zeros(N_LEAVES, np.int32); dst = np.arange(1, N_LEAVES + 1, dtype=np.int32)
    w = None if pattern == "unit" else np.tile(np.array([1.5, 0.5], np.float32), N_LEAVES // 2)
    seed = 77
    with pkg().Engine(device=0) as eng:
        eng.load_coo(src, dst, w, directed=False)
        paths, lens, st = eng.walk(walk_length=STAR_L, seed=seed)
        assert st["kernel_kind"] == 1 and st["record_bytes"] == 16, st
        pf, lf, stf = eng.walk(walk_length=STAR_L, seed=seed, compact=False)
        assert stf["record_bytes"] == 32, stf
    assert np.array_equal(paths, pf) and np.array_equal(lens, lf)           # every walker
    assert st["n_steps"] == stf["n_steps"] == (N_LEAVES + 1) * (STAR_L + 1)
    g = oracle.Graph.from_coo(src, dst, w, directed=False)
    some = np.unique(np.concatenate([[0, 1, N_LEAVES], np.random.default_rng(5).integers(0, N_LEAVES + 1, 13)])).astype(np.int32)
    rp, rl, _ = g.walk(sources=some, walk_length=STAR_L, seed=seed)
    assert np.array_equal(paths[some], rp) and np.array_equal(lens[some], rl)   # (vertex v is walker v: ids 0 .. 2^20, all present)
    n_hub, n_low = _lowest_hub_draws(paths, seed, N_LEAVES)
    print("%s star: %d hub steps, %d lowest draws of a bucket j >= 1; ent_reads %d, steps %d" % (pattern, n_hub, n_low, st["ent_reads"], st["n_steps"]))
    assert n_low >= 1000                                                     # about 2^20 * 4 / 16 expected: the boundary is exercised
    if pattern == "unit":
        # 2^24 / 2^20 = 16 draws per bucket, every bucket j >= 1 coded: two loads for its lowest draw, one for the other fifteen;
        # a leaf's row has one entry: one load
        assert st["ent_reads"] == st["n_steps"] + n_low, (st["ent_reads"], st["n_steps"], n_low)


def test_rmat13_one_record_per_step(oracle):
    scale, L, seed = 13, 30, 2026
    s, d = oracle.rmat_edges(scale, 16 << scale, seed=9)
    g = oracle.Graph.from_coo(s, d, None, directed=False)
    rp, rl, rsteps = g.walk(walk_length=L, seed=seed)
    out = {}
    for plain in (False, True):
        with pkg().Engine(device=0) as eng:
            eng.generate_rmat(scale, 16 << scale, seed=9)
            if plain:
                with _no_edge_code():
                    paths, lens, st = eng.walk(walk_length=L, seed=seed)
            else:
                paths, lens, st = eng.walk(walk_length=L, seed=seed)
        assert st["kernel_kind"] == 1 and st["record_bytes"] == 16, st
        assert np.array_equal(paths, rp) and np.array_equal(lens, rl) and st["n_steps"] == rsteps
        out[plain] = st["ent_reads"] / st["n_steps"]
    print("RMAT-13 records per step: %.5f coded, %.5f plain" % (out[False], out[True]))
    assert out[False] < 1.001
    assert out[True] > 1.03
