"""The first-order kernel's path flush on the device (csrc/walk_kernels.hip): rows go out as runs that lie inside one
address-aligned line, cut by each row's own address.  Whatever the stride and the phase of a row, every slot of the whole [n, L + 2]
array — the -1 tails of dead walkers included — and lens equal the oracle's, and the walk under legacy_flush=True (the flush of before,
include/stellar_rw.h: SRW_WALK_LEGACY_FLUSH) of the same handle gives the same.

Strides L + 2 for L in LS: odd ones (every phase of a line occurs among the rows), multiples of 16 (one phase) and the headline's 82.

The oracle walks every configuration ONCE, at the longest L: a walker's draw at step s is keyed by (seed, iteration, source, s) — or is
the constant — and nothing else, so its walk of length L is the first L + 2 slots of its walk of length 81 and its len is capped at
L + 2.  test_prefix_rule_holds_in_the_oracle checks that on the oracle itself.
"""
import numpy as np
import pytest

from conftest import KARATE
from helpers import pkg

pytestmark = pytest.mark.gpu

LS = (1, 2, 13, 14, 15, 16, 17, 30, 31, 46, 79, 80, 81)
LMAX = max(LS)
SEED = 2027


@pytest.fixture(scope="module")
def graphs(oracle):
    """{name: (engine, oracle graph)}: karate (34 walkers: less than a wave), RMAT-10 and RMAT-13 undirected, RMAT-10 directed (dead ends
    at step 1 and later: -1 tails)."""
    out = {}
    e = pkg().Engine(device=0)
    e.load_edgelist(KARATE, directed=False)
    out["karate"] = (e, oracle.Graph.load(KARATE, directed=False))
    for name, scale, directed in (("rmat10", 10, False), ("rmat13", 13, False), ("rmat10d", 10, True)):
        s, d = oracle.rmat_edges(scale, 16 << scale, seed=9)
        e = pkg().Engine(device=0)
        e.load_coo(s, d, None, directed=directed)
        out[name] = (e, oracle.Graph.from_coo(s, d, None, directed=directed))
    yield out
    for e, _ in out.values():
        e.close()


SOURCES = {}                                                     # name -> the 65 ids of test_source_list_of_65
_REF = {}


def _reference(oracle, graphs, name, num_walks, rng, use_sources):
    """(paths, lens) of the oracle at LMAX for one configuration, computed once."""
    key = (name, num_walks, rng, use_sources)
    if key not in _REF:
        g = graphs[name][1]
        src = None
        if use_sources:
            src = SOURCES.setdefault(name, np.random.default_rng(65).choice(g.vertices(), 65, replace=True).astype(np.int32))
        kw = {"rng": "const", "const_r": 0.37} if rng == "const" else {"seed": SEED}
        rp, rl, _ = g.walk(sources=src, walk_length=LMAX, num_walks=num_walks, threads=oracle.threads(), **kw)
        rp.setflags(write=False); rl.setflags(write=False)
        _REF[key] = (rp, rl, src)
    return _REF[key]


def _check(oracle, graphs, name, L, num_walks=1, rng="philox", use_sources=False, record_bytes=16, **eng_kw):
    """The default flush and the legacy one against the oracle: whole arrays."""
    eng = graphs[name][0]
    rp81, rl81, src = _reference(oracle, graphs, name, num_walks, rng, use_sources)
    rp, rl = rp81[:, :L + 2], np.minimum(rl81, L + 2)
    kw = {"rng": "const", "const_r": 0.37} if rng == "const" else {"seed": SEED}
    res = {}
    for legacy in (False, True):
        paths, lens, st = eng.walk(sources=src, legacy_flush=legacy, walk_length=L, num_walks=num_walks, **kw, **eng_kw)
        assert st["kernel_kind"] == 1 and st["record_bytes"] == record_bytes, st
        assert paths.shape == rp.shape, (paths.shape, rp.shape)
        bad = np.flatnonzero((paths != rp).any(axis=1))
        assert bad.size == 0, ("legacy" if legacy else "aligned", name, L, bad[:8], paths[bad[:1]], rp[bad[:1]])
        assert np.array_equal(lens, rl)
        res[legacy] = (paths, lens)
    assert np.array_equal(res[False][0], res[True][0]) and np.array_equal(res[False][1], res[True][1])
    return rp, rl


def test_walker_counts_exercise_partial_waves(graphs):
    assert graphs["karate"][1].num_vertices == 34
    for name in ("rmat10", "rmat13", "rmat10d"):
        n = graphs[name][1].num_vertices
        assert n % 64 != 0 and (3 * n) % 64 != 0, (name, n)     # a partial wave, and iterations that begin inside a wave


def test_prefix_rule_holds_in_the_oracle(oracle, graphs):
    """What _check derives from the LMAX walk is what the oracle gives when asked for the shorter walk."""
    for name, L in (("rmat10d", 13), ("rmat10d", 1), ("karate", 30)):
        g = graphs[name][1]
        rp81, rl81, _ = _reference(oracle, graphs, name, 3, "philox", False)
        rp, rl, _ = g.walk(walk_length=L, num_walks=3, seed=SEED)
        assert np.array_equal(rp, rp81[:, :L + 2]) and np.array_equal(rl, np.minimum(rl81, L + 2))


@pytest.mark.parametrize("L", LS)
def test_every_slot_matches_oracle_and_legacy(oracle, graphs, L):
    for name in ("karate", "rmat10", "rmat13"):
        _check(oracle, graphs, name, L)
    for name in ("karate", "rmat10"):                            # rows cross iteration boundaries
        _check(oracle, graphs, name, L, num_walks=3)


@pytest.mark.parametrize("L", LS)
def test_dead_ends_keep_their_tails(oracle, graphs, L):
    rp, rl = _check(oracle, graphs, "rmat10d", L, num_walks=3)
    assert (rl == 1).any()                                       # dead at step 1
    if L >= 13:
        assert ((rl > 2) & (rl < L + 1)).any()                   # and later
        assert (rp[rl < L + 1, -1] == -1).all()


@pytest.mark.parametrize("L", LS)
def test_source_list_of_65(oracle, graphs, L):
    _check(oracle, graphs, "rmat10", L, num_walks=3, use_sources=True)


@pytest.mark.parametrize("L", LS)
def test_other_record_paths_through_the_same_flush(oracle, graphs, L):
    _check(oracle, graphs, "rmat10", L, num_walks=3, record_bytes=32, compact=False)      # the 32-byte records
    _check(oracle, graphs, "rmat10", L, num_walks=3, rng="const", record_bytes=32)        # the exact path, constant draws
