"""Mode A on the device at its edges: k_alias_build / k_alias_link (alias_tables.hip) and k_walk_alias (walk_kernels.hip).

Rows, graphs and the statements they are held to come from tests/mode_a_ref.py; tests/test_mode_a_ref_cpu.py checks, without a GPU,
that those inputs hit what they are meant to hit and that the oracle itself keeps the statements.  Here:
  a. the tables of every boundary row (tile, block-scan and LDS / HBM staging boundaries, ties at every prefix, prefix sums beyond
     2^64, the certificate at 29 against 30, zero and subnormal weights, irregular rows) equal the oracle's bit for bit AND imply the
     weights' distribution within the derived bound, on the device's own arrays;
  b. a first step over those tables; c. the path staging at every tile cut, both strides, walkers stopping at every length;
  d. the trial cap, to the trial; e. the return edge's weight (hint, NaN fallback, zero, absent); f. membership by the shorter row;
  g. the walk's distribution against the float64 restatement — the one test that does not go through the oracle.
Each test asserts the path it means to take (kernel_kind, the regular flag, row lengths, trials, fallbacks)."""
import numpy as np
import pytest

import mode_a_ref as ref
from helpers import pkg

pytestmark = pytest.mark.gpu

ROWS = ref.boundary_rows()
DST0 = 100000                          # destinations 100000 + k: no row of their own, every first step ends the walk
GRAPHS = ref.walk_edge_graphs()


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


def _same(a, b):
    """a, b: (paths, lens, ...) — whole rows, the -1 padding included"""
    if a[0].shape == b[0].shape and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]):
        return True, ""
    bad = np.nonzero((a[0] != b[0]).any(axis=1) | (a[1] != b[1]))[0]
    return False, "%d walkers differ, first %d:\n  %s\n  %s" % (len(bad), bad[0], a[0][bad[0]], b[0][bad[0]])


def _load(eng, oracle, name):
    s, d, w, directed = GRAPHS[name]
    g = oracle.Graph.from_coo(s, d, w, directed=directed)
    eng.load_coo(s, d, w, directed=directed)
    assert eng.stats() == (g.num_vertices, g.num_entries)
    return g


def _alias_walk(eng, g, **kw):
    """the device's Mode A walk against the oracle's, every walker; returns (device result, oracle result)"""
    dev_kw = {k: kw.pop(k) for k in ("edge_hash", "nt_loads") if k in kw}
    a = eng.walk(sampler="alias", **kw, **dev_kw)
    b = g.walk(sampler=1, **kw)
    ok, why = _same(a, b)
    assert ok, "%s %s: device != oracle: %s" % (kw, dev_kw, why)
    assert a[2]["kernel_kind"] == 3 and a[2]["n_steps"] == b[2], (kw, a[2])
    return a, b


# ---- a, b: the boundary rows ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_graph(oracle):
    """one directed graph whose vertex i has row i of boundary_rows() (a directed load keeps the input order)"""
    s = np.concatenate([np.full(len(w), i, np.int32) for i, (_, w, _) in enumerate(ROWS)])
    d = np.concatenate([DST0 + np.arange(len(w), dtype=np.int32) for _, w, _ in ROWS])
    w = np.concatenate([w for _, w, _ in ROWS])
    g = oracle.Graph.from_coo(s, d, w, directed=True)
    degs = np.array([g.degree(i) for i in range(len(ROWS))])
    assert degs.tolist() == [len(r[1]) for r in ROWS]
    assert degs.max() > 2048 and (degs <= 2048).any() and (degs > 2048).sum() >= 20        # both staging paths, LDS and HBM
    return s, d, w, g


def test_tables_of_the_boundary_rows(eng, rows_graph):
    s, d, w, g = rows_graph
    eng.load_coo(s, d, w, directed=True)
    differ, wrong = [], []
    for v, (name, wv, regular) in enumerate(ROWS):
        a, b = eng.alias_row(v), g.alias_row(v)
        assert len(a[1]) == len(b[1]) == len(wv), name
        assert np.array_equal(eng.neighbors(v)[1].view(np.uint32), wv.view(np.uint32)), name      # the row is the input, in its order
        if a[0] != b[0] or a[0] != int(regular):
            differ.append(name + ":regular")
            continue
        if not regular:
            continue
        if not (np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])):
            differ.append(name)
        # the device's own arrays against the weights, independent of the oracle (exact integers: about 0.1 s for a 32 768-entry row,
        # 0.6 s for all of them)
        if not ref.table_is_well_formed(a[1], a[2]) or ref.implied_error(wv, a[1], a[2]) > 1:
            wrong.append(name)
    assert not differ and not wrong, "tables differ from the oracle's: %s; tables that are not the weights' distribution: %s" % (differ, wrong)


@pytest.mark.parametrize("nt_loads", [True, False])
def test_first_step_over_the_boundary_rows(eng, rows_graph, nt_loads):
    s, d, w, g = rows_graph
    eng.load_coo(s, d, w, directed=True)
    src = np.arange(len(ROWS), dtype=np.int32)
    a, b = _alias_walk(eng, g, sources=src, walk_length=2, num_walks=64, seed=21, nt_loads=nt_loads)
    assert (a[1] == 2).all() and (a[0][:, 2:] == -1).all()               # the destinations are dead ends
    n_irregular = sum(1 for r in ROWS if not r[2])
    assert a[2]["fallbacks"] == 64 * n_irregular and a[2]["trials"] == 64 * (len(ROWS) - n_irregular), a[2]
    assert a[2]["dead_ends"] == 64 * len(ROWS)
    took = a[0][:, 1].reshape(64, len(ROWS)) - DST0                       # the entry each walker took
    big = [v for v, r in enumerate(ROWS) if r[0].startswith("u128")]
    assert all(len(np.unique(took[:, v])) > 32 for v in big)


# ---- c: path staging -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ref.STAGING_L)
def test_path_staging_at_every_cut(eng, oracle, L):
    """odd and even row stride L + 2, full tiles of 16 and every partial last run, walkers that stop at every position of a tile"""
    g = _load(eng, oracle, "staging")
    for p, q in ref.STAGING_PQ:
        a, b = _alias_walk(eng, g, walk_length=L, num_walks=ref.STAGING_NUM_WALKS, seed=5, p=p, q=q)
        assert len(b[1]) >= 3 * 256 + 1
        want = set(range(1, min(L + 2, 34) + 1)) | {L + 2}
        assert want <= set(b[1].tolist()), (L, p, q, sorted(want - set(b[1].tolist())))
        assert a[2]["fallbacks"] == 0 and a[2]["dead_ends"] > 0
        assert (a[2]["trials"] > a[2]["n_steps"]) == (p != 1.0)


# ---- d: the trial cap -------------------------------------------------------------------------------------------------------------------
def test_trial_cap(eng, oracle):
    """one call; a lane runs at most 7 x 65 536 trials.  The number of trials is the replayed one, to the trial: a cap at any other
    count would show here even where the paths happened to agree."""
    g = _load(eng, oracle, "cap")
    a, b = _alias_walk(eng, g, **ref.CAP_KW)
    assert (a[1] == 9).all()
    tables = {int(v): eng.alias_row(int(v))[1:] for v in g.vertices()}
    s, d, w, directed = GRAPHS["cap"]
    rp, trials = ref.cap_walk(ref.adjacency(s, d, w, directed), tables, **ref.CAP_KW)
    assert np.array_equal(rp, a[0])
    assert trials >= 65536 and a[2]["trials"] == trials, (a[2]["trials"], trials)


# ---- e: the return edge's weight --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi", "multi_directed"])
@pytest.mark.parametrize("p,q", [(0.25, 4.0), (0.25, 0.25), (0.5, 1.0)])
def test_return_edge_weight(eng, oracle, name, p, q):
    """undirected: the record's hint where the float64 sum of a parallel group is a float32, the search where it is not (NaN);
    directed: every hint is NaN and the occurrences come from the equal-range search"""
    g = _load(eng, oracle, name)
    for edge_hash in (True, False):
        a, _ = _alias_walk(eng, g, walk_length=20, num_walks=50, seed=13, p=p, q=q, edge_hash=edge_hash)
        assert a[2]["fallbacks"] == 0 and (a[2]["trials"] > a[2]["n_steps"]) == (q != 1.0)    # q = 1: nothing is ever rejected
        assert a[2]["dead_ends"] == 0 and (a[1] == 22).all()


@pytest.mark.parametrize("q", [4.0, 1.0])
def test_no_fold_without_return_weight(eng, oracle, q):
    """a -> b weighs 1 and b -> a weighs 0 or does not exist: 1 / p > Q and nothing to fold"""
    g = _load(eng, oracle, "noreturn")
    for edge_hash in (True, False):
        a, _ = _alias_walk(eng, g, walk_length=20, num_walks=50, seed=17, p=0.25, q=q, edge_hash=edge_hash)
        assert a[2]["fallbacks"] == 0 and (a[1] == 22).all()


# ---- f: membership by the shorter row ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [4.0, 0.25])
def test_membership_by_the_shorter_row(eng, oracle, q):
    g = _load(eng, oracle, "hub")
    assert g.degree(0) == ref.HUB_N and g.degree(1) == 2
    a, _ = _alias_walk(eng, g, walk_length=10, num_walks=2, seed=19, p=1.0, q=q, edge_hash=False)
    h = eng.walk(sampler="alias", walk_length=10, num_walks=2, seed=19, p=1.0, q=q, edge_hash=True)
    ok, why = _same(a, h)
    assert ok, "sorted rows != edge hash: %s" % why
    assert a[2]["trials"] > a[2]["n_steps"] and a[2]["fallbacks"] == 0
    # walkers came to a leaf from the hub and to the hub from a leaf: both orders of the two degrees were asked
    hub_then_leaf = (a[0][:, :-2] == 0) & (a[0][:, 1:-1] > 0) & (a[0][:, 2:] > 0)
    leaf_then_hub = (a[0][:, :-2] > 0) & (a[0][:, 1:-1] == 0) & (a[0][:, 2:] > 0)
    assert hub_then_leaf.sum() > 100 and leaf_then_hub.sum() > 100


# ---- g: the distribution on the device, against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("p,q", ref.STAT_PQ)
def test_device_walk_has_the_stated_distribution(eng, directed, p, q):
    s, d, w = ref.stat_graph()
    eng.load_coo(s, d, w, directed=directed)
    assert all(eng.alias_row(int(v))[0] == 1 for v in eng.vertices() if len(eng.neighbors(int(v))[0]))
    paths, lens, st = eng.walk(sampler="alias", p=p, q=q, **ref.STAT_KW)
    assert st["kernel_kind"] == 3 and st["fallbacks"] == 0 and len(lens) == 12 * ref.STAT_KW["num_walks"]
    expected = ref.transition_probabilities(ref.adjacency(s, d, w, directed), p, q, "exact")
    z, dof, left = ref.chi_z(ref.triple_counts(paths), expected, ref.STAT_KW["num_walks"])
    print("directed %d p %g q %g: z = %.2f, dof %d, %.1f %% of cells left out" % (directed, p, q, z, dof, 100 * left))
    assert abs(z) <= 5 and left <= 0.10, (z, dof, left)
