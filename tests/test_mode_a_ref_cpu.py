"""Mode A without a GPU: the footing of tests/test_gpu_mode_a_edges.py.

  - the oracle's alias_row on every row of mode_a_ref.boundary_rows(): regular as named, the table well formed, and the distribution it
    implies within the derived bound of mode_a_ref.implied_error — the oracle's own exactness, asserted by test_mode_a.py up to
    n = 128, extended to the shapes the GPU file builds (tile, block-scan and staging boundaries, prefix sums beyond 2^64);
  - the conditions on the GPU file's inputs, so that a GPU test cannot silently miss its target;
  - the oracle's Mode A walk against a float64 restatement of the transition probabilities that does not go through the oracle
    (mode_a_ref.transition_probabilities), as a chi-square over the (v1, v2, v3) triples of 50 000 walks per vertex, with three wrong
    readings of the specification that the same statistic must reject by a wide margin;
  - the trial cap of the rejection loop, reached on purpose and replayed trial for trial.

What the statistical test cannot see: a bias of about 1 % in one cell is within its noise (a cell of 5 000 expected walks has a
standard deviation of 70), and so is anything that moves probability only among the cells left out for NW * p < 10.  It tells a
wrong DEFINITION (a fold that is missing, a bias read the other way, weights ignored) from the right one; subtle defects of a
kernel are the job of the bit-parity tests against the oracle."""
import numpy as np
import pytest

import mode_a_ref as ref

ROWS = ref.boundary_rows()
BY_NAME = {name: (w, regular) for name, w, regular in ROWS}


# ---- the oracle's tables on the boundary rows -----------------------------------------------------------------------------------------
def test_boundary_rows_are_the_ones_named():
    names = [r[0] for r in ROWS]
    for n in ref.LENGTHS:
        for pat in ("tie3113", "oneheavy_first", "oneheavy_mid", "oneheavy_last", "onelight_first", "onelight_last", "rand", "zeros"):
            assert "%s_%d" % (pat, n) in names
        for split in (256, 257):
            assert ("lights_then_heavies_%d_%d" % (split, n) in names) == (n > split) == ("heavies_then_lights_%d_%d" % (split, n) in names)
        assert ("zeros_tile_%d" % n in names) == (n >= 512)
    assert all(w.dtype == np.float32 and w.ndim == 1 and len(w) >= 1 for _, w, _ in ROWS)
    lens = [len(w) for _, w, _ in ROWS]
    assert max(lens) == ref.U128_N and sum(lens) < 300000
    assert not BY_NAME["zeros_tile_513"][0][256:512].any() and BY_NAME["zeros_tile_513"][0][-1] == 1
    assert sum(1 for _, _, regular in ROWS if not regular) == 12


def test_oracle_tables_on_the_boundary_rows(oracle):
    """every row: regular as named; every regular row: well formed and implied_error <= 1 (the 32 768-entry rows cost about 0.1 s each)"""
    worst = ("", 0.0)
    for name, w, regular in ROWS:
        reg, prob, alias = oracle.alias_row(w)
        assert reg == int(regular), name
        if regular:
            assert ref.table_is_well_formed(prob, alias), name
            e = ref.implied_error(w, prob, alias)
            assert e <= 1, (name, float(e))
            worst = max(worst, (name, float(e)), key=lambda x: x[1])
    print("worst implied error / bound: %.6f on %s" % (worst[1], worst[0]))
    assert worst[1] > 0.5             # the bound is tight, not loose: some row comes within a factor of two of it


def test_implied_error_notices_a_wrong_table(oracle):
    w = BY_NAME["rand_257"][0]
    _, prob, alias = oracle.alias_row(w)
    assert ref.implied_error(w, prob, alias) <= 1
    k = int(np.nonzero((alias != np.arange(len(w))) & (prob < 0.9) & (np.bincount(alias, minlength=len(w)) == 0))[0][0])
    bad = prob.copy(); bad[k] += np.float32(2.0 ** -22)           # eight roundings' worth on a slot nothing aliases to: bound 2^-25 / n
    assert 6 < ref.implied_error(w, bad, alias) < 10
    other = alias.copy(); other[k] = (alias[k] + 1) % len(w)
    assert ref.implied_error(w, prob, other) > 1
    assert not ref.table_is_well_formed(prob, np.where(np.arange(len(w)) == k, len(w), alias))


def test_uniform_rows_are_trivial(oracle):
    for n in ref.LENGTHS + (ref.U128_N,):
        reg, prob, alias = oracle.alias_row(np.full(n, 2.5, np.float32))
        assert reg == 1 and (prob == 1).all() and np.array_equal(alias, np.arange(n)), n


# ---- conditions on the GPU file's inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u128_split", "u128_interleaved", "u128_rand"])
def test_u128_rows_carry_into_the_high_word(name):
    w, regular = BY_NAME[name]
    D, E, L, H = ref.deficit_excess_prefixes(w)
    assert regular and ref.certificate(w) == 29 and len(w) == ref.U128_N > 2048
    assert D[-1] > 2 ** 64 and D[-1] == E[-1]                     # total deficit = total excess, beyond one 64-bit word
    assert sum(1 for x in D if x >> 64) > len(D) // 2             # and most prefixes already are
    assert len(L) == len(H) == ref.U128_N // 2


def test_tie_rows_tie():
    """slots where a heavy's excess prefix equals a light's deficit prefix: the `<=` of both binary searches decides there"""
    for n in ref.LENGTHS:
        D, E, L, H = ref.deficit_excess_prefixes(BY_NAME["tie3113_%d" % n][0])
        ties = len(set(D) & set(E))
        assert (ties > 0) == (n >= 2), n
        if n >= 4:
            assert ties > 0
        if n % 4 == 0:
            assert ties == n // 2 and D == E, n                   # every prefix ties: every heavy keeps T


def test_split_rows_have_tiles_without_lights_or_heavies():
    for n in ref.LENGTHS:
        for split in (256, 257):
            if n > split:
                for pat, first_light in (("lights_then_heavies", True), ("heavies_then_lights", False)):
                    D, E, L, H = ref.deficit_excess_prefixes(BY_NAME["%s_%d_%d" % (pat, split, n)][0])
                    assert (L if first_light else H) == list(range(split)), (pat, split, n)
                    assert (H if first_light else L) == list(range(split, n)), (pat, split, n)


def test_certificate_pairs():
    for name, c in (("cert_2_29", 29), ("cert_2_30", 30), ("cert_2048_29", 29), ("cert_2049_30", 30), ("cert_2049_29", 29), ("subnormal", 7)):
        w, regular = BY_NAME[name]
        assert ref.certificate(w) == c and regular == (c <= 29), name
    assert len(BY_NAME["cert_2048_29"][0]) == 2048 and len(BY_NAME["cert_2049_30"][0]) == 2049
    sub = BY_NAME["subnormal"][0].view(np.uint32)
    assert ((sub[:2] >> 23) == 0).all() and (sub[:2] != 0).all() and (sub[2] >> 23) == 1     # two subnormals and the smallest normal


def test_walk_edge_graphs_meet_their_conditions(oracle):
    G = ref.walk_edge_graphs()
    # e. parallel groups whose float64 sum is a float32, and groups whose sum is not
    sums = ref.parallel_groups(*G["multi"][:3])
    exact = {k for k, t in sums.items() if float(np.float32(t)) == t}
    assert {(0, 1), (1, 2), (4, 4)} <= exact and {(2, 3), (3, 4)} <= set(sums) - exact
    s, d = G["multi"][0].tolist(), G["multi"][1].tolist()
    assert (4, 5) in zip(s, d) and (5, 4) in zip(s, d)
    # every row of every graph is alias-regular: the walks below go through the tables, not through the fallback
    for name, (s, d, w, directed) in G.items():
        g = oracle.Graph.from_coo(s, d, w, directed=directed)
        assert all(g.alias_row(int(v))[0] == 1 for v in g.vertices() if g.degree(int(v)) > 0), name
    # the directed graph without return weight: b -> a weighs 0 or is absent
    nb = ref.adjacency(*G["noreturn"])
    for a, b, back in ((0, 1, 0.0), (2, 3, 0.0), (4, 5, None), (6, 7, None)):
        assert b in nb[a][0]
        assert (nb[b][1][nb[b][0] == a].tolist() == [back] * int((nb[b][0] == a).sum())) and ((a in nb[b][0]) == (back is not None))
    # f. the hub: both orders of (candidate's degree, previous degree), both answers
    nb = ref.adjacency(*G["hub"])
    deg = {v: len(r[0]) for v, r in nb.items()}
    assert deg[0] == ref.HUB_N and all(deg[v] == 2 for v in range(1, ref.HUB_N + 1))
    assert 2 in nb[1][0] and 0 in nb[2][0]                             # hub -> leaf 1 -> leaf 2: shorter row is the candidate's, answer yes
    assert deg[ref.HUB_N + 1] < ref.HUB_N and 0 not in nb[ref.HUB_N + 1][0] and ref.HUB_N + 1 in nb[2001][0]   # ... answer no
    assert 3 not in nb[1][0] and 2 in nb[1][0]                         # leaf 1 -> hub -> leaf 3 / leaf 2: N(prev) searched, no / yes


def test_staging_graph_stops_walkers_at_every_length(oracle):
    s, d, w, directed = ref.walk_edge_graphs()["staging"]
    g = oracle.Graph.from_coo(s, d, w, directed=directed)
    assert g.num_vertices * ref.STAGING_NUM_WALKS >= 3 * 256 + 1
    for p, q in ref.STAGING_PQ:
        lens = g.walk(p=p, q=q, sampler=1, walk_length=max(ref.STAGING_L), num_walks=ref.STAGING_NUM_WALKS, seed=5)[1]
        assert set(range(1, max(ref.STAGING_L) + 3)) <= set(lens.tolist()), (p, q)


# ---- the walk's distribution against the restatement ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stat_walks(oracle):
    """{(directed, p, q): observed triples of the oracle's Mode A walk} — computed once"""
    s, d, w = ref.stat_graph()
    out = {}
    for directed in (False, True):
        g = oracle.Graph.from_coo(s, d, w, directed=directed)
        nb = ref.adjacency(s, d, w, directed)
        for v in g.vertices():                                       # the restatement reads the rows the oracle walks
            ids, ws = g.neighbors(int(v))
            assert np.array_equal(ids, nb[int(v)][0]) and np.array_equal(ws, nb[int(v)][1])
            assert len(ids) == 0 or g.alias_row(int(v))[0] == 1
        for p, q in ref.STAT_PQ:
            paths = g.walk(p=p, q=q, sampler=1, threads=oracle.threads(), **ref.STAT_KW)[0]
            out[(directed, p, q)] = ref.triple_counts(paths)
    return out


def test_stat_graph_is_what_the_test_needs():
    s, d, w = ref.stat_graph()
    assert s.dtype == d.dtype == np.int32 and w.dtype == np.float32 and len(s) == 60
    assert (s == d).any()
    sums = ref.parallel_groups(s, d, w)
    assert any(float(np.float32(t)) != t for t in sums.values()) and any(float(np.float32(t)) == t for t in sums.values())
    assert len(ref.transition_probabilities(ref.adjacency(s, d, w, False), 1.0, 1.0)) == 400
    assert len(ref.transition_probabilities(ref.adjacency(s, d, w, True), 1.0, 1.0)) == 119


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("p,q", ref.STAT_PQ)
def test_oracle_walk_has_the_stated_distribution(stat_walks, directed, p, q):
    nb = ref.adjacency(*ref.stat_graph(), directed)
    obs = stat_walks[(directed, p, q)]
    z, dof, left = ref.chi_z(obs, ref.transition_probabilities(nb, p, q, "exact"), ref.STAT_KW["num_walks"])
    print("directed %d p %g q %g: z = %.2f, dof %d, %.1f %% of cells left out" % (directed, p, q, z, dof, 100 * left))
    assert abs(z) <= 5 and left <= 0.10
    for model in ref.MODELS[1:]:
        zm, _, _ = ref.chi_z(obs, ref.transition_probabilities(nb, p, q, model), ref.STAT_KW["num_walks"])
        print("    %s: z = %.0f" % (model, zm))
        if ref.model_differs(model, p, q):
            assert zm > 100, (model, zm)          # measured: 900 and more; the condition comes from nothing finer than that gap
        else:
            assert zm == z, model


# ---- the trial cap -----------------------------------------------------------------------------------------------------------------
CAP_GOLDEN = [[0, 1, 0, 1, 2, 1, 2, 1, 2], [1, 2, 3, 2, 1, 0, 1, 2, 3], [2, 1, 2, 1, 2, 1, 2, 1, 2],
              [3, 4, 3, 4, 3, 4, 3, 4, 3], [4, 3, 4, 3, 4, 3, 4, 3, 2], [0, 1, 2, 1, 2, 1, 2, 1, 2]]


def test_oracle_trial_cap(oracle):
    """p = q = 2^20 on a path: a second-order trial is accepted with probability 2^-20, so nearly every step runs its 65 536 trials and
    falls through with the last candidate.  The rows are complete, the first six are pinned, and a replay of the loop from the
    specification (mode_a_ref.cap_walk) gives every row and the number of trials."""
    s, d, w, directed = ref.walk_edge_graphs()["cap"]
    g = oracle.Graph.from_coo(s, d, w, directed=directed)
    paths, lens, steps = g.walk(sampler=1, **ref.CAP_KW)
    assert paths.shape == (15, 9) and (lens == 9).all() and steps == 15 * 8
    assert paths[:6].tolist() == CAP_GOLDEN
    tables = {int(v): g.alias_row(int(v))[1:] for v in g.vertices()}
    rp, trials = ref.cap_walk(ref.adjacency(s, d, w, directed), tables, **ref.CAP_KW)
    assert np.array_equal(rp, paths)
    capped = (trials - 15) // 65536                                # second-order steps that ran into the cap
    print("trials %d: %d of %d second-order steps ran all 65 536" % (trials, capped, 15 * 7))
    # a step escapes the cap with probability 1 - (1 - 2^-20)^65536 = 6 %: most of the 105 must have run into it
    assert capped > 15 * 7 // 2 and trials >= 65536 * capped + 15
