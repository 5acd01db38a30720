"""The footing of tests/test_gpu_embedding_exact.py, on the CPU: the float64 restatement of the trainer (tests/w2v_ref.py) against
the answers worked out by hand in test_w2v_known_answers.py, and the tolerance the GPU is held to.

Per shared case: noise = the largest distance, over all elements, of the two float32 restatements (the oracle's C, summing left to
right; w2v_ref in wave order) to ref64, and T = 8 * noise.  Two float32 summation orders lie apart by a small multiple of either one's
distance to float64, and the GPU's order is a third; 8 leaves it room.  T is a margin over the REFERENCE's error, measured here and
nowhere taken from a kernel: it must stay within the relative tolerance the suite held before (2e-3 of the vectors' scale), and every
wrong trainer a case is held against (w2v_ref.MUTANTS) must move some element by at least 4 * T."""
import numpy as np
import pytest

import w2v_ref
from helpers import pkg
from test_w2v_known_answers import HAND_TREE

CASES = list(w2v_ref.cases())


# ---- ref64 against the hand-worked answers ------------------------------------------------------------------------------------------
def test_trees_by_hand():
    assert w2v_ref.huffman([5, 4, 3, 2, 1]) == HAND_TREE
    assert w2v_ref.huffman([7, 3]) == [([1], [0]), ([0], [0])]
    assert w2v_ref.huffman([1, 1, 1, 1]) == [([1, 1], [2, 1]), ([1, 0], [2, 1]), ([0, 1], [2, 0]), ([0, 0], [2, 0])]


def test_trees_equal_the_product_and_the_oracle(oracle):
    rng = np.random.default_rng(5)
    for V in (3, 17, 1000):
        cn = np.sort(rng.integers(1, 50, V))[::-1].copy()
        t = w2v_ref.huffman(cn)
        assert t == pkg().w2v_huffman(cn) and t == oracle.w2v_huffman(cn)
    cn = np.maximum(1, (1e6 / np.arange(1, 5001) ** 1.2).astype(np.int64))
    t = w2v_ref.huffman(cn)
    assert t == pkg().w2v_huffman(cn) and t == oracle.w2v_huffman(cn) and max(len(c) for c, _ in t) >= 15
    for name in CASES:                             # and the trees the shared cases train on
        _, counts, _ = w2v_ref.vocabulary(w2v_ref.cases()[name].paths, w2v_ref.cases()[name].lens)
        assert w2v_ref.huffman(counts) == pkg().w2v_huffman(counts), name


def test_table_and_draws_equal_the_oracle(oracle):
    assert np.array_equal(w2v_ref.exp_table(), oracle.w2v_exp_table())
    assert w2v_ref.exp_table().dtype == np.float32


def test_one_pair_by_hand():
    """test_w2v_known_answers.py::test_one_pair_update_by_hand, in float64: index 495, g = -0.01212511."""
    table = w2v_ref.exp_table()
    r0, R1 = np.array([0.1, -0.2]), np.array([[0.3, 0.4]])
    n0, n1, ind = w2v_ref.pair_update(r0, R1, np.array([1.0]), 0.025, table)
    assert ind.tolist() == [495]
    assert np.allclose(n0, [0.09636247, -0.20485004], rtol=0, atol=1e-7) and np.allclose(n1, [[0.29878749, 0.40242502]], rtol=0, atol=1e-7)
    # two nodes: both f from the ORIGINAL r0 (indices 520 and 531), neu from the OLD rows
    r0, R1 = np.array([0.5, 0.25]), np.array([[1.0, -1.0], [0.5, 0.5]])
    n0, n1, ind = w2v_ref.pair_update(r0, R1, np.array([0.0, 1.0]), np.float32(0.1), table)
    assert ind.tolist() == [520, 531]
    g = [(1.0 - 0.0 - float(table[520])) * float(np.float32(0.1)), (1.0 - 1.0 - float(table[531])) * float(np.float32(0.1))]
    assert np.allclose(n0, r0 + g[0] * R1[0] + g[1] * R1[1], rtol=0, atol=1e-12)
    assert np.allclose(n1, [R1[0] + g[0] * r0, R1[1] + g[1] * r0], rtol=0, atol=1e-12)
    # |f| >= 6: the node is skipped
    n0, n1, ind = w2v_ref.pair_update(np.array([4.0, 0.0]), np.array([[2.0, 0.0]]), np.array([1.0]), 0.025, table)
    assert ind.tolist() == [-1] and n0.tolist() == [4.0, 0.0] and n1.tolist() == [[2.0, 0.0]]


def test_one_pair_equals_the_oracle_in_float32(oracle):
    rng = np.random.default_rng(3)
    table = w2v_ref.exp_table()
    for dim, n in ((2, 1), (16, 5), (70, 12)):
        r0 = rng.uniform(-1, 1, dim).astype(np.float32); R1 = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        bits = rng.integers(0, 2, n)
        o0, o1 = oracle.w2v_pair_update(r0, R1, bits, 0.05)
        n0, n1, _ = w2v_ref.pair_update(r0.astype(np.float64), R1.astype(np.float64), bits.astype(np.float64), np.float32(0.05), table)
        assert np.allclose(o0, n0, rtol=0, atol=1e-5) and np.allclose(o1, n1, rtol=0, atol=1e-5)


# ---- iterations = 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["karate-d16-w5", "lanes-d513", "tokens-d16"])
def test_initial_vectors_bit_for_bit(oracle, name):
    c = w2v_ref.cases()[name]
    r = w2v_ref.fit(c.paths, c.lens, c.dim, c.window, 0, c.lr, c.seed, dtype=np.float32)
    oids, ovec = oracle.w2v_fit(c.paths, c.lens, dim=c.dim, window=c.window, iterations=0, lr=c.lr, seed=c.seed)
    assert np.array_equal(r.ids, oids) and np.array_equal(r.vectors.astype(np.float32), ovec) and len(r.indices) == 0


# ---- the tolerance and what it separates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_tolerance_and_mutants(name):
    c = w2v_ref.cases()[name]
    assert int(c.lens.sum()) <= 5000
    r64, noise, T = w2v_ref.footing(name)
    scale = float(np.abs(r64.vectors).max())
    effects = {}
    for m in c.mutants:
        v = w2v_ref.run(c, mutate=m, reg_rows=w2v_ref.reg_rows_of(c.dim)).vectors
        effects[m] = float(np.abs(v - r64.vectors).max()) / T
    print("%s: tokens %d noise %.3g T %.3g T/scale %.3g smallest mutant/T %s %s" % (
        name, int(c.lens.sum()), noise, T, T / scale, "%.1f" % min(effects.values()) if effects else "-",
        " ".join("%s=%.1f" % kv for kv in effects.items())))
    assert 0.0 < T <= 2e-3 * scale, (T, scale)
    for m, e in effects.items():
        assert e >= 4.0, (m, e)


def test_every_mutant_is_held_by_some_case():
    held = {m for c in w2v_ref.cases().values() for m in c.mutants}
    assert held == set(w2v_ref.MUTANTS)
    # the tail mutants at both register depths a small vocabulary can reach: 8 rows (dim 257 .. 512) and 4 (dim 513 .. 1024)
    assert {w2v_ref.reg_rows_of(c.dim) for c in w2v_ref.cases().values() if "tail_last" in c.mutants} == {8, 4}


def test_the_tail_cases_reach_the_tail():
    """Codes longer than the register rows, visited often; in the residue cases every length mod 4 on both sides of the rows."""
    for name, c in w2v_ref.cases().items():
        if "tail_last" not in c.mutants:
            continue
        R = w2v_ref.reg_rows_of(c.dim)
        _, counts, _ = w2v_ref.vocabulary(c.paths, c.lens)
        n = np.array([len(code) for code, _ in w2v_ref.huffman(counts)])
        assert n.max() > R and counts[n > R].sum() >= 50, name
        if name.startswith("residues"):
            assert {int(x) % 4 for x in n[n <= R]} == {0, 1, 2, 3} and {int(x) % 4 for x in n[n > R]} == {0, 1, 2, 3}, name


def test_the_gate_case_reaches_the_gate():
    r64, noise, T = w2v_ref.footing("gate-d16")
    ev = r64.indices[r64.indices >= 0]
    print("gate-d16: %d of %d nodes gated out, %d bins, indices %d .. %d" % (r64.gated, len(r64.indices), len(np.unique(ev)), ev.min(), ev.max()))
    assert r64.gated >= 20 and len(np.unique(ev)) >= 300
    assert ev.min() < 10 and ev.max() >= 990       # both ends of the table
    assert T <= 2e-3 * float(np.abs(r64.vectors).max())
