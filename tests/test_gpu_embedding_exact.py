"""The embedding trainer on the GPU against the float64 restatement (tests/w2v_ref.py), and exact statements about the Hogwild launch.

Sequential mode (threads = 1): every element of the vectors within the case's T of ref64.  T = 8 * noise, noise = the largest
distance of two float32 restatements to ref64, measured on the CPU (tests/test_w2v_ref_cpu.py holds T within the tolerance the suite
had before and every wrong trainer of w2v_ref.MUTANTS at least 4 * T away).  The cases: every instantiation of k_w2v_train_rows and
the dims on either side of a lane boundary; windows on either side of the switch between window tokens in a register and from
memory (2 * W + 1 <= 64); codes longer than the register rows at R = 8 and R = 4, visited often, and groups of every fill; token
patterns in hand-made sentences; a learning rate that reaches the |f| < 6 gate; the device-resident walk; and k_w2v_train, the
kernel behind SRW_W2V_ROWS_IN_MEMORY=1, in a child process (the switch is read once per process).

Hogwild mode (threads = 0): no tolerance fits a race, so only what must hold EXACTLY: one sentence, or one trained sentence among
100 000 empty ones, gives the sequential mode's bits wherever it sits; sentences without a pair leave the initial vectors; and of
70 000 sentences with vocabularies of their own every one is trained."""
import os
import subprocess
import sys

import numpy as np
import pytest

import w2v_ref
from helpers import pkg

pytestmark = pytest.mark.gpu
CASES = list(w2v_ref.cases())
ROWS_IN_MEMORY_CASES = ("karate-d16-w5", "fib13x8-d300", "fib9x16-d600")


@pytest.fixture(scope="module")
def eng():
    e = pkg().Engine(device=0)
    yield e
    e.close()


def _hold(name, ids, vec, what="sequential"):
    r64, noise, T = w2v_ref.footing(name)
    assert np.array_equal(ids, r64.ids)
    worst = float(np.abs(vec.astype(np.float64) - r64.vectors).max())
    print("%s [%s]: noise %.3g T %.3g worst |got - want| / T = %.3f" % (name, what, noise, T, worst / T))
    assert np.isfinite(vec).all() and worst <= T, (name, worst, T)


def _fit(e, c, **kw):
    return e.w2v_fit(c.paths, c.lens, dim=c.dim, window=c.window, iterations=c.iterations, lr=c.lr, seed=c.seed, **kw)


# ---- the sequential mode against ref64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_sequential_mode_within_T_of_float64(eng, name):
    ids, vec = _fit(eng, w2v_ref.cases()[name], threads=1)
    _hold(name, ids, vec)


def test_fit_device_on_the_resident_walk_within_T_of_float64(eng):
    name = "lanes-d129"
    c = w2v_ref.cases()[name]
    eng.load_edgelist(w2v_ref.KARATE, directed=False)
    paths, lens, _ = eng.walk(p=0.5, q=2.0, walk_length=12, num_walks=2, seed=3)
    assert np.array_equal(paths, c.paths) and np.array_equal(lens, c.lens)      # the walk the case took through the oracle
    ids, vec = eng.w2v_fit_device(dim=c.dim, window=c.window, iterations=c.iterations, lr=c.lr, seed=c.seed, threads=1)
    _hold(name, ids, vec, "w2v_fit_device")


_CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import w2v_ref
from helpers import pkg
out = {}
with pkg().Engine(device=0) as e:
    for name in sys.argv[2:]:
        c = w2v_ref.cases()[name]
        ids, vec = e.w2v_fit(c.paths, c.lens, dim=c.dim, window=c.window, iterations=c.iterations, lr=c.lr, seed=c.seed, threads=1)
        out[name + ":ids"], out[name + ":vec"] = ids, vec
np.savez(sys.argv[1], **out)
"""


def test_rows_in_memory_kernel_within_T_of_float64(eng, tmp_path):
    """k_w2v_train<ND> (SRW_W2V_ROWS_IN_MEMORY=1, tools/SWITCHES.md): every (context, node) pair through memory."""
    out = str(tmp_path / "rows_in_memory.npz")
    code = _CHILD % (os.path.join(w2v_ref.ROOT, "tests"), os.path.join(w2v_ref.ROOT, "oracle"), w2v_ref.ROOT)
    r = subprocess.run([sys.executable, "-c", code, out, *ROWS_IN_MEMORY_CASES], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, SRW_W2V_ROWS_IN_MEMORY="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    same = []
    for name in ROWS_IN_MEMORY_CASES:
        _hold(name, got[name + ":ids"], got[name + ":vec"], "k_w2v_train")
        same.append(bool(np.array_equal(_fit(eng, w2v_ref.cases()[name], threads=1)[1], got[name + ":vec"])))
    # f feeds nothing but its table index: the two kernels' bits part only where their summation orders put an f in different bins
    print("bit-identical to k_w2v_train_rows:", dict(zip(ROWS_IN_MEMORY_CASES, same)))


# ---- the Hogwild launch: exact statements -----------------------------------------------------------------------------------------
def _one_sentence(n_tokens, n_words, seed):
    return [int(x) + 10 for x in np.random.default_rng(seed).integers(0, n_words, n_tokens)]


@pytest.mark.parametrize("dim", [16, 128, 200, 300, 600])
def test_hogwild_one_sentence_is_the_sequential_mode(eng, dim):
    """One sentence: one wave has work.  The launch differs (a block of 256 threads, not 64): the bits may not."""
    paths, lens = w2v_ref.pack([_one_sentence(300, 40, dim)], stride=310)
    kw = dict(dim=dim, window=5, iterations=2, lr=0.05, seed=9)
    ids1, seq = eng.w2v_fit(paths, lens, threads=1, **kw)
    ids0, hog = eng.w2v_fit(paths, lens, threads=0, **kw)
    _, v0 = eng.w2v_fit(paths, lens, dim=dim, window=5, iterations=0, seed=9)
    assert np.array_equal(ids0, ids1) and np.array_equal(hog, seq)
    assert float(np.abs(seq - v0).max()) > 1e-3                                # (and it trained)


@pytest.mark.parametrize("at", [0, 1, 255, 256, 65537, 99999])
def test_hogwild_one_trained_sentence_among_empty_ones(eng, at):
    """100 000 sentences, all empty but one: whichever wave of whichever block takes it, in the first round over the sentences or a
    later one (s += n_waves), with the window draws and the learning rate of sentence `at` — the sequential mode's bits.  The
    fillers are EMPTY: a sentence of one word has a position without a context, and that position still writes its centre word's
    rows of syn1 back as it read them, which may overwrite what the trained sentence's wave wrote in between
    (docs/embedding_stage.md, "Why the fillers are empty")."""
    n = 100000
    sent = _one_sentence(60, 12, 4)
    paths = np.full((n, 64), -1, np.int32); lens = np.zeros(n, np.int32)
    paths[at, : len(sent)] = sent; lens[at] = len(sent)
    kw = dict(dim=32, window=4, iterations=2, lr=0.05, seed=9)
    ids1, seq = eng.w2v_fit(paths, lens, threads=1, **kw)
    ids0, hog = eng.w2v_fit(paths, lens, threads=0, **kw)
    _, v0 = eng.w2v_fit(paths, lens, dim=32, window=4, iterations=0, seed=9)
    assert len(ids1) == 12 and np.array_equal(ids0, ids1) and np.array_equal(hog, seq)
    assert float(np.abs(seq - v0).max()) > 1e-3
    if at == 0:                                    # the sentence alone, as sentence 0: the fillers change nothing
        _, alone = eng.w2v_fit(paths[:1], lens[:1], threads=1, **kw)
        assert np.array_equal(alone, seq)


def test_sentences_without_a_pair_train_nothing(eng):
    rng = np.random.default_rng(8)
    n = 3000
    paths = np.full((n, 3), -1, np.int32)
    paths[:, 0] = rng.integers(0, 50, n)
    lens = rng.integers(0, 2, n).astype(np.int32)
    paths[lens == 0, 0] = -1
    i0, v0 = eng.w2v_fit(paths, lens, dim=24, window=3, iterations=0, seed=6)
    assert len(i0) == 50
    for threads in (1, 0):
        ids, vec = eng.w2v_fit(paths, lens, dim=24, window=3, iterations=2, lr=0.05, seed=6, threads=threads)
        assert np.array_equal(ids, i0) and np.array_equal(vec, v0), threads


def test_hogwild_trains_every_sentence(eng):
    """70 000 sentences [a, b, a, b], every one with two words of its own: a sentence no wave took leaves its two rows untouched."""
    n, base = 70000, 1000
    a = base + 2 * np.arange(n, dtype=np.int32)
    paths = np.stack([a, a + 1, a, a + 1], axis=1).astype(np.int32)
    lens = np.full(n, 4, np.int32)
    # all counts are equal: CreateBinaryTree joins the leaves pairwise, from the vocabulary's end, before it joins any inner node — so
    # the last node of words 2s and 2s + 1 is theirs alone, and what sentence s writes there no other sentence reads or writes
    tree = pkg().w2v_huffman(np.full(2 * n, 2, np.int64))
    last = np.array([p[-1] for _, p in tree])
    upper = {x for _, p in tree for x in p[:-1]}
    assert np.array_equal(last[0::2], last[1::2]) and len(set(last[0::2].tolist())) == n and not upper & set(last.tolist())
    kw = dict(dim=8, window=1, seed=3)
    i0, v0 = eng.w2v_fit(paths, lens, iterations=0, **kw)
    ids, vec = eng.w2v_fit(paths, lens, iterations=1, lr=0.025, threads=0, **kw)
    assert np.array_equal(ids, i0) and np.array_equal(ids, base + np.arange(2 * n)) and np.isfinite(vec).all()
    untouched = np.flatnonzero((vec == v0).all(axis=1))
    assert len(untouched) == 0, (len(untouched), ids[untouched[:10]])
