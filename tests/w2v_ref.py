"""The embedding trainer (csrc/embedding.hip) restated in numpy, and the inputs the tests built on it share.

Written from the header comment of embedding.hip and include/stellar_rw.h: skip-gram with hierarchical softmax over sentences of
vocabulary indices, ONE logical partition, sentences and positions in order (the sequential mode, threads == 1).

  vocabulary      every distinct token, by descending count, ties by ascending id
  tree            word2vec.c's CreateBinaryTree over those counts: per word the inner nodes from the root down (rows of syn1, the root
                  is row V - 2) and one code bit per node
  table           1 000 entries over [-6, 6): e = float32(exp(double)), entry = e / (e + 1) in float32
  draws           h(seed, a, b, c), a 32-bit mix; syn0[r][j] = ((h(seed, 0xA11CE, r, j) >> 8) / 2^24 - 0.5) / dim in float32, syn1 = 0;
                  the window shrink of (iteration k, sentence s, position pos) is b = h(seed, k, s, pos) % window
  learning rate   per sentence, in double: lr * (1 - (k * total + words_before[s]) / (iterations * total + 1)), not below lr * 1e-4,
                  rounded to float32
  one position    for a in b .. 2 * window - b, a != window, c = pos - window + a inside the sentence: the pair (centre = sent[pos],
                  context = sent[c]).  r0 = syn0[context]; for every node d of the CENTRE's code: f = r0 . syn1[d]; if |f| < 6:
                  index = trunc((f + 6) * (1000 / 12)), g = (1 - bit_d - table[index]) * alpha, neu += g * syn1[d] (the OLD row),
                  syn1[d] += g * r0.  After the pair's nodes: syn0[context] = r0 + neu.

The nodes of one pair do not depend on each other (r0 changes after them, every node has its own row), so a pair is one batch of
numpy operations over its nodes; neu is summed over the nodes in their order.  `dtype` is the type of syn0, syn1, f, g and the
updates; with float32, `order="wave"` sums a dot product the way a 64-lane wave can: every lane its elements lane + 64 * i in turn,
then a six-step butterfly across the lanes — a second float32 order beside the left-to-right one of oracle/srw_oracle.c.

`mutate` names ONE wrong trainer (tests/test_w2v_ref_cpu.py measures how far each moves the vectors):
  tail_last       the last node of a code longer than reg_rows gets g = 0
  group_partial   the last node of a code whose length is no multiple of 4, and <= reg_rows, gets g = 0
  stale_repeat    a context word equal to the previous context word of the same position uses the row as it was read for that
                  previous pair (and writes its update on top of that)
  alpha_late      the learning rate of sentence s from words_before[s + 1]
  index_round     the table index rounded to nearest
  window_last     b = 0 at a sentence's last position
"""
import collections
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KARATE = os.path.join(ROOT, "tests", "golden", "karate.txt")

EXP_TABLE_SIZE = 1000
MAX_EXP = 6.0
MAX_CODE_LENGTH = 40
MUTANTS = ("tail_last", "group_partial", "stale_repeat", "alpha_late", "index_round", "window_last")

Fit = collections.namedtuple("Fit", "ids vectors indices gated")


# ---- the pieces ---------------------------------------------------------------------------------------------------------------------
def w2v_hash(seed, a, b, c):
    """The build's seeded draw, elementwise over uint32 arrays (or scalars)."""
    u = np.uint32
    a, b, c = (np.asarray(x).astype(np.uint32) for x in (a, b, c))
    with np.errstate(over="ignore"):
        h = np.asarray(u(seed) ^ u(0x9E3779B9), dtype=np.uint32)
        h = h ^ (a + u(0x7F4A7C15) + (h << u(6)) + (h >> u(2))); h = h * u(0x85EBCA6B); h = h ^ (h >> u(13))
        h = h ^ (b + u(0x165667B1) + (h << u(6)) + (h >> u(2))); h = h * u(0xC2B2AE35); h = h ^ (h >> u(16))
        h = h ^ (c + u(0x27D4EB2F) + (h << u(6)) + (h >> u(2))); h = h * u(0x9E3779B1); h = h ^ (h >> u(15))
    return h


def vocabulary(paths, lens):
    """(ids by descending count, ties by ascending id; their counts; the sentences as lists of vocabulary indices)."""
    paths = np.asarray(paths, dtype=np.int32); lens = np.asarray(lens, dtype=np.int64)
    rows = [paths[i, : lens[i]] for i in range(len(lens))]
    flat = np.concatenate(rows) if rows else np.zeros(0, np.int32)
    ids, counts = np.unique(flat, return_counts=True)
    order = np.lexsort((ids, -counts))
    ids, counts = ids[order].astype(np.int32), counts[order].astype(np.int64)
    rank = {int(v): r for r, v in enumerate(ids)}
    sents = [np.array([rank[int(t)] for t in row], dtype=np.int64) for row in rows]
    return ids, counts, sents


def huffman(counts):
    """CreateBinaryTree over counts in descending order: per word (code bits, rows of syn1), both from the root down."""
    cn = [int(x) for x in counts]
    V = len(cn)
    if V < 2:
        return [([], []) for _ in range(V)]
    count = cn + [10 ** 15] * (V + 1)
    parent = [0] * (2 * V + 1)
    binary = [0] * (2 * V + 1)
    pos1, pos2 = V - 1, V
    for a in range(V - 1):
        two = []
        for _ in range(2):                         # the two smallest of: the leaves not taken yet (from the rare end), the inner nodes
            if pos1 >= 0 and count[pos1] < count[pos2]:
                two.append(pos1); pos1 -= 1
            else:
                two.append(pos2); pos2 += 1
        count[V + a] = count[two[0]] + count[two[1]]
        parent[two[0]] = parent[two[1]] = V + a
        binary[two[1]] = 1
    out = []
    for w in range(V):
        bits, nodes, b = [], [], w
        while True:
            if len(bits) >= MAX_CODE_LENGTH:
                raise ValueError("a Huffman code exceeds 40 bits")
            bits.append(binary[b]); nodes.append(b)
            b = parent[b]
            if b == 2 * V - 2:
                break
        # bits[k] is the branch taken INTO nodes[k]; read from the root: the root's own row first, then the inner nodes below it
        out.append((bits[::-1], [V - 2] + [n - V for n in nodes[:0:-1]]))
    return out


def exp_table():
    """The 1 000 float32 entries, computed as the kernel computes them."""
    x = (np.arange(EXP_TABLE_SIZE, dtype=np.float64) / EXP_TABLE_SIZE * 2.0 - 1.0) * MAX_EXP
    e = np.exp(x).astype(np.float32)
    return e / (e + np.float32(1.0))


def initial_vectors(V, dim, seed):
    r, j = np.meshgrid(np.arange(V, dtype=np.uint32), np.arange(dim, dtype=np.uint32), indexing="ij")
    h = w2v_hash(seed, 0xA11CE, r, j)
    return ((h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) - np.float32(0.5)) / np.float32(dim)


def learning_rate(lr, k, iterations, total, words_before):
    lr = float(np.float32(lr))
    a = lr * (1.0 - (float(k) * float(total) + float(words_before)) / (float(iterations) * float(total) + 1.0))
    return np.float32(max(a, lr * 0.0001))


def _dots(R1, r0, order):
    if order == "dot":
        return R1 @ r0
    n, D = R1.shape
    nd = (D + 63) // 64
    p = np.zeros((n, nd * 64), R1.dtype)
    p[:, :D] = R1 * r0
    p = p.reshape(n, nd, 64)
    v = p[:, 0, :].copy()
    for i in range(1, nd):                         # lane l: its elements l + 64 * i, in turn
        v += p[:, i, :]
    w = 32
    while w >= 1:                                  # v[l] += v[l ^ w]: what lane 0 ends up with
        v = v[:, :w] + v[:, w:2 * w]
        w >>= 1
    return v[:, 0]


def pair_update(r0, R1, bits, alpha, table, order="dot", index_round=False, kill=None):
    """One (centre, context) pair: r0 the context's row of syn0, R1 [n, dim] the centre's node rows, bits [n] in R1's dtype.
    Returns (new r0, new R1, table index per node or -1)."""
    dt = R1.dtype.type
    f = _dots(R1, r0, order)
    ok = (f > dt(-MAX_EXP)) & (f < dt(MAX_EXP))
    x = (np.where(ok, f, dt(0)) + dt(MAX_EXP)) * (dt(EXP_TABLE_SIZE) / dt(MAX_EXP) / dt(2.0))
    ind = np.minimum(np.floor(x + dt(0.5)), EXP_TABLE_SIZE - 1).astype(np.int64) if index_round else x.astype(np.int64)
    g = np.where(ok, (dt(1.0) - bits - table[ind].astype(dt)) * dt(alpha), dt(0)).astype(dt)
    if kill is not None:
        g[kill] = 0
    neu = (g[:, None] * R1).sum(axis=0)            # over the nodes in their order, every g with the OLD row
    return r0 + neu, R1 + g[:, None] * r0, np.where(ok, ind, -1)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def fit(paths, lens, dim, window, iterations, lr, seed, dtype=np.float64, order="dot", mutate=None, reg_rows=None):
    """-> Fit(ids, vectors float64 [V, dim], table index of every evaluated node in evaluation order (-1: gated out), gated nodes)."""
    if mutate is not None and mutate not in MUTANTS:
        raise ValueError(mutate)
    if mutate in ("tail_last", "group_partial") and reg_rows is None:
        raise ValueError("%s needs reg_rows" % mutate)
    dt = np.dtype(dtype).type
    ids, counts, sents = vocabulary(paths, lens)
    V = len(ids)
    syn0 = initial_vectors(V, dim, seed).astype(dt)
    indices = []
    if V >= 2 and iterations > 0:
        tree = huffman(counts)
        bits = [np.array(c, dtype=dt) for c, _ in tree]
        nodes = [np.array(p, dtype=np.int64) for _, p in tree]
        kill = [None] * V
        for w in range(V):
            n = len(nodes[w])
            if (mutate == "tail_last" and n > reg_rows) or (mutate == "group_partial" and n % 4 != 0 and n <= reg_rows):
                kill[w] = n - 1
        table = exp_table()
        syn1 = np.zeros((V, dim), dt)
        words_before = np.concatenate([[0], np.cumsum([len(s) for s in sents])])
        total = int(words_before[-1])
        for k in range(iterations):
            for s, sent in enumerate(sents):
                n_tok = len(sent)
                if n_tok == 0:
                    continue
                alpha = learning_rate(lr, k, iterations, total, words_before[s + 1 if mutate == "alpha_late" else s])
                shrink = (w2v_hash(seed, k, s, np.arange(n_tok)) % np.uint32(window)).astype(np.int64)
                if mutate == "window_last":
                    shrink[n_tok - 1] = 0
                for pos in range(n_tok):
                    word = int(sent[pos]); b = int(shrink[pos])
                    prev_ctx, prev_row = -1, None
                    for a in range(b, 2 * window + 1 - b):
                        c = pos - window + a
                        if a == window or c < 0 or c >= n_tok:
                            continue
                        ctx = int(sent[c])
                        r0 = prev_row if (mutate == "stale_repeat" and ctx == prev_ctx) else syn0[ctx].copy()
                        new0, new1, ind = pair_update(r0, syn1[nodes[word]], bits[word], alpha, table, order,
                                                      mutate == "index_round", kill[word])
                        syn1[nodes[word]] = new1
                        syn0[ctx] = new0
                        indices.append(ind)
                        prev_ctx, prev_row = ctx, r0
    indices = np.concatenate(indices) if indices else np.zeros(0, np.int64)
    return Fit(ids, syn0.astype(np.float64), indices, int((indices < 0).sum()))


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def reg_rows_of(dim):
    """Node rows k_w2v_train_rows keeps in registers at this dim; the nodes past them go through memory."""
    return 32 if dim <= 64 else 24 if dim <= 256 else 8 if dim <= 512 else 4


def pack(sentences, stride=None):
    """Sentences (lists of ids) -> (paths [n, stride] padded with -1, lens)."""
    stride = stride or max([len(s) for s in sentences] + [1])
    paths = np.full((len(sentences), stride), -1, np.int32)
    lens = np.zeros(len(sentences), np.int32)
    for i, s in enumerate(sentences):
        paths[i, : len(s)] = s; lens[i] = len(s)
    return paths, lens


@functools.lru_cache(maxsize=None)
def karate_walks(walk_length, num_walks, seed=3):
    import oracle_py
    g = oracle_py.Graph.load(KARATE)
    paths, lens, _ = g.walk(p=0.5, q=2.0, walk_length=walk_length, num_walks=num_walks, seed=seed)
    paths.setflags(write=False); lens.setflags(write=False)
    return paths, lens


def counted_words(counts, seed, stride=40, base=100):
    """Word base + i occurs counts[i] times; the tokens shuffled, cut into sentences of `stride` (the last one shorter)."""
    toks = np.repeat(np.arange(len(counts), dtype=np.int32) + base, counts)
    np.random.default_rng(seed).shuffle(toks)
    n = (len(toks) + stride - 1) // stride
    paths = np.full((n, stride), -1, np.int32)
    paths.reshape(-1)[: len(toks)] = toks
    lens = np.full(n, stride, np.int32); lens[-1] = len(toks) - (n - 1) * stride
    return paths, lens


def fibonacci_words(n_words, k, seed, stride=40):
    """Fibonacci counts give the deepest tree a vocabulary can have (code lengths 1 .. n_words - 1, the two rarest words alike);
    every count times k, so that the deep nodes are visited often."""
    fib = [1, 1]
    while len(fib) < n_words:
        fib.append(fib[-1] + fib[-2])
    return counted_words(np.array(fib[:n_words]) * k, seed, stride)


Case = collections.namedtuple("Case", "name paths lens dim window iterations lr seed mutants")


def _case(name, pl, dim, window, iterations, lr=0.025, seed=11, mutants=()):
    return Case(name, pl[0], pl[1], dim, window, iterations, lr, seed, tuple(mutants))


PAIR_MUTANTS = ("alpha_late", "index_round", "window_last", "stale_repeat")
TAIL_MUTANTS = ("tail_last", "group_partial")

# code lengths 1 .. 12 (every residue mod 4 below and above 4 and 8 register rows), words 11 and 12 alike
RESIDUE_COUNTS = np.array([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233]) * 8

# one sentence of 1 200 tokens, hand-made patterns, an empty sentence between two trained ones: stride > every length but the first
_rng = np.random.default_rng(12)
TOKEN_SENTENCES = [
    [int(x) for x in _rng.integers(0, 12, 1200)],
    [7, 7, 7, 7, 7],
    [3, 9, 3, 9, 3, 9],
    [5, 5, 8, 5],                                  # a context equal to the centre
    [4, 6],
    [2],
    [],
    [1, 0, 11, 0, 1, 10, 10, 2],
    [],
    [],
    [9, 8, 7, 6, 5, 4, 3, 2, 1, 0],
]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: every input the CPU footing and the GPU comparison share."""
    out = []
    for dim in (16, 128):
        out.append(_case("karate-d%d-w5" % dim, karate_walks(20, 4), dim, 5, 3, mutants=PAIR_MUTANTS))
    # lr 0.1: at 0.025 the wide vectors (initial scale 0.5 / dim) keep every f within two or three table bins of 0 in so short a run;
    # at 0.1 the look-ups spread over 600 and more bins at every dim
    for dim in (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024):
        out.append(_case("lanes-d%d" % dim, karate_walks(12, 2), dim, 3, 2, lr=0.1, seed=5))
    for window in (1, 31, 32, 33):
        out.append(_case("window-%d" % window, karate_walks(80, 1), 64, window, 1))
    for dim in (300, 512):
        out.append(_case("fib13x8-d%d" % dim, fibonacci_words(13, 8, 1), dim, 2, 2, mutants=TAIL_MUTANTS))
    for dim in (600, 1024):
        out.append(_case("fib9x16-d%d" % dim, fibonacci_words(9, 16, 2), dim, 2, 2, mutants=TAIL_MUTANTS))
    for dim in (300, 600):
        out.append(_case("residues-d%d" % dim, counted_words(RESIDUE_COUNTS, 3), dim, 2, 1, mutants=TAIL_MUTANTS))
    out.append(_case("tokens-d16", pack(TOKEN_SENTENCES, stride=1203), 16, 4, 2, mutants=("stale_repeat", "window_last")))
    # lr 1: the vectors leave the table's range within the first sentences (the first gated node is the 146th evaluated) and stay
    # there: most nodes are gated out, the rest spread over both ends of the table.  Rates between 0.4 and 0.9 reach the gate too, but
    # through a chaotic stretch in which float32 and float64 part by whole units: no tolerance can be derived there.
    out.append(_case("gate-d16", karate_walks(12, 2), 16, 5, 1, lr=1.0, mutants=("index_round",)))
    return collections.OrderedDict((c.name, c) for c in out)


def run(case, **kw):
    return fit(case.paths, case.lens, case.dim, case.window, case.iterations, case.lr, case.seed, **kw)


@functools.lru_cache(maxsize=None)
def footing(name):
    """(ref64 Fit, noise, T) of a case: noise = the largest distance to ref64 of the two float32 restatements (the oracle's, left to
    right, and this module's in wave order), T = 8 * noise."""
    import oracle_py
    c = cases()[name]
    r64 = run(c)
    r32 = run(c, dtype=np.float32, order="wave")
    oids, ovec = oracle_py.w2v_fit(c.paths, c.lens, dim=c.dim, window=c.window, iterations=c.iterations, lr=c.lr, seed=c.seed)
    assert np.array_equal(oids, r64.ids) and np.array_equal(r32.ids, r64.ids)
    noise = max(float(np.abs(ovec.astype(np.float64) - r64.vectors).max()), float(np.abs(r32.vectors - r64.vectors).max()))
    r64.vectors.setflags(write=False)
    return r64, noise, 8.0 * noise
