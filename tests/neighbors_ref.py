"""The specification of srw_sample_neighbors restated in numpy (include/stellar_rw.h) — written from the header comment, not
from the kernels.  Shared by tests/test_neighbors_cpu.py (a graph worked by hand, planted misreadings) and tests/test_gpu_neighbors.py.

  layout    F_0 = 1, F_l = F_{l-1} * fanouts[l-1]; layer l is [B][F_l]; the parent of (b, j) of layer l is (b, j // fanouts[l-1]) of layer
            l-1; layer 0 is the seed list
  -1        the child of -1, of an id that is no present vertex, of a vertex whose row is empty
  word      philox4x32_10(ctr = (b, j, l, epoch), key = (seed, 64))[0]        (skipgram_ref.philox_np, pinned to the oracle's Philox)
  replace   m = word >> 8, u = m * 2^-24, the entry oracle_py.sample_index (RandomSample.sample) returns for the row's raw weights and u
  distinct  deg <= f: the row in row order, then -1; else Floyd in selection order: J = deg - f + i, t = (word_i * (J + 1)) >> 32,
            position t unless an earlier child of this parent took it, else position J

`neighbors(v)` is how the graph is asked: (ids, weights) in srw_graph_neighbors order, or None when v is no present vertex —
oracle_py.Graph.neighbors, or Engine.neighbors for a graph loaded through load_adjacency."""
import numpy as np

from skipgram_ref import philox_np

KEY = 64
DEFECTS = ("vertex_key", "parent_mod", "floyd_j_minus_1")      # planted misreadings of the header comment (test_neighbors_cpu.py)


def row_lengths(fanouts):
    F = [1]
    for f in fanouts:
        F.append(F[-1] * int(f))
    return F


def words(b, F, layer, epoch, seed):
    """word of every element (b[r], j), j = 0 .. F - 1 -> uint64 [len(b), F]"""
    b = np.asarray(b, dtype=np.int64).reshape(-1, 1)
    j = np.arange(F, dtype=np.int64).reshape(1, -1)
    return philox_np(b, j, layer, epoch, seed, KEY)[0]


class Rows:
    """neighbors(v) with a cache; -1 never names a vertex"""

    def __init__(self, neighbors):
        self.neighbors, self.cache = neighbors, {}

    def __call__(self, v):
        v = int(v)
        if v == -1:
            return None
        if v not in self.cache:
            nb = self.neighbors(v)
            self.cache[v] = None if nb is None else (np.asarray(nb[0], dtype=np.int32), np.ascontiguousarray(nb[1], dtype=np.float32))
        return self.cache[v]


def sample(oracle, neighbors, seeds, fanouts, seed=1, epoch=0, replace=True, rows=None, defect=None):
    """-> (layers: list of int32 [len(rows), F_l], n_unknown over ALL the seeds, Floyd collisions resolved).  rows: the seed indices b
    to work out (default: all of them) — a row depends on nothing else in the batch."""
    assert defect is None or defect in DEFECTS
    seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
    row_of = neighbors if isinstance(neighbors, Rows) else Rows(neighbors)
    n_unknown = sum(1 for v in seeds.tolist() if row_of(v) is None)
    b = np.arange(len(seeds), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    key_b = seeds[b] & 0xFFFFFFFF if defect == "vertex_key" else b
    F = row_lengths(fanouts)
    prev = seeds[b].reshape(-1, 1)
    layers, collisions = [], 0
    for l in range(1, len(F)):
        f, Fp = int(fanouts[l - 1]), F[l - 1]
        W = words(key_b, F[l], l, epoch, seed)
        out = np.full((len(b), F[l]), -1, dtype=np.int64)
        U = ((W >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).tolist()      # m = word >> 8, u = m * 2^-24: exact, m < 2^24
        for r in range(len(b)):
            if replace:
                for j in range(F[l]):
                    jp = (j % f) % Fp if defect == "parent_mod" else j // f
                    nb = row_of(prev[r, jp])
                    if nb is None or len(nb[0]) == 0:
                        continue
                    out[r, j] = nb[0][oracle.sample_index(nb[1], U[r][j])]
            else:
                for jp in range(Fp):
                    nb = row_of(prev[r, jp])
                    if nb is None or len(nb[0]) == 0:
                        continue
                    ids, deg = nb[0], len(nb[0])
                    if deg <= f:
                        out[r, jp * f:jp * f + deg] = ids
                        continue
                    taken = []
                    for i in range(f):                                               # Floyd's loop, in selection order
                        J = deg - f + i
                        t = (int(W[r, jp * f + i]) * (J + 1)) >> 32
                        if t in taken:
                            collisions += 1
                            t = J - 1 if defect == "floyd_j_minus_1" else J
                        taken.append(t)
                        out[r, jp * f + i] = ids[t]
        layers.append(out.astype(np.int32))
        prev = out
    return layers, n_unknown, collisions
