"""The specification of srw_importance_neighbors restated in numpy (include/stellar_rw.h) — written from the header comment,
not from the kernels.  Shared by tests/test_importance_cpu.py (a graph worked by hand, planted misreadings, the Monte-Carlo reading) and
tests/test_gpu_importance.py.  R = num_walks, L = walk_length, T = top.

  words     philox4x32_10(ctr = (base + b, w, s, epoch), key = (seed, 65))     (skipgram_ref.philox_np, pinned to the oracle's Philox)
  restart   before a step s >= 1 the walk ends if (words[1] >> 8) < restart_m; never before step 0
  dead end  the walk ends if N(curr) is empty
  step      m = words[0] >> 8, u = m * 2^-24, next = the entry oracle_py.sample_index (RandomSample.sample) returns for N(curr)'s raw
            weights and u; arriving at next is one visit
  counts    c(v) over the R walks of the seed; the seed's own visits dropped unless keep_seed; total = the sum of c after that drop
  row       the vertices with c > 0 by c descending, then id ascending (signed); the first T, padded with (-1, 0)
  unknown   a seed that is -1 or no present vertex: an all-padding row, total 0, counted; a present seed with an empty row: not counted

`neighbors(v)` is how the graph is asked, as in neighbors_ref: (ids, weights) in srw_graph_neighbors order, or None when v is no present
vertex.  The draws of all walks of a step are taken together: a row's running sums acc_k are formed once, in RandomSample.sample's order
(S = the f64 left fold of the weights, acc += (double)w / S entry by entry), and "the first k with acc_k >= m * 2^-24, the head if
none" is looked up in them.  That holds for a row of finite non-negative weights with a positive sum, where acc does not decrease;
every other row (a negative or NaN weight) asks oracle_py.sample_index draw by draw.  Rows.check_against holds the former to the
latter (tests/test_importance_cpu.py does it for every row the GPU file uses)."""
import numpy as np

from neighbors_ref import Rows as _NeighborRows
from skipgram_ref import philox_np

KEY = 65
DEFECTS = ("vertex_key", "restart_at_0", "restart_le", "ties_desc", "seed_kept")      # planted misreadings of the header comment
ARMS = ("restart_cuts", "dead_ends", "boundary_ties", "dropped_seed_visits")
HOLE = np.iinfo(np.int64).max                        # no visit: the walk has ended


def words(b, w, s, epoch, seed):
    """(words[0], words[1]) of step s of walk w of seed b -> two uint64 arrays (broadcast over b, w, s)"""
    o = philox_np(b, w, s, epoch, seed, KEY)
    return o[0], o[1]


class Rows(_NeighborRows):
    """neighbors(v) with a cache, and the draw over a row for many m at once"""

    def __init__(self, neighbors):
        super().__init__(neighbors)
        self.acc = {}

    def running_sums(self, v):
        """acc_k of a row as RandomSample.sample forms them, or None when the row is not one of finite non-negative weights"""
        v = int(v)
        if v not in self.acc:
            w = self(v)[1]
            a = None
            if len(w) and np.isfinite(w).all() and (w >= 0).all():
                w64 = w.astype(np.float64)
                S = np.add.accumulate(w64)[-1]                                # the left fold, entry by entry
                if S > 0:
                    a = np.add.accumulate(w64 / S)                            # acc += w / S, entry by entry
            self.acc[v] = a
        return self.acc[v]

    def pick(self, oracle, v, m):
        """positions in N(v) of the draws m (uint array) -> int array"""
        m = np.asarray(m, dtype=np.int64)
        a = self.running_sums(v)
        if a is None:
            w = self(v)[1]
            return np.array([oracle.sample_index(w, float(np.float32(x) * np.float32(2.0 ** -24))) for x in m.tolist()], dtype=np.int64)
        k = np.searchsorted(a, m.astype(np.float64) * 2.0 ** -24, side="left")   # the first k with acc_k >= u (m * 2^-24 is exact)
        return np.where(k < len(a), k, 0)                                     # none: the row's head

    def check_against(self, oracle, v, rng, n=64):
        """the lookup in the running sums against oracle_py.sample_index: random draws, and the draws on both sides of every acc_k"""
        a = self.running_sums(v)
        if a is None:
            return 0
        w = self(v)[1]
        edge = np.floor(a[:min(len(a), 256)] * 2.0 ** 24).astype(np.int64)
        m = np.concatenate([rng.integers(0, 1 << 24, size=n), edge - 1, edge, edge + 1, [0, (1 << 24) - 1]])
        m = np.unique(m[(m >= 0) & (m < (1 << 24))])
        got = self.pick(oracle, v, m)
        for x, k in zip(m.tolist(), got.tolist()):
            assert k == oracle.sample_index(w, float(np.float32(x) * np.float32(2.0 ** -24))), (v, x, k)
        return len(m)


def visits(oracle, neighbors, seeds, R, L, restart_m, seed=1, epoch=0, base=0, rows=None, defect=None):
    """-> (V, arms): V int64 [len(rows), R, L], the vertex walk w of seed rows[r] arrives at in step s, or a hole (HOLE) where the walk
    has ended; arms: restart cuts and dead ends met"""
    row_of = neighbors if isinstance(neighbors, Rows) else Rows(neighbors)
    seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
    b = np.arange(len(seeds), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    key_b = (seeds[b] & 0xFFFFFFFF) if defect == "vertex_key" else (base + b)
    V = np.full((len(b), R, L), HOLE, dtype=np.int64)
    curr = np.repeat(seeds[b].reshape(-1, 1), R, axis=1)                      # [rows, R]
    known = np.array([row_of(v) is not None for v in seeds[b].tolist()], dtype=bool)
    alive = np.repeat(known.reshape(-1, 1), R, axis=1)
    w_idx = np.arange(R, dtype=np.int64).reshape(1, -1)
    arms = {"restart_cuts": 0, "dead_ends": 0}
    for s in range(L):
        if not alive.any():
            break
        w0, w1 = words(key_b.reshape(-1, 1), w_idx, s, epoch, seed)
        if s >= 1 or defect == "restart_at_0":
            d = (w1 >> np.uint64(8)).astype(np.int64)
            cut = alive & ((d <= restart_m) if defect == "restart_le" else (d < restart_m))
            arms["restart_cuts"] += int(cut.sum())
            alive = alive & ~cut
        m = (w0 >> np.uint64(8)).astype(np.int64)
        nxt = curr.copy()
        for v in np.unique(curr[alive]).tolist():
            at = alive & (curr == v)
            nb = row_of(v)
            ids = nb[0] if nb is not None else ()                             # (an id the rows name without a row of its own: no entries)
            if len(ids) == 0:                                                  # a dead end
                arms["dead_ends"] += int(at.sum())
                alive = alive & ~at
                continue
            nxt[at] = ids[row_of.pick(oracle, v, m[at])]
        V[:, :, s][alive] = nxt[alive]
        curr = nxt
    return V, arms



def sample(oracle, neighbors, seeds, R, L, T, restart_m, seed=1, epoch=0, base=0, keep_seed=False, rows=None, defect=None):
    """-> (ids int32 [len(rows), T], counts int32 [len(rows), T], total int32 [len(rows)], n_unknown over ALL the seeds, arms).  rows: the
    seed indices b to work out (default: all of them) — a row depends on nothing else in the batch.  arms: how often each arm was met
    (ARMS) over the rows worked out."""
    assert defect is None or defect in DEFECTS
    row_of = neighbors if isinstance(neighbors, Rows) else Rows(neighbors)
    seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
    n_unknown = sum(1 for v in seeds.tolist() if row_of(v) is None)
    b = np.arange(len(seeds), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    V, arms = visits(oracle, row_of, seeds, R, L, restart_m, seed=seed, epoch=epoch, base=base, rows=b, defect=defect)
    arms.update(boundary_ties=0, dropped_seed_visits=0)
    ids = np.full((len(b), T), -1, dtype=np.int32)
    counts = np.zeros((len(b), T), dtype=np.int32)
    total = np.zeros(len(b), dtype=np.int32)
    keep = keep_seed or defect == "seed_kept"
    for r in range(len(b)):
        v = V[r][V[r] != HOLE]
        if not keep:
            own = v == seeds[b[r]]
            arms["dropped_seed_visits"] += int(own.sum())
            v = v[~own]
        total[r] = len(v)
        u, c = np.unique(v, return_counts=True)
        order = np.lexsort((-u if defect == "ties_desc" else u, -c))           # c descending, then id ascending
        u, c = u[order], c[order]
        if len(u) > T and c[T - 1] == c[T]:
            arms["boundary_ties"] += 1
        n = min(T, len(u))
        ids[r, :n], counts[r, :n] = u[:n], c[:n]
    return ids, counts, total, n_unknown, arms
