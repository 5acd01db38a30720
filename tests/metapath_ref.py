"""The metapath walk restated from the header comment of srw_walk_metapath (include/stellar_rw.h) — TEST INFRASTRUCTURE ONLY.

Per walker and step: the row from the oracle's Graph.neighbors, a numpy mask by type, the draw from oracle_py.walk_uniform (or const_r),
and oracle_py.sample_index on the masked weights.  Nothing here knows how the device evaluates a step.

    types     one integer per present vertex, indexed by position in g.vertices() (ascending ids)
    pattern   m entries, a type or -1 (any); path position j (0 = the source) needs pattern[j mod m]
    a source whose type does not match pattern[0] gives the one-entry path; a step without a matching entry ends the walk
    dead_ends walkers that stopped at a step s > 1

`defect` plants a wrong reading of the comment (tests/test_metapath_cpu.py shows that each one is noticed):
    "zero_weight"  an entry that does not match is a candidate of weight zero
    "head0"        the fallback when no acc reaches the draw is position 0 of the ROW
    "s_minus_1"    step s takes pattern[(s - 1) mod m]
"""
import numpy as np


def sample_py(w, r):
    """RandomSample.sample in Python floats (IEEE f64, the oracle's operation order) -> (index, found): found is False when the
    head was taken because no acc reached the draw.  Only the planted defects need `found`; the restatement calls the oracle."""
    s = 0.0
    for x in w:
        s = s + float(x)
    p, acc = float(np.float32(r)), 0.0
    with np.errstate(all="ignore"):
        for k, x in enumerate(w):
            acc += float(np.float64(x) / np.float64(s))
            if acc >= p:
                return k, True
    return 0, False


class Walker:
    def __init__(self, oracle, g, types, pattern, rng="philox", const_r=0.0, seed=42, defect=None):
        self.oracle, self.g = oracle, g
        V = g.vertices()
        types = np.asarray(types)
        assert len(types) == len(V)
        self.V, self.types = V, types.astype(np.int64)
        self.type_of = dict(zip(V.tolist(), types.tolist()))
        self.pattern = [int(x) for x in pattern]
        self.rng, self.const_r, self.seed, self.defect = rng, float(const_r), int(seed), defect
        self._rows = {}

    def row(self, v):
        r = self._rows.get(v)
        if r is None:
            ids, w = self.g.neighbors(int(v))
            r = (ids, w, self.types[np.searchsorted(self.V, ids)])       # (every neighbour is a present vertex)
            self._rows[v] = r
        return r

    def draw(self, it, src, s):
        return self.const_r if self.rng == "const" else self.oracle.walk_uniform(self.seed, it, int(src), s)

    def pick(self, w, mask, u):
        """-> position in the row."""
        pos = np.flatnonzero(mask)
        if self.defect == "zero_weight":
            return self.oracle.sample_index(np.where(mask, w, np.float32(0)), u)
        if self.defect == "head0":
            k, found = sample_py(w[mask], u)
            return int(pos[k]) if found else 0
        return int(pos[self.oracle.sample_index(w[mask], u)])

    def path(self, it, src, walk_length):
        """-> (list of ids, stopped at a step s > 1)."""
        m = len(self.pattern)
        out = [int(src)]
        if self.pattern[0] >= 0 and self.type_of[int(src)] != self.pattern[0]:
            return out, False
        curr = int(src)
        for s in range(1, walk_length + 2):
            ids, w, tp = self.row(curr)
            req = self.pattern[((s - 1) if self.defect == "s_minus_1" else s) % m]
            mask = np.ones(len(ids), dtype=bool) if req < 0 else (tp == req)
            if not mask.any():
                return out, s > 1
            curr = int(ids[self.pick(w, mask, self.draw(it, src, s))])
            out.append(curr)
        return out, False


def walk(oracle, g, types, pattern, walk_length=80, num_walks=1, first_walk=0, rng="philox", const_r=0.0, seed=42, sources=None,
         defect=None, only=None):
    """-> (paths [n_walkers, walk_length + 2] int32 with -1 tail, lens, n_steps, dead_ends); walker = iteration * n + position, over the
    present vertices in ascending order or over `sources` in list order.  only: walker indices to evaluate (the other rows stay -1 /
    0 and are not counted)."""
    W = Walker(oracle, g, types, pattern, rng=rng, const_r=const_r, seed=seed, defect=defect)
    srcs = W.V if sources is None else np.asarray(sources)
    n = len(srcs)
    nw = num_walks * n
    paths = np.full((nw, walk_length + 2), -1, dtype=np.int32)
    lens = np.zeros(nw, dtype=np.int32)
    steps = dead = 0
    for wi in (range(nw) if only is None else only):
        it, vi = divmod(int(wi), n)
        p, d = W.path(first_walk + it, srcs[vi], walk_length)
        paths[wi, :len(p)] = p
        lens[wi] = len(p)
        steps += len(p) - 1
        dead += int(d)
    return paths, lens, steps, dead
