"""The specification of srw_skipgram_batch's negatives restated in numpy (include/stellar_rw.h) — written from the text, not
from the kernel.  Shared by tests/test_negatives_cpu.py and tests/test_gpu_negatives.py; Philox is skipgram_ref.philox_np (pinned to
the oracle's by tests/test_skipgram_cpu.py).

  table      w[nV] unsigned 32-bit weights over V (ascending present vertices), cdf[i] = w[0] + .. + w[i] (uint64), T = cdf[nV - 1] > 0
  weighted   blk = philox4x32_10(ctr = (r, j, k >> 1, epoch), key = (seed, 2 + 2 a)),  u = blk[2 (k & 1)] << 32 | blk[2 (k & 1) + 1],
             t = (u * T) >> 64,  i = smallest index with cdf[i] > t,  negative = V[i]
  uniform    word = philox4x32_10(ctr = (r, j, k >> 2, epoch), key = (seed, 1 + 2 a))[k & 3],  negative = V[(word * nV) >> 32]
  exclusion  a draw equal to one of the C vertices of its window is rejected and attempt a + 1 taken, up to max_draws attempts; the last
             attempt's vertex stands
"""
import numpy as np

import skipgram_ref as ref

MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def cdf_of(w):
    return np.cumsum(np.asarray(w).astype(np.uint64), dtype=np.uint64)


def hi64_int(u, T):
    """(u * T) >> 64 with Python integers"""
    return (int(u) * int(T)) >> 64


def hi64_split(uh, ul, T):
    """the same from 32-bit halves of u (arrays) and T, every product and sum inside uint64"""
    uh, ul = np.asarray(uh).astype(np.uint64), np.asarray(ul).astype(np.uint64)
    th, tl = np.uint64(int(T) >> 32), np.uint64(int(T) & 0xFFFFFFFF)
    ll, lh, hl, hh = ul * tl, ul * th, uh * tl, uh * th
    mid = (ll >> S32) + (lh & MASK) + (hl & MASK)          # < 3 * 2^32
    return hh + (lh >> S32) + (hl >> S32) + (mid >> S32)


def select(cdf, t):
    """smallest index with cdf[i] > t"""
    return np.searchsorted(cdf, np.asarray(t).astype(np.uint64), side="right")


def select_linear(cdf, t):
    for i, c in enumerate(cdf):
        if int(c) > int(t):
            return i
    raise ValueError("t >= T")


def draw(r, j, k, a, seed, epoch, V, cdf):
    """negative k of the windows (r, j) (arrays or scalars), attempt a"""
    if cdf is None:
        word = ref.philox_np(r, j, k >> 2, epoch, seed, 1 + 2 * a)[k & 3]
        return V[ref.index_of(word, len(V)).astype(np.int64)]
    blk = ref.philox_np(r, j, k >> 1, epoch, seed, 2 + 2 * a)
    t = hi64_split(blk[2 * (k & 1)], blk[2 * (k & 1) + 1], int(cdf[-1]))
    return V[select(cdf, t)]


def negatives(lens, C, K, seed, epoch, V, w=None, paths=None, exclude=False, max_draws=8):
    """-> (neg [W, K] int32, redraws, entries whose every attempt was rejected).  w: the quantised weights in force (None: uniform);
    paths: needed with exclude."""
    V = np.asarray(V)
    cdf = None if w is None else cdf_of(w)
    assert cdf is None or (len(cdf) == len(V) and int(cdf[-1]) > 0)
    r, j = ref.window_keys(lens, C)
    out = np.zeros((len(r), K), dtype=np.int32)
    for k in range(K):
        out[:, k] = draw(r, j, k, 0, seed, epoch, V, cdf)
    redraws = exhausted = 0
    if exclude and len(r):
        assert 1 <= max_draws <= 16
        win = np.asarray(paths)[r[:, None], j[:, None] + np.arange(C)[None, :]]         # [W, C]
        hit = (out[:, :, None] == win[:, None, :]).any(axis=2)
        for wi, k in np.argwhere(hit):                     # the loop per entry
            a, x = 0, out[wi, k]
            while x in win[wi] and a + 1 < max_draws:
                a += 1
                redraws += 1
                x = int(draw(r[wi], j[wi], int(k), a, seed, epoch, V, cdf))
            exhausted += int(x in win[wi])
            out[wi, k] = x
    return out, redraws, exhausted
