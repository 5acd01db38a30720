"""The specification of srw_skipgram_windows restated in numpy (include/stellar_rw.h) — written from the text, not from
the kernel.  Shared by tests/test_skipgram_cpu.py (which pins philox_np to the oracle's Philox) and tests/test_gpu_skipgram.py.

  windows    row r has cnt[r] = max(0, lens[r] - C + 1) windows, window (r, j) = paths[r][j .. j + C - 1]; output order: r, then j
  negatives  entry k of window (r, j) = V[(word * nV) >> 32], word = philox4x32_10(ctr = (r, j, k >> 2, epoch), key = (seed, 1))[k & 3]
"""
import numpy as np

MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon et al., Random123) on arrays of counters and keys, in uint64 arithmetic -> four uint64 arrays < 2^32."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x).astype(np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                        # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + w0) & MASK, (k1 + w1) & MASK
    return c0, c1, c2, c3


def index_of(word, n_v):
    """(uint64(word) * nV) >> 32"""
    return (np.asarray(word).astype(np.uint64) * np.uint64(n_v)) >> S32


def counts(lens, C):
    return np.maximum(0, np.asarray(lens).astype(np.int64) - C + 1)


def windows_loop(paths, lens, C):
    """the double loop over (r, j)"""
    out = [paths[r, j:j + C] for r in range(len(lens)) for j in range(max(0, int(lens[r]) - C + 1))]
    return np.array(out, dtype=np.int32).reshape(len(out), C)


def windows_fast(paths, lens, C):
    """the same through sliding_window_view + a mask (row-major, then j: the order of a boolean index)"""
    n, stride = paths.shape
    if n == 0 or stride < C:
        return np.zeros((0, C), dtype=np.int32)
    view = np.lib.stride_tricks.sliding_window_view(paths, C, axis=1)           # [n, stride - C + 1, C]
    keep = np.arange(stride - C + 1)[None, :] < counts(lens, C)[:, None]
    return np.ascontiguousarray(view[keep])


def window_keys(lens, C):
    """(r, j) of every window in output order"""
    cnt = counts(lens, C)
    off = np.cumsum(cnt) - cnt
    r = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(off, cnt)
    return r, j


def negatives(lens, C, K, seed, epoch, V):
    r, j = window_keys(lens, C)
    V = np.asarray(V)
    out = np.zeros((len(r), K), dtype=np.int32)
    for b in range((K + 3) // 4):
        words = philox_np(r, j, b, epoch, seed, 1)
        for e in range(4):
            if 4 * b + e < K:
                out[:, 4 * b + e] = V[index_of(words[e], len(V)).astype(np.int64)]
    return out
