"""CFO_GD_EDGE on the CPU: the builder's rule and the pick restated in numpy (tests/first_order_code_ref.py) against brute force —
first k with c_k >= m, else 0 — on every row and every draw the issue names, and the four planted defects those inputs must catch.
No GPU: the same rows and draws go through the kernels in tests/test_gpu_first_order_reads.py."""
import numpy as np
import pytest

import first_order_code_ref as ref

ROWS = ref.rows()
_BUILT = {}


def built(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _BUILT:
        w = dict(ROWS)[name]
        _BUILT[key] = ref.build(w, **kw)
    return _BUILT[key]


def wrong_picks(name, build_kw=None, pick_kw=None):
    """Draws of the row whose pick differs from brute force over the CORRECT c values."""
    w = dict(ROWS)[name]
    c, _ = built(name)
    _, code = built(name, **(build_kw or {}))
    bad = []
    for m in ref.draws(w, c):
        k, _ = ref.pick(c, code, int(m), **(pick_kw or {}))
        if k != ref.brute(c, int(m)):
            bad.append(int(m))
    return bad


@pytest.mark.parametrize("name", [n for n, _ in ROWS])
def test_pick_equals_brute_force(name):
    w = dict(ROWS)[name]
    c, code = built(name)
    assert np.all(np.diff(c) >= 0)
    n_coded = len(ref.coded_buckets(code))
    print("%s: deg %d, coded buckets %d" % (name, len(w), n_coded))
    assert code[0] != ref.EDGE
    for plain in (False, True):                     # the coded tables, and the plain ones of the A/B switch with the earlier pick
        cd = ref.build(w, edge_code=False)[1] if plain else code
        for m in ref.draws(w, c):
            m = int(m)
            k, reads = ref.pick(c, cd, m, reload=plain)
            assert k == ref.brute(c, m), (name, plain, m, k)
            assert reads >= 1


@pytest.mark.parametrize("name", [n for n, _ in ROWS])
def test_reads_of_the_coded_buckets(name):
    """What the code buys: a draw of a coded bucket that is not its lowest loads ONE record where c_j >= m (three before), its lowest
    draw two; and the code never stands where the certificate fails."""
    w = dict(ROWS)[name]
    deg = len(w)
    c, code = built(name)
    _, plain = built(name, edge_code=False)
    T = ref.thresholds(deg).astype(np.int64)
    for j in ref.coded_buckets(code):
        assert plain[j] == 1 and c[j - 1] == T[j]
    for m in ref.draws(w, c):
        m = int(m)
        j = (m * deg) >> 24
        if code[j] != ref.EDGE:
            assert ref.pick(c, code, m) == ref.pick(c, plain, m)                  # nothing else changes a load ...
            continue
        k, reads = ref.pick(c, code, m)
        kp, reads_p = ref.pick(c, plain, m, reload=True)
        assert k == kp
        if ref.is_lowest(m, deg, j):
            assert (k, reads, reads_p) == (j - 1, 2, 2)
        elif c[j] >= m:
            assert (k, reads, reads_p) == (j, 1, 3)
        assert ref.pick(c, plain, m)[1] == reads_p - (0 if ref.is_lowest(m, deg, j) else 1)   # ... but the kept record: one load less


def test_where_the_code_appears():
    n = {name: len(ref.coded_buckets(built(name)[1])) for name, _ in ROWS}
    print(n)
    assert n["unit1"] == 0 and n["unit16"] > 0 and n["unit3072"] > 0
    # (1.5, 0.5) repeated: cdf_k is (k + 1.5) / 64 at even k, (k + 1) / 64 at odd k — every bucket j >= 1 has delta 1, the predecessor
    # sits ON the threshold for even j (coded) and half an entry above it for odd j (the certificate fails: the plain delta remains)
    _, plain = built("pattern1.5_0.5", edge_code=False)
    _, code = built("pattern1.5_0.5")
    assert np.all(plain[1:] == 1)
    assert np.all(code[1::2] == 1) and np.all(code[2::2] == ref.EDGE)
    _, heavy = built("heavy_first")
    assert heavy[2047] == ref.SAT and heavy[2046] == 2046


def test_planted_defects_are_caught():
    # the lowest-draw test dropped: the bucket's lowest draw crosses at j - 1
    assert wrong_picks("unit16", pick_kw={"drop_lowest_test": True})
    # the code written without the certificate, on the row where delta is 1 and the certificate fails
    assert wrong_picks("pattern1.5_0.5", build_kw={"certificate": False})
    # a genuine delta equal to the reserved value, not saturated
    assert wrong_picks("heavy_first", build_kw={"saturate_reserved": False})
    # the kept record reused at an index other than j
    assert wrong_picks("random5decades", pick_kw={"reuse_at": -1})        # (needs a delta >= 2 whose scan ends at j: weighted rows)
    # and none of those inputs flags the code as it is
    for name, _ in ROWS:
        assert not wrong_picks(name)
