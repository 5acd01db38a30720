"""The rule of the first-order kernel's path flush (tests/path_flush_ref.py restates it): for every stride, base offset and
ring width every slot of every row is stored exactly once, no run crosses a line, the ring loses nothing — and at the headline's stride
the sector and granule counts are the ones the change was reasoned from.  Two planted defects must be caught by the same checks."""
import pytest

import path_flush_ref as ref

STRIDES = (3, 7, 15, 16, 17, 18, 32, 33, 48, 82, 83)
BASES = (0, 4, 8, 60)
WIDTHS = (16, 32)
N_ROWS = 64                                  # one wave: every phase an odd stride has, twice over at W = 32


def problems(stride, base, W, **defect):
    """What the checks find: a list of strings, empty when the flush is right."""
    runs, faults = ref.simulate(stride, base, W, N_ROWS, **defect)
    out = ["%s row %d slot %d" % f for f in faults]
    n = ref.coverage(runs, stride, N_ROWS)
    for w in range(N_ROWS):
        for t in range(stride):
            if n.get((w, t), 0) != 1:
                out.append("row %d slot %d stored %d times" % (w, t, n.get((w, t), 0)))
    out += ["row %d slot %d: outside its row" % k for k in n if not 0 <= k[1] < stride]
    out += ["run %s crosses a %d-byte line" % (r, 4 * W) for r in ref.crossings(runs, stride, base, W)]
    return out


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("stride", STRIDES)
def test_rule(stride, base, W):
    assert problems(stride, base, W) == []


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("stride", STRIDES)
def test_interior_runs_are_whole_lines(stride, W):
    runs, _ = ref.simulate(stride, 0, W, N_ROWS)
    for w, t0, t1, _ in runs:
        if t0 > 0 and t1 < stride - 1:       # neither the head nor the tail of its row
            lo, hi = ref.run_bytes((w, t0, t1, 0), stride, 0)
            assert lo % (4 * W) == 0 and hi - lo == 4 * W


@pytest.mark.parametrize("W", WIDTHS)
def test_planted_due_test_off_by_one_is_caught(W):
    caught = [(s, b) for s in STRIDES for b in BASES if problems(s, b, W, due_off=1)]
    assert len(caught) == len(STRIDES) * len(BASES)
    # a row that goes out one slot early leaves the last slot of each line behind: never stored, and overwritten in the ring
    found = problems(82, 0, W, due_off=1)
    assert any("stored 0 times" in p for p in found) and any(p.startswith("overwritten") for p in found)


@pytest.mark.parametrize("W", WIDTHS)
def test_planted_unmasked_head_is_caught(W):
    # the head window starts below slot 0 wherever a row does not start on a line: stride 16 at base 0 is the one shape without such a row
    for s in STRIDES:
        for b in BASES:
            aligned = all(ref.phase(b, w, s, W) == 0 for w in range(N_ROWS))
            found = problems(s, b, W, mask_head=False)
            assert bool(found) != aligned, (s, b, found[:3])
            assert aligned or any("outside its row" in p for p in found)


def test_headline_stride_figures():
    """Stride 82 (walk length 80): per walk-step 0.128 sector requests, 0.105 partly written granules and 1.439 bytes written per payload
    byte with the flush of before; 0.074, 0.0185 and 1.073 with windows cut at address boundaries — at either width."""
    runs, faults = ref.simulate(82, 0, 16, 4096, legacy=True)
    assert not faults
    t = ref.traffic(runs, 82, 0, 4096)
    print("legacy", t)
    assert round(t["sector_requests"], 3) == 0.128 and round(t["partial_granules"], 3) == 0.105 and round(t["bytes_over_payload"], 3) == 1.439
    for W in WIDTHS:
        runs, faults = ref.simulate(82, 0, W, 4096)
        assert not faults
        t = ref.traffic(runs, 82, 0, 4096)
        print("aligned W", W, t)
        assert round(t["sector_requests"], 3) == 0.074 and round(t["partial_granules"], 4) == 0.0185 and round(t["bytes_over_payload"], 3) == 1.073


def test_legacy_flush_is_the_flush_of_before():
    """The restated legacy flush stores every slot once as well; its runs cross lines wherever a row does not start on one."""
    for s in STRIDES:
        runs, faults = ref.simulate(s, 0, 16, N_ROWS, legacy=True)
        n = ref.coverage(runs, s, N_ROWS)
        assert not faults and all(n.get((w, t), 0) == 1 for w in range(N_ROWS) for t in range(s)) and len(n) == N_ROWS * s
    assert ref.crossings(ref.simulate(82, 0, 16, N_ROWS, legacy=True)[0], 82, 0, 16)
