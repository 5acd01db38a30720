"""The first-order kernel's path flush restated in plain Python (csrc/walk_kernels.hip:k_walk_first_order).

A row of `stride` ints starts at byte base + 4 * w * stride.  A walker writes slot s of its row into ring column s & (W - 1) at step s
(slot 0 before the first step).  With a = (address of the row >> 2) & (W - 1), slot t lies at position (a + t) & (W - 1) of its
4W-byte line.  After slot s is written the row is DUE when (a + s) & (W - 1) == W - 1, or when s is the last slot; a due row stores
slots t0 .. s, t0 = s - ((a + s) & (W - 1)), those below 0 masked, each read from ring column t & (W - 1).

simulate() plays that, and also the flush of before (`legacy`: every row at s & 15 == 15 and at the last slot, slots s - (s & 15) .. s),
and returns the store runs as (row, first slot, last slot, step).  Two defects can be planted: `due_off` shifts the due test by one
position, `mask_head=False` lets the first window start below slot 0.
"""

SECTOR = 64      # bytes of one write request
GRANULE = 32     # bytes the memory writes whole


def phase(base, w, stride, W):
    return ((base >> 2) + w * stride) & (W - 1)


def simulate(stride, base=0, W=16, n_rows=64, legacy=False, due_off=0, mask_head=True):
    """-> (runs, faults): runs = [(row, t_first, t_last, step)], in the order they are stored; faults = what the ring lost:
    ("overwritten", row, slot) for a ring entry written again before it was stored, ("stale", row, slot) for a stored slot whose
    ring entry holds another slot."""
    last = stride - 1
    runs, faults = [], []
    for w in range(n_rows):
        a = phase(base, w, stride, W)
        ring = [None] * W                   # ring column -> the slot it holds
        stored = set()
        for s in range(stride):
            c = s & (W - 1)
            if ring[c] is not None and ring[c] not in stored:
                faults.append(("overwritten", w, ring[c]))
            ring[c] = s
            if legacy:
                due, t0 = (s & 15) == 15 or s == last, s - (s & 15)
            else:
                pos = (a + s) & (W - 1)
                due, t0 = ((a + s + due_off) & (W - 1)) == W - 1 or s == last, s - pos
            if not due:
                continue
            if mask_head:
                t0 = max(t0, 0)
            for t in range(max(t0, 0), s + 1):
                if ring[t & (W - 1)] != t:
                    faults.append(("stale", w, t))
                stored.add(t)
            runs.append((w, t0, s, s))
    return runs, faults


def coverage(runs, stride, n_rows):
    """{(row, slot): times stored}, slots outside 0 .. stride - 1 included (a run that starts below 0 writes into the row before)."""
    n = {}
    for w, t0, t1, _ in runs:
        for t in range(t0, t1 + 1):
            n[(w, t)] = n.get((w, t), 0) + 1
    return n


def run_bytes(run, stride, base):
    w, t0, t1, _ = run
    lo = base + 4 * (w * stride + t0)
    return lo, lo + 4 * (t1 - t0 + 1)       # [lo, hi)


def crossings(runs, stride, base, W):
    """The runs that do not lie inside one 4W-byte line."""
    return [r for r in runs if run_bytes(r, stride, base)[0] // (4 * W) != (run_bytes(r, stride, base)[1] - 1) // (4 * W)]


def traffic(runs, stride, base, n_rows):
    """64-byte sector write requests and partly written 32-byte granules per walk-step (a row of `stride` slots is stride - 1 steps),
    and bytes written in whole granules over payload bytes (4 per slot) — each run counted on its own, as a store instruction's run
    reaches the memory."""
    sectors = partial = granules = 0
    for r in runs:
        lo, hi = run_bytes(r, stride, base)
        sectors += (hi - 1) // SECTOR - lo // SECTOR + 1
        g0, g1 = lo // GRANULE, (hi - 1) // GRANULE
        granules += g1 - g0 + 1
        for g in range(g0, g1 + 1):
            if max(lo, g * GRANULE) != g * GRANULE or min(hi, (g + 1) * GRANULE) != (g + 1) * GRANULE:
                partial += 1
    steps, slots = n_rows * (stride - 1), n_rows * stride
    return {"sector_requests": sectors / steps, "partial_granules": partial / steps, "bytes_over_payload": granules * GRANULE / (4.0 * slots)}
