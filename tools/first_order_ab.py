"""Interleaved A/B of the first-order walk with and without CFO_GD_EDGE (tools/SWITCHES.md: SRW_NO_EDGE_CODE), in ONE process on ONE GPU:
two engines over the same generated RMAT graph, one with its compact tables built under the switch; after the warm-ups the two walk
the same iteration in strict alternation, so launch-to-launch drift and the box-to-box spread (STATUS.md) hit both arms alike.
Prints per-launch kernel_ms, the median and the spread (max - min) of each arm, ent_reads per step, and whether the two path buffers
are identical (compared on the device).  Scale 26 needs about 110 GB.

The kernel's time also moves by several per cent with the ALLOCATION its table landed in (profiles/r03_placement.md (b): 63 - 70 ms
from one rebuild to the next at RMAT-26), and the two arms are two allocations.  --rounds N repeats the whole experiment with both
engines rebuilt, the arm that is built first alternating: the summary then also compares the arms slot by slot (coded built first
against plain built first, second against second) — a difference that follows the slot and not the arm is placement.

--in-place takes the allocation out altogether: one engine that also holds the 32-byte table derives its compact records again, into
the buffer they are in, whenever the switch changes — the arms then differ in the table's CONTENTS only.

--arm flush compares the two forms of the path flush instead (include/stellar_rw.h: SRW_WALK_LEGACY_FLUSH, the keyword legacy_flush):
one engine, one table, one path buffer; the flag alternates per block of launches (aligned legacy legacy aligned ...), --rounds blocks
per arm, and every block's paths and lens are compared on the device with the first block's.  It counts as a gain when the paths are
identical, every block median of the aligned arm is below every block median of the legacy arm, and the median gain is larger than the
larger arm's spread (the rule of profiles/r07_edge_code.md).

usage: first_order_ab.py [--arm edge|flush] [--scale 26] [--launches 10] [--warmups 2] [--rounds 1] [--plain-first 0] [--in-place]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _pkg  # noqa: E402

SWITCH = "SRW_NO_EDGE_CODE"
ARMS = ("coded", "plain")


def same_on_device(torch, a, b, rows=1 << 22):
    """a == b everywhere, a slab of rows at a time (no temporary the size of the paths)."""
    if a.shape != b.shape:
        return False
    return all(bool(torch.equal(a[i:i + rows], b[i:i + rows])) for i in range(0, a.shape[0], rows))


def one_round(pkg, torch, scale, ef, L, K, W, order):
    """Both engines built in `order`, W warm-ups, K timed launches each in strict alternation -> {arm: {...}}, paths identical."""
    arms = {}
    try:
        for name in order:
            eng = pkg.Engine(device=0)
            arms[name] = {"eng": eng, "ms": []}
            eng.generate_rmat(scale, ef << scale, seed=42)
            if name == "plain":
                os.environ[SWITCH] = "1"             # read when the tables are built: the first walk
            try:
                st = eng.walk(fetch=False, walk_length=L, num_walks=1, first_walk=0, seed=42)
            finally:
                os.environ.pop(SWITCH, None)
            assert st["kernel_kind"] == 1 and st["record_bytes"] == 16, st
            print("  %s: tables built in %.0f ms, first launch %.2f ms, %.5f records per step" %
                  (name, st["setup_ms"], st["kernel_ms"], st["ent_reads"] / max(st["n_steps"], 1)), flush=True)
        for it in range(1, W):                       # (the table-building walk above was the first warm-up)
            for name in ARMS:
                arms[name]["eng"].walk(fetch=False, walk_length=L, num_walks=1, first_walk=it, seed=42)
        same = True
        for it in range(W, W + K):
            for name in (ARMS if it % 2 == 0 else ARMS[::-1]):       # strictly alternating, the order swapped every iteration
                st = arms[name]["eng"].walk(fetch=False, walk_length=L, num_walks=1, first_walk=it, seed=42)
                arms[name]["ms"].append(st["kernel_ms"]); arms[name]["last"] = st
            print("  iteration %d: coded %.3f ms  plain %.3f ms" % (it, arms["coded"]["ms"][-1], arms["plain"]["ms"][-1]), flush=True)
            if it in (W, W + K - 1):                 # the same iteration of both engines: the first and the last timed one
                (pa, la), (pb, lb) = arms["coded"]["eng"].paths_tensor(), arms["plain"]["eng"].paths_tensor()
                same = same and same_on_device(torch, pa, pb) and bool(torch.equal(la, lb))
                torch.cuda.synchronize()
        out = {}
        for name in ARMS:
            a, st = arms[name], arms[name]["last"]
            out[name] = {"kernel_ms": [round(x, 4) for x in a["ms"]], "median_ms": statistics.median(a["ms"]),
                         "spread_ms": max(a["ms"]) - min(a["ms"]), "n_steps": st["n_steps"], "ent_reads": st["ent_reads"],
                         "records_per_step": st["ent_reads"] / max(st["n_steps"], 1)}
        return out, same
    finally:
        for a in arms.values():
            a["eng"].close()


def in_place(pkg, torch, scale, ef, L, K, W, blocks):
    """ONE engine, ONE allocation: the exact table is built first, the compact records are derived from it — and derived again into
    the same buffer whenever the switch changes (sampler_tables.hip:build_first_order_tables).  `blocks` blocks of K launches per arm,
    alternating; every block walks the same K iterations.  -> {arm: {...}}, paths identical."""
    eng = pkg.Engine(device=0)
    try:
        eng.generate_rmat(scale, ef << scale, seed=42)
        eng.walk(fetch=False, walk_length=1, num_walks=1, rng="const", const_r=0.5)      # the exact 32-byte table
        arms = {name: {"ms": [], "blocks": []} for name in ARMS}
        ref_paths, same = None, True
        for b in range(2 * blocks):
            name = ARMS[(b + b // 2) % 2]            # coded plain plain coded coded plain ...: no arm always follows a rebuild of the other
            if name == "plain":
                os.environ[SWITCH] = "1"
            try:
                ms = []
                for it in range(W + K):
                    st = eng.walk(fetch=False, walk_length=L, num_walks=1, first_walk=it, seed=42)
                    assert st["kernel_kind"] == 1 and st["record_bytes"] == 16, st
                    if it >= W:
                        ms.append(st["kernel_ms"])
            finally:
                os.environ.pop(SWITCH, None)
            pa, la = eng.paths_tensor()
            if ref_paths is None:
                ref_paths = (pa.clone(), la.clone())
            else:
                same = same and same_on_device(torch, pa, ref_paths[0]) and bool(torch.equal(la, ref_paths[1]))
            arms[name]["ms"] += ms; arms[name]["blocks"].append(statistics.median(ms)); arms[name]["last"] = st
            print("  block %d %s: %s ms, %.5f records per step" % (b, name, " ".join("%.3f" % x for x in ms), st["ent_reads"] / max(st["n_steps"], 1)), flush=True)
        out = {}
        for name in ARMS:
            a, st = arms[name], arms[name]["last"]
            out[name] = {"kernel_ms": [round(x, 4) for x in a["ms"]], "block_medians_ms": a["blocks"], "median_ms": statistics.median(a["ms"]),
                         "spread_ms": max(a["ms"]) - min(a["ms"]), "n_steps": st["n_steps"], "ent_reads": st["ent_reads"],
                         "records_per_step": st["ent_reads"] / max(st["n_steps"], 1)}
        return out, same
    finally:
        eng.close()


def one_engine(pkg, torch, scale, ef, L, K, W, blocks, names, arm_of, compare=True):
    """ONE engine and ONE table; arm_of(name) -> (walk keywords, environment) of an arm.  `blocks` blocks of W warm-ups and K timed
    launches per arm in the order A B B A ..., every block walking the same iterations.  -> {arm: {...}}, paths identical."""
    eng = pkg.Engine(device=0)
    try:
        eng.generate_rmat(scale, ef << scale, seed=42)
        arms = {name: {"ms": [], "blocks": []} for name in names}
        ref_paths, same = None, True
        for b in range(2 * blocks):
            name = names[(b + b // 2) % 2]
            kw, env = arm_of(name)
            os.environ.update(env)
            try:
                ms = []
                for it in range(W + K):
                    st = eng.walk(fetch=False, walk_length=L, num_walks=1, first_walk=it, seed=42, **kw)
                    assert st["kernel_kind"] == 1 and st["record_bytes"] == 16, st
                    if it >= W:
                        ms.append(st["kernel_ms"])
            finally:
                for k in env:
                    os.environ.pop(k, None)
            if compare:
                pa, la = eng.paths_tensor()
                if ref_paths is None:
                    ref_paths = (pa.clone(), la.clone())
                else:
                    same = same and same_on_device(torch, pa, ref_paths[0]) and bool(torch.equal(la, ref_paths[1]))
            arms[name]["ms"] += ms; arms[name]["blocks"].append(statistics.median(ms)); arms[name]["last"] = st
            print("  block %d %s: %s ms" % (b, name, " ".join("%.3f" % x for x in ms)), flush=True)
        out = {}
        for name in names:
            a, st = arms[name], arms[name]["last"]
            out[name] = {"kernel_ms": [round(x, 4) for x in a["ms"]], "block_medians_ms": a["blocks"], "median_ms": statistics.median(a["ms"]),
                         "spread_ms": max(a["ms"]) - min(a["ms"]), "n_steps": st["n_steps"], "ent_reads": st["ent_reads"],
                         "records_per_step": st["ent_reads"] / max(st["n_steps"], 1)}
        return out, same
    finally:
        eng.close()


def summary(out, rounds, new, old, same):
    """The one-engine arms' figures and the rule: all of new's block medians below all of old's, the gain above the larger spread."""
    for name in (new, old):
        ms = rounds[0][name]["kernel_ms"]
        out[name] = {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "min_ms": min(ms), "max_ms": max(ms),
                     "block_medians_ms": rounds[0][name]["block_medians_ms"], "records_per_step": rounds[0][name]["records_per_step"]}
        print("%s: median %.3f ms over %d launches, spread %.3f ms (min %.3f, max %.3f), block medians %s" %
              (name, out[name]["median_ms"], len(ms), out[name]["spread_ms"], min(ms), max(ms),
               " ".join("%.3f" % x for x in out[name]["block_medians_ms"])))
    gain = out[old]["median_ms"] - out[new]["median_ms"]
    out["gain_ms"] = gain
    out["gain_frac"] = gain / out[old]["median_ms"]
    out["larger_spread_ms"] = max(out[new]["spread_ms"], out[old]["spread_ms"])
    out["gain_exceeds_spread"] = bool(gain > out["larger_spread_ms"])
    out["blocks_separated"] = bool(max(out[new]["block_medians_ms"]) < min(out[old]["block_medians_ms"]))
    out["is_gain"] = bool(same and out["gain_exceeds_spread"] and out["blocks_separated"])
    print("paths identical: %s; %s is %.3f ms (%.2f %%) below %s; larger spread %.3f ms; block medians separated: %s; a gain by the rule: %s" %
          (same, new, gain, 100.0 * out["gain_frac"], old, out["larger_spread_ms"], out["blocks_separated"], out["is_gain"]))
    return out


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=("edge", "flush"), default="edge", help="edge: CFO_GD_EDGE against plain deltas; flush: the aligned path flush against SRW_WALK_LEGACY_FLUSH")
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--walk-length", type=int, default=80)
    ap.add_argument("--launches", type=int, default=10, help="timed launches per arm and round (or per block)")
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=1, help="two engines: how often both are rebuilt; --in-place: blocks per arm")
    ap.add_argument("--plain-first", type=int, default=0, help="two engines: the plain arm's engine is built first in round 0")
    ap.add_argument("--in-place", action="store_true", help="one engine, the records re-derived into the same buffer (needs the 32-byte table too)")
    args = ap.parse_args()
    scale, K, W, R, L, ef = args.scale, max(args.launches, 1), args.warmups, max(args.rounds, 1), args.walk_length, args.edge_factor
    plain_first = args.plain_first
    if os.environ.get(SWITCH):
        raise SystemExit("%s is set in the environment: both arms would be the plain one" % SWITCH)
    pkg = _pkg.load()
    torch.zeros(1, device="cuda")
    rounds, same = [], True
    if args.arm == "flush":
        res, same = one_engine(pkg, torch, scale, ef, L, K, W, R, ("aligned", "legacy"), lambda name: ({"legacy_flush": name == "legacy"}, {}))
        out = {"arm": "flush", "scale": scale, "edge_factor": ef, "walk_length": L, "launches": K, "warmups": W, "blocks_per_arm": R,
               "paths_identical": bool(same)}
        print(json.dumps(summary(out, [res], "aligned", "legacy", same)), flush=True)
        if not same:
            raise SystemExit("the two arms' paths differ")
        return
    if args.in_place:
        res, same = in_place(pkg, torch, scale, ef, L, K, W, R)
        res["built_first"] = "one engine, in place"
        rounds.append(res)
        R = 1
    for r in range(0 if args.in_place else R):
        order = ARMS[::-1] if (r + plain_first) % 2 else ARMS
        print("round %d: %s built first" % (r, order[0]), flush=True)
        res, ok = one_round(pkg, torch, scale, ef, L, K, W, order)
        same = same and ok
        res["built_first"] = order[0]
        rounds.append(res)
        for name in ARMS:
            print("  %s: median %.3f ms, spread %.3f ms, %.5f records per step" %
                  (name, res[name]["median_ms"], res[name]["spread_ms"], res[name]["records_per_step"]))
    out = {"scale": scale, "edge_factor": ef, "walk_length": L, "launches": K, "warmups": W, "rounds": rounds, "paths_identical": bool(same)}
    for name in ARMS:
        ms = [x for rd in rounds for x in rd[name]["kernel_ms"]]
        out[name] = {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "min_ms": min(ms), "max_ms": max(ms),
                     "records_per_step": rounds[-1][name]["records_per_step"], "ent_reads": rounds[-1][name]["ent_reads"]}
        print("%s: median %.3f ms over %d launches, spread %.3f ms (min %.3f, max %.3f), %.5f records per step" %
              (name, out[name]["median_ms"], len(ms), out[name]["spread_ms"], min(ms), max(ms), out[name]["records_per_step"]))
    gain = out["plain"]["median_ms"] - out["coded"]["median_ms"]
    out["gain_ms"] = gain
    out["gain_frac"] = gain / out["plain"]["median_ms"]
    out["larger_spread_ms"] = max(out["coded"]["spread_ms"], out["plain"]["spread_ms"])
    out["gain_exceeds_spread"] = bool(gain > out["larger_spread_ms"])
    print("paths identical: %s; coded is %.3f ms (%.2f %%) below plain; larger spread %.3f ms" %
          (same, gain, 100.0 * out["gain_frac"], out["larger_spread_ms"]))
    if R > 1:                                        # slot by slot: the arms in the same place of the build order
        out["by_slot"] = {}
        for slot in ("first", "second"):
            med = {}
            for name in ARMS:
                ms = [x for rd in rounds if (rd["built_first"] == name) == (slot == "first") for x in rd[name]["kernel_ms"]]
                if ms:
                    med[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": len(ms)}
            out["by_slot"][slot] = med
            if len(med) == 2:
                print("built %s: coded median %.3f ms (%.3f .. %.3f), plain median %.3f ms (%.3f .. %.3f): coded %.2f %% below plain" %
                      (slot, med["coded"]["median_ms"], med["coded"]["min_ms"], med["coded"]["max_ms"], med["plain"]["median_ms"],
                       med["plain"]["min_ms"], med["plain"]["max_ms"], 100.0 * (1.0 - med["coded"]["median_ms"] / med["plain"]["median_ms"])))
    print(json.dumps(out), flush=True)
    if not same:
        raise SystemExit("the two arms' paths differ")


if __name__ == "__main__":
    main()
