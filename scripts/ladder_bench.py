"""K11 ladder build against the torch composition a user would write without it.

    python scripts/ladder_bench.py [--players 1000000,10000000] [--runs 25] [--out FILE]
    python scripts/ladder_bench.py --players 10000000 --runs 3 --only ladder   # under a kernel trace

Per roster size, one track (shared) and all seven: ``build_ladder`` and the comparator
are timed with device events in the same process, interleaved run by run, and the
medians printed as one JSON line per size.  The comparator is plain torch on the
strided roster views -- ``s = mu - sigma``, a stable sort with the unranked players
masked to NaN, an index scatter for the ranks -- once per track; it shares no code with
the ladder.  Both end in the one host read that sizes their outputs.  Before timing,
the two orders are compared on every track (they must be equal).

``keys_bytes`` is what ladder_keys moves (the roster read once, keys and ids written per
track); divide it by the kernel's time from ``rocprofv3 --kernel-trace --stats`` (a run
of its own, ``--only ladder``) for its effective bytes per second.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.config import MODES  # noqa: E402
from analyzer_amd.ops.ladder import build_ladder  # noqa: E402
from analyzer_amd.ops.synth import RosterSpec, make_roster  # noqa: E402

TRACKS = ("shared",) + MODES


def torch_ladder(state, granule):
    """(order int64 [R], score [R], rank int64 [P]) of one track with torch ops alone."""
    mu, sigma = state[:, 4 * granule], state[:, 4 * granule + 2]
    s = mu - sigma + 0.0
    ranked = ~torch.isnan(s) & (sigma <= float("inf"))
    neg = torch.where(ranked, -s, torch.full_like(s, float("nan")))  # ascending sort, NaN last
    vals, idx = torch.sort(neg, stable=True)
    R = int(ranked.sum())
    order = idx[:R]
    rank = torch.full((state.shape[0],), -1, dtype=torch.int64, device=state.device)
    rank[order] = torch.arange(R, dtype=torch.int64, device=state.device)
    return order, -vals[:R], rank


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--players", default="1000000,10000000")
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "ladder"], default="both",
                    help="ladder: no comparator and no check (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("ladder_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    for P in [int(float(p)) for p in args.players.split(",")]:
        state = make_roster(RosterSpec(num_players=P, seed=5, p_rated=0.9, p_mode_rated=0.6), device=dev).state
        cases = {"ladder_1": lambda: build_ladder(state, ("shared",)),
                 "ladder_7": lambda: build_ladder(state, TRACKS)}
        if args.only == "both":
            cases["torch_1"] = lambda: torch_ladder(state, 0)
            cases["torch_7"] = lambda: [torch_ladder(state, g) for g in range(7)]
            lad = build_ladder(state, TRACKS)
            for g, t in enumerate(TRACKS):
                order, score, rank = torch_ladder(state, g)
                assert torch.equal(order.to(torch.int32), lad.order(t)), "orders differ on " + t
                assert torch.equal(score, lad.score(t)) and torch.equal(rank.to(torch.int32), lad.rank(t))
            ranked = {t: lad.ranked(t) for t in TRACKS}
            del lad, order, score, rank
        else:
            ranked = None
        for _ in range(args.warmup):
            for fn in cases.values():
                timed(fn)
        times = {k: [] for k in cases}
        for _ in range(args.runs):  # interleaved: every run times each case once
            for k, fn in cases.items():
                times[k].append(timed(fn))
        line = {"players": P, "runs": args.runs, "ranked": ranked,
                "keys_bytes": {"1": P * 128 + 1 * P * 8, "7": P * 128 + 7 * P * 8}}
        for k, v in times.items():
            line[k + "_ms"] = round(statistics.median(v), 4)
            line[k + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        if args.only == "both":
            line["torch_over_ladder_1"] = round(line["torch_1_ms"] / line["ladder_1_ms"], 3)
            line["torch_over_ladder_7"] = round(line["torch_7_ms"] / line["ladder_7_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del state, cases
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
