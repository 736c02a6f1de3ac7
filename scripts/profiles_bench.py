"""K17 profiles against K13 careers on the same window and the torch composition a user would
write without it.

    python scripts/profiles_bench.py [--matches 10000000] [--team 3] [--runs 9]
    python scripts/profiles_bench.py --runs 3 --only native   # under a kernel trace

Windows of M KvK matches, each folded into a profile table (``ProfileTable.add``):

* ``uniform_1M`` / ``uniform_10M``: players drawn uniformly from 1M / 10M;
* ``hot``: one player in slot 0 of every match, the rest uniform over 1M.

The records come from the counter-RNG stream (AFK and tie rates of the re-rate); rows and stat
vectors are synthetic (``careers_bench.synthetic_rows``; stats in whole units of 1/256 below
256), since only the fold is timed.  In the same process ``CareerTable.add`` folds the same
windows, and plain torch computes the same two tables: the terms as int64, ``index_add_`` per
player and per cell, ``bucketize`` for the brackets.  The composition's tables must be equal to
``ProfileTable``'s, bit for bit: the script asserts it.  All cases are timed with device events,
interleaved run by run; the medians are printed as one JSON line per window.
``ns_per_slot`` = time / (M * 2K).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.ops.careers import CareerTable  # noqa: E402
from analyzer_amd.ops.profiles import ProfileTable  # noqa: E402
from analyzer_amd.ops.synth import StreamSpec, make_stream  # noqa: E402

from careers_bench import synthetic_rows, timed  # noqa: E402


def synthetic_stats(M, K, seed, dev):
    """Stat vectors [M, 2K, 8]: whole units of 1/256 in [0, 256)."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    i = torch.randint(1 << 16, (M, 2 * K, 8), generator=gen, device=dev, dtype=torch.int32)
    return i.to(torch.float32) / 256


def torch_profiles(rec, rows, stats, P, K, edges):
    """(games, wins [P], sums [P, 8], cells flat with the two counters) with torch ops alone
    (occupied slots are all in range and on a mode in these windows)."""
    S, M = 2 * K, rec.shape[0]
    dev = rec.device
    B = edges.numel() + 1
    ids = rec[:, :S].reshape(-1).to(torch.int64)
    rated = ((rows.view(torch.int32)[:, 5 * S + 1] & 0xFF) == 0).repeat_interleave(S)
    pos = torch.arange(S, device=dev).repeat(M)
    n = torch.where(pos < K, ((rec[:, S] >> 8) & 0xFF).repeat_interleave(S),
                    ((rec[:, S] >> 16) & 0xFF).repeat_interleave(S))
    game = rated & (torch.where(pos < K, pos, pos - K) < n)
    win = torch.where(pos < K, (rec[:, S + 1] & 1).repeat_interleave(S),
                      ((rec[:, S + 1] >> 1) & 1).repeat_interleave(S)).to(torch.int64)
    mode = (rec[:, S] & 0xFF).repeat_interleave(S).to(torch.int64)
    x = stats.reshape(-1, 8)
    good = torch.isfinite(x) & (x >= 0) & (x <= 2.0 ** 30)
    terms = torch.where(good, torch.round(x.to(torch.float64) * 256), 0.0).to(torch.int64)  # ties to even
    counted = torch.cat([game.to(torch.int64)[:, None], (game & (win == 1)).to(torch.int64)[:, None],
                         terms * game[:, None]], dim=1)
    rows_of = torch.where(game, ids, P)
    players = torch.zeros((P + 1, 10), dtype=torch.int64, device=dev).index_add_(0, rows_of, counted)
    score = (rows[:, :S] - rows[:, S:2 * S]).reshape(-1) + 0.0
    bracket = torch.bucketize(score, edges.to(dev), right=True)  # the number of edges <= score
    inside = game & ~torch.isnan(score)
    cell = torch.where(inside, (mode * B + bracket) * 2 + win, 6 * B * 2)
    ones = torch.cat([inside.to(torch.int64)[:, None], terms * inside[:, None]], dim=1)
    cells = torch.zeros((6 * B * 2 + 1, 9), dtype=torch.int64, device=dev).index_add_(0, cell, ones)
    counters = torch.stack([(~good & game[:, None]).sum(), (game & torch.isnan(score)).sum()])
    return players[:P, 0], players[:P, 1], players[:P, 2:], torch.cat([cells[:-1].reshape(-1), counters])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=float, default=1e7)
    ap.add_argument("--team", type=int, default=3)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", default="uniform_1M,uniform_10M,hot")
    ap.add_argument("--only", choices=["both", "native"], default="both",
                    help="native: profiles and careers, no torch comparator (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("profiles_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    M, K = int(args.matches), args.team
    S = 2 * K
    shapes = {"uniform_1M": (1_000_000, False), "uniform_10M": (10_000_000, False), "hot": (1_000_000, True)}
    windows = {}
    for name in args.windows.split(","):
        P, hot = shapes[name]
        rec = make_stream(StreamSpec(team_size=K, seed=41), M, P, K=K, device=dev)
        if hot:
            rec[:, 0] = 0
        windows[name] = (rec, synthetic_rows(rec, K, seed=43), synthetic_stats(M, K, 47, dev), P)
    # timed: the window added to a table that exists (again and again: the cost is the same)
    profs = {name: ProfileTable(w[3], dev) for name, w in windows.items()}
    careers = {name: CareerTable(w[3], dev) for name, w in windows.items()}
    cases = {}
    lines = {name: {"window": name, "matches": M, "team_size": K, "players": w[3], "runs": args.runs}
             for name, w in windows.items()}
    for name, (rec, rows, stats, P) in windows.items():
        cases["profiles_" + name] = lambda w=windows[name], t=profs[name]: t.add(w[0], w[1], w[2]) and None
        cases["careers_" + name] = lambda w=windows[name], t=careers[name]: t.add(w[0], w[1], 0) and None
        if args.only == "both":
            edges = profs[name].edges
            cases["torch_" + name] = lambda w=windows[name], e=edges: torch_profiles(w[0], w[1], w[2], w[3], K, e)
            one = ProfileTable(P, dev).add(rec, rows, stats)
            cols = one.columns()
            games, wins, sums, cells = torch_profiles(rec, rows, stats, P, K, edges)
            equal = (torch.equal(cols["games"].to(torch.int64), games)
                     and torch.equal(cols["wins"].to(torch.int64), wins)
                     and torch.equal(cols["sums"], sums) and torch.equal(one.cells, cells))
            assert equal, "the torch composition and ProfileTable disagree on window %s" % name
            lines[name]["torch_tables_equal"] = bool(equal)
            lines[name]["max_games"] = int(cols["games"].max())
            lines[name]["cells_used"] = int((one.baselines()["games"] > 0).sum())
            del one, cols, games, wins, sums, cells
            torch.cuda.empty_cache()
    for _ in range(args.warmup):
        for fn in cases.values():
            timed(fn)
    times = {k: [] for k in cases}
    for _ in range(args.runs):  # interleaved: every run times each case once
        for k, fn in cases.items():
            times[k].append(timed(fn))
    for name, line in lines.items():
        for label in ("profiles", "careers", "torch"):
            v = times.get(label + "_" + name)
            if not v:
                continue
            line[label + "_ms"] = round(statistics.median(v), 4)
            line[label + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        line["ns_per_slot"] = round(line["profiles_ms"] * 1e6 / (M * S), 4)
        line["profiles_over_careers"] = round(line["profiles_ms"] / line["careers_ms"], 3)
        if "torch_ms" in line:
            line["torch_over_profiles"] = round(line["torch_ms"] / line["profiles_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
