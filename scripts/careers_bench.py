"""K13 careers against the torch composition a user would write without it.

    python scripts/careers_bench.py [--matches 10000000] [--team 3] [--runs 15]
    python scripts/careers_bench.py --runs 3 --only native   # under a kernel trace

Windows of M KvK matches, each folded into a career table (``CareerTable.add``):

* ``uniform_1M`` / ``uniform_10M``: players drawn uniformly from 1M / 10M;
* ``skew2``: ``StreamSpec(skew=2)`` over 10M players (power-law activity);
* ``hot``: one player in slot 0 of every match, the rest uniform over 1M.

The records come from the counter-RNG stream (AFK and tie rates of the re-rate); the rows
are synthetic -- random scores and qualities under a status byte that follows the record --
since only the fold is timed.  The comparator is plain torch on the same inputs: a stable
``sort`` of the slots by player and ``scatter_reduce`` for the fields torch can express
(games, wins, first, last, peak, trough -- not the streaks, nor the match of the peak);
those fields are checked to be equal.  All cases are timed with device events in the same
process, interleaved run by run; the medians are printed as one JSON line per window.
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
from analyzer_amd.ops.rate import RateResult  # noqa: E402
from analyzer_amd.ops.synth import StreamSpec, make_stream  # noqa: E402


def synthetic_rows(rec, K, seed):
    """Packed rows [M, W] for ``rec``: rated unless the record says AFK, random (s_mu, s_sig)
    and quality; everything else zero."""
    S, M = 2 * K, rec.shape[0]
    gen = torch.Generator(device=rec.device).manual_seed(seed)
    rows = torch.zeros((M, RateResult.row_floats(K)), dtype=torch.float32, device=rec.device)
    rows[:, :S] = torch.randn((M, S), generator=gen, device=rec.device) * 400 + 1500
    rows[:, S:2 * S] = torch.rand((M, S), generator=gen, device=rec.device) * 300 + 50
    rows[:, 5 * S] = torch.rand((M,), generator=gen, device=rec.device)
    rows.view(torch.int32)[:, 5 * S + 1] = (rec[:, S + 1] >> 2) & 1  # afk_any -> status AFK
    return rows


def torch_careers(rec, rows, base, P, K):
    """(games, wins, first, last, peak, trough) [P] with torch ops alone (occupied slots are
    all in range in these windows)."""
    S, M = 2 * K, rec.shape[0]
    dev = rec.device
    ids = rec[:, :S].reshape(-1).to(torch.int64)
    rated = ((rows.view(torch.int32)[:, 5 * S + 1] & 0xFF) == 0).repeat_interleave(S)
    pos = torch.arange(S, device=dev).repeat(M)
    n = torch.where(pos < K, ((rec[:, S] >> 8) & 0xFF).repeat_interleave(S),
                    ((rec[:, S] >> 16) & 0xFF).repeat_interleave(S))
    game = rated & (torch.where(pos < K, pos, pos - K) < n)
    win = torch.where(pos < K, (rec[:, S + 1] & 1).repeat_interleave(S),
                      ((rec[:, S + 1] >> 1) & 1).repeat_interleave(S))
    score = (rows[:, :S] - rows[:, S:2 * S]).reshape(-1) + 0.0
    match = base + torch.arange(M, device=dev).repeat_interleave(S)
    order = torch.sort(torch.where(game, ids, P), stable=True).indices  # what a full composition sorts by
    ids, game, win, score, match = (x[order] for x in (torch.where(game, ids, P), game, win, score, match))
    one = game.to(torch.int64)
    games = torch.zeros(P + 1, dtype=torch.int64, device=dev).scatter_add_(0, ids, one)
    wins = torch.zeros(P + 1, dtype=torch.int64, device=dev).scatter_add_(0, ids, one * win)
    big = torch.iinfo(torch.int64).max
    first = torch.full((P + 1,), big, dtype=torch.int64, device=dev).scatter_reduce_(0, ids, match, "amin")
    last = torch.full((P + 1,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, ids, match, "amax")
    inf = float("inf")
    peak = torch.full((P + 1,), -inf, device=dev).scatter_reduce_(0, ids, score, "amax")
    trough = torch.full((P + 1,), inf, device=dev).scatter_reduce_(0, ids, score, "amin")
    none = games[:P] == 0
    nan = torch.full((P,), float("nan"), device=dev)
    return (games[:P], wins[:P], torch.where(none, -1, first[:P]), last[:P], torch.where(none, nan, peak[:P]),
            torch.where(none, nan, trough[:P]))


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
    ap.add_argument("--matches", type=float, default=1e7)
    ap.add_argument("--team", type=int, default=3)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", default="uniform_1M,uniform_10M,skew2,hot")
    ap.add_argument("--only", choices=["both", "native"], default="both",
                    help="native: no comparator (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("careers_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    M, K = int(args.matches), args.team
    S = 2 * K
    shapes = {"uniform_1M": (1_000_000, 1, False), "uniform_10M": (10_000_000, 1, False),
              "skew2": (10_000_000, 2, False), "hot": (1_000_000, 1, True)}
    windows = {}
    for name in args.windows.split(","):
        P, skew, hot = shapes[name]
        rec = make_stream(StreamSpec(team_size=K, seed=41, skew=skew), M, P, K=K, device=dev)
        if hot:
            rec[:, 0] = 0
        windows[name] = (rec, synthetic_rows(rec, K, seed=43), P)
    base = 123_000_000
    fold = lambda rec, rows, P: CareerTable(P, dev).add(rec, rows, base)  # noqa: E731
    # timed: the window added to a table that exists (again and again: the cost is the same)
    tables = {name: CareerTable(w[2], dev) for name, w in windows.items()}
    cases = {name: (lambda w=w, t=tables[name]: t.add(w[0], w[1], base) and None) for name, w in windows.items()}
    lines = {name: {"window": name, "matches": M, "team_size": K, "players": w[2], "runs": args.runs}
             for name, w in windows.items()}
    if args.only == "both":
        for name, (rec, rows, P) in windows.items():
            cases["torch_" + name] = lambda rec=rec, rows=rows, P=P: torch_careers(rec, rows, base, P, K)
            cols = fold(rec, rows, P).columns()
            ref = torch_careers(rec, rows, base, P, K)
            equal = all(torch.equal(cols[f].to(r.dtype).view(torch.int32 if r.dtype == torch.float32 else r.dtype),
                                    r.view(torch.int32 if r.dtype == torch.float32 else r.dtype))
                        for f, r in zip(("games", "wins", "first", "last", "peak", "trough"), ref))
            lines[name]["torch_fields_equal"] = bool(equal)
            lines[name]["max_games"] = int(cols["games"].max())
            del cols, ref
            torch.cuda.empty_cache()
    for _ in range(args.warmup):
        for fn in cases.values():
            timed(fn)
    times = {k: [] for k in cases}
    for _ in range(args.runs):  # interleaved: every run times each case once
        for k, fn in cases.items():
            times[k].append(timed(fn))
    for name, line in lines.items():
        for key, label in ((name, "careers"), ("torch_" + name, "torch")):
            if key not in times:
                continue
            v = times[key]
            line[label + "_ms"] = round(statistics.median(v), 4)
            line[label + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        line["ns_per_slot"] = round(line["careers_ms"] * 1e6 / (M * S), 4)
        if "torch_ms" in line:
            line["torch_over_careers"] = round(line["torch_ms"] / line["careers_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
