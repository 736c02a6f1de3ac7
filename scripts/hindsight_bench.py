"""K16 hindsight against its two neighbours on the same windows: ``match_priors`` (K14, the scan
it is modelled on) and ``CareerTable.add`` (K13, a fold of the same sorted slots).

    python scripts/hindsight_bench.py [--matches 10000000] [--team 3] [--runs 15]
    python scripts/hindsight_bench.py --runs 3 --only native   # under a kernel trace

Windows of M KvK matches:

* ``uniform_1M`` / ``uniform_10M``: players drawn uniformly from 1M / 10M;
* ``hot``: one player in slot 0 of every match, the rest uniform over 1M -- one run of M
  elements across every tile.

The records come from the counter-RNG stream (AFK and tie rates of the re-rate); the rows are
synthetic -- random (mu, sigma) on both tracks under a status byte that follows the record --
since only the analytics pass is timed.  ``Hindsight.add`` smooths the window against a carry
table that exists (again and again: the carry moves, the cost does not); ``match_priors``
walks it against a chain table, ``CareerTable.add`` folds it.  All are timed with device
events in the same process, interleaved run by run; medians and ranges are printed as one
JSON line per window.  ``ns_per_slot`` = time / (M * 2K).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.ops.careers import CareerTable  # noqa: E402
from analyzer_amd.ops.hindsight import Hindsight  # noqa: E402
from analyzer_amd.ops.rate import RateResult  # noqa: E402
from analyzer_amd.ops.scorecard import match_priors  # noqa: E402
from analyzer_amd.ops.synth import StreamSpec, make_stream  # noqa: E402


def synthetic_rows(rec, K, seed):
    """Packed rows [M, W] for ``rec``: rated unless the record says AFK, random (mu, sigma) on
    the shared and the mode fields; everything else zero."""
    S, M = 2 * K, rec.shape[0]
    gen = torch.Generator(device=rec.device).manual_seed(seed)
    rows = torch.zeros((M, RateResult.row_floats(K)), dtype=torch.float32, device=rec.device)
    for lo in (0, 3 * S):
        rows[:, lo:lo + S] = torch.randn((M, S), generator=gen, device=rec.device) * 400 + 1500
        rows[:, lo + S:lo + 2 * S] = torch.rand((M, S), generator=gen, device=rec.device) * 300 + 50
    rows.view(torch.int32)[:, 5 * S + 1] = (rec[:, S + 1] >> 2) & 1  # afk_any -> status AFK
    return rows


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
    ap.add_argument("--windows", default="uniform_1M,uniform_10M,hot")
    ap.add_argument("--only", choices=["all", "native"], default="all",
                    help="native: hindsight alone (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("hindsight_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    M, K = int(args.matches), args.team
    S = 2 * K
    shapes = {"uniform_1M": (1_000_000, False), "uniform_10M": (10_000_000, False), "hot": (1_000_000, True)}
    cases, lines = {}, {}
    for name in args.windows.split(","):
        P, hot = shapes[name]
        rec = make_stream(StreamSpec(team_size=K, seed=41), M, P, K=K, device=dev)
        if hot:
            rec[:, 0] = 0
        rows = synthetic_rows(rec, K, seed=43)
        hs = Hindsight(P, dev)
        out = hs.add(rec, rows)
        lines[name] = {"window": name, "matches": M, "team_size": K, "players": P, "runs": args.runs,
                       "elements": int((~torch.isnan(out[:, :, 1])).sum()), "bad": hs.bad}
        del out
        cases["hindsight_" + name] = lambda hs=hs, rec=rec, rows=rows: hs.add(rec, rows)
        if args.only == "all":
            chain = torch.full((P, 16), float("nan"), device=dev)
            table = CareerTable(P, dev)
            cases["priors_" + name] = lambda chain=chain, rec=rec, rows=rows: match_priors(chain, rec, rows)
            cases["careers_" + name] = lambda table=table, rec=rec, rows=rows: table.add(rec, rows, 0) and None
    for _ in range(args.warmup):
        for fn in cases.values():
            timed(fn)
    times = {k: [] for k in cases}
    for _ in range(args.runs):  # interleaved: every run times each case once
        for k, fn in cases.items():
            times[k].append(timed(fn))
    for name, line in lines.items():
        for label in ("hindsight", "priors", "careers"):
            v = times.get(label + "_" + name)
            if v:
                line[label + "_ms"] = round(statistics.median(v), 4)
                line[label + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        line["ns_per_slot"] = round(line["hindsight_ms"] * 1e6 / (M * S), 4)
        if "priors_ms" in line:
            line["hindsight_over_priors"] = round(line["hindsight_ms"] / line["priors_ms"], 3)
            line["hindsight_over_careers"] = round(line["hindsight_ms"] / line["careers_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
