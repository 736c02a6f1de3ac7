"""K20 through time against its neighbours on the same histories: ``Hindsight.add`` (K16, one
backward scan of the same chains) and ``CareerTable.add`` (K13, a fold of the same sorted slots).

    python scripts/through_time_bench.py [--matches 10000000] [--team 3] [--runs 7]

Histories of M KvK matches:

* ``uniform_1M`` / ``uniform_10M``: players drawn uniformly from 1M / 10M;
* ``hot``: one player in slot 0 of every match, the rest uniform over 1M -- one chain of M
  elements across every tile.

The records come from the counter-RNG stream (AFK and tie rates of the re-rate) and are rated by
``BatchRater`` from a generated roster, so the rows are a real filtered history and the priors
resolve.  ``ThroughTime.fit`` is timed with 0, 4 and 8 sweeps; ``fit_ms`` is the whole fit of 8
sweeps (K14 priors, setup, two sorts, nine chain passes, eight match passes), ``setup_ms`` the
fit of 0 sweeps (everything once and one chain pass), ``sweep_ms`` = (fit of 8 - fit of 4) / 4.
All cases are timed with device events in the same process, interleaved run by run; medians and
ranges are printed as one JSON line per history.  ``sweep_ns_per_slot`` = sweep_ms / (M * 2K).
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
from analyzer_amd.ops.rate import BatchRater  # noqa: E402
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream  # noqa: E402
from analyzer_amd.ops.through_time import ThroughTime  # noqa: E402


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
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--windows", default="uniform_1M,uniform_10M,hot")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("through_time_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    M, K = int(args.matches), args.team
    S = 2 * K
    shapes = {"uniform_1M": (1_000_000, False), "uniform_10M": (10_000_000, False), "hot": (1_000_000, True)}
    for name in args.windows.split(","):  # one history at a time: a fit holds ~100 B per slot
        P, hot = shapes[name]
        rec = make_stream(StreamSpec(team_size=K, seed=41), M, P, K=K, device=dev)
        if hot:
            rec[:, 0] = 0
        roster = make_roster(RosterSpec(num_players=P, seed=42), device=dev)
        tt = ThroughTime(roster)
        rows = BatchRater().rate(roster, rec, K).packed
        fit = tt.fit(rec, rows, sweeps=8)
        line = {"window": name, "matches": M, "team_size": K, "players": P, "runs": args.runs,
                "elements": int((~torch.isnan(fit.smoothed[:, :, 1])).sum()), "bad": tt.bad, "flat": tt.flat,
                "inconsistent": tt.inconsistent, "residual": [float("%.3g" % r) for r in fit.residual]}
        del fit
        hs, table = Hindsight(P, dev), CareerTable(P, dev)
        cases = {"fit0": lambda: tt.fit(rec, rows, sweeps=0), "fit4": lambda: tt.fit(rec, rows, sweeps=4),
                 "fit8": lambda: tt.fit(rec, rows, sweeps=8), "hindsight": lambda: hs.add(rec, rows),
                 "careers": lambda: table.add(rec, rows, 0) and None}
        for _ in range(args.warmup):
            for fn in cases.values():
                timed(fn)
        times = {k: [] for k in cases}
        for _ in range(args.runs):  # interleaved: every run times each case once
            for k, fn in cases.items():
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            line[k + "_ms"] = round(med[k], 3)
            line[k + "_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
        line["setup_ms"], line["fit_ms"] = line["fit0_ms"], line["fit8_ms"]
        line["sweep_ms"] = round((med["fit8"] - med["fit4"]) / 4, 3)
        line["sweep_ns_per_slot"] = round(line["sweep_ms"] * 1e6 / (M * S), 4)
        line["sweep_over_hindsight"] = round(line["sweep_ms"] / med["hindsight"], 3)
        line["sweep_over_careers"] = round(line["sweep_ms"] / med["careers"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del tt, hs, table, rows, rec, roster, cases
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
