"""K18 islands against K13 careers on the same windows.

    python scripts/islands_bench.py [--matches 10000000] [--team 3] [--runs 9]
    python scripts/islands_bench.py --runs 3 --only native   # under a kernel trace

Windows of M KvK matches from the counter-RNG stream (AFK and tie rates of the re-rate):

* ``p1M_r1`` / ``p10M_r1``: players drawn uniformly from 1M / 10M, one region;
* ``p1M_r8`` / ``p10M_r8``: the same streams in 8 regions (``remap_regions``: match m only
  holds players of region m % 8), so at least 8 islands;
* ``hot``: one player in slot 0 of every match, the rest uniform over 1M: every union meets at
  one root.

Rows are synthetic (``careers_bench.synthetic_rows``), since only the status byte is read.
Timed with device events, run by run interleaved with ``CareerTable.add`` on the same window:
``Islands.add`` into a fresh forest (the reset is not timed), then ``labels()`` (the flatten)
and ``table()`` (the census and the island rows).  Medians are printed as one JSON line per
window, with the number of islands, the largest island's share of matches and the 8-rank
imbalance of ``partition``.  Unless ``--only native`` the device's parent, slots and credit are
asserted equal to the host mirror's on every window.

``--timing-only`` prints the times alone.  It is for the experiment builds of the hook with
its counters alone or its unions alone (``ANA_ISLAND_HOOK_PART`` in csrc/islands.hip, loaded
with ``ANA_NATIVE_LIB``), which compute no islands to summarise.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.ops.careers import CareerTable  # noqa: E402
from analyzer_amd.ops.islands import Islands  # noqa: E402
from analyzer_amd.ops.synth import StreamSpec, make_stream  # noqa: E402

from careers_bench import synthetic_rows, timed  # noqa: E402


def remap_regions(rec, regions):
    """A copy of the stream ``rec`` [M, 2K+2] in which match m only holds players of region
    m % regions: id -> (id // regions) * regions + m % regions (ids < 0 stay).  With P a
    multiple of ``regions`` the ids stay in [0, P)."""
    out = rec.clone()
    S = rec.shape[1] - 2
    m = torch.arange(rec.shape[0], device=rec.device, dtype=torch.int64).unsqueeze(1) % regions
    ids = out[:, :S].to(torch.int64)
    out[:, :S] = torch.where(ids >= 0, ids // regions * regions + m, ids).to(torch.int32)
    return out


def reset(isl):
    """Back to the empty forest, in place."""
    isl.parent.copy_(torch.arange(isl.num_players, dtype=torch.int32, device=isl.device))
    isl.slots.zero_()
    isl.credit.zero_()
    isl.ctrl.zero_()
    isl._dirty()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=float, default=1e7)
    ap.add_argument("--team", type=int, default=3)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", default="p1M_r1,p1M_r8,p10M_r1,p10M_r8,hot")
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--only", choices=["both", "native"], default="both",
                    help="native: no host mirror comparison (kernel-trace runs)")
    ap.add_argument("--timing-only", action="store_true",
                    help="no summary, partition or mirror comparison (experiment builds of the hook)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("islands_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    M, K = int(args.matches), args.team
    S = 2 * K
    shapes = {"p1M_r1": (1_000_000, 1, False), "p1M_r8": (1_000_000, 8, False), "p10M_r1": (10_000_000, 1, False),
              "p10M_r8": (10_000_000, 8, False), "hot": (1_000_000, 1, True)}
    for name in args.windows.split(","):
        P, R, hot = shapes[name]
        rec = make_stream(StreamSpec(team_size=K, seed=41), M, P, K=K, device=dev)
        if R > 1:
            rec = remap_regions(rec, R)
        if hot:
            rec[:, 0] = 0
        rows = synthetic_rows(rec, K, seed=43)
        isl, career = Islands(P, dev), CareerTable(P, dev)
        line = {"window": name, "matches": M, "team_size": K, "players": P, "regions": R, "runs": args.runs}
        times = {"add": [], "labels": [], "table": [], "careers": []}
        for run in range(args.warmup + args.runs):
            reset(isl)
            torch.cuda.synchronize()
            t = {"add": timed(lambda: isl.add(rec, rows) and None), "labels": timed(isl.labels),
                 "table": timed(isl.table), "careers": timed(lambda: career.add(rec, rows, 0) and None)}
            if run >= args.warmup:
                for k, v in t.items():
                    times[k].append(v)
        for k, v in times.items():
            line[k + "_ms"] = round(statistics.median(v), 4)
            line[k + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        line["ns_per_match"] = round(line["add_ms"] * 1e6 / M, 4)
        line["add_over_careers"] = round(line["add_ms"] / line["careers_ms"], 3)
        line["all_over_careers"] = round((line["add_ms"] + line["labels_ms"] + line["table_ms"]) / line["careers_ms"], 3)
        if args.timing_only:
            text = json.dumps(dict(line, timing_only=True))
            print(text, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(text + "\n")
            del rec, rows, isl, career
            torch.cuda.empty_cache()
            continue
        summary = isl.summary()
        line["islands"], line["singletons"], line["players_seen"] = (summary["islands"], summary["singletons"],
                                                                    summary["players_seen"])
        line["largest"] = summary["largest"]
        part = isl.partition(args.ranks)
        line["partition"] = {"ranks": args.ranks, "load": part["load"].tolist(), "imbalance": part["imbalance"]}
        if summary["largest"] and summary["largest"]["share_of_matches"]:
            line["exact_speedup_bound"] = round(1.0 / summary["largest"]["share_of_matches"], 4)
        if args.only == "both":
            host = Islands(P, "cpu").add(rec.cpu(), rows.cpu())
            host.labels(), isl.labels()
            equal = all(torch.equal(getattr(isl, n).cpu(), getattr(host, n)) for n in ("parent", "slots", "credit"))
            assert equal, "the device and the host mirror disagree on window %s" % name
            line["host_mirror_equal"] = bool(equal)
            del host
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del rec, rows, isl, career, part
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
