"""K14 scorecard: what one window costs, next to K13 careers on the same window.

    python scripts/scorecard_bench.py [--matches 10000000] [--team 3] [--runs 15]
    python scripts/scorecard_bench.py --runs 3 --only native   # under a kernel trace

Windows of M KvK matches (``careers_bench.py``'s): ``uniform_1M`` / ``uniform_10M`` -- players
drawn uniformly from 1M / 10M -- and ``hot`` -- one player in slot 0 of every match, the rest
uniform over 1M, so one key's run crosses every tile of the scan.

The records come from the counter-RNG stream; the rows are synthetic -- random post-states
under a status byte that follows the record -- since only the scorecard is timed.  Per window:

* ``priors``   ``match_priors``: keys, sort, summaries, stitch, apply (the chain advances, and
               is then whatever the rows say; the cost is the same window after window);
* ``score``    the score kernel alone, from priors computed once;
* ``add``      ``Scorecard.add``: both;
* ``careers``  ``CareerTable.add`` on the same window (``--only native`` leaves it out): the
               sort is the same call, its keys and fold move about half the bytes per slot.

All cases are timed with device events in the same process, interleaved run by run; the
medians are printed as one JSON line per window.  ``ns_per_slot`` = add time / (M * 2K).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.ops.careers import CareerTable  # noqa: E402
from analyzer_amd.ops.native import native  # noqa: E402
from analyzer_amd.ops.rate import RateResult, Roster  # noqa: E402
from analyzer_amd.ops.scorecard import TRACKS, Scorecard, match_priors  # noqa: E402
from analyzer_amd.ops.synth import StreamSpec, make_stream  # noqa: E402


def synthetic_rows(rec, K, seed):
    """Packed rows [M, W] for ``rec``: rated unless the record says AFK, random (s_mu, s_sig)
    and (m_mu, m_sig); everything else zero."""
    S, M = 2 * K, rec.shape[0]
    gen = torch.Generator(device=rec.device).manual_seed(seed)
    rows = torch.zeros((M, RateResult.row_floats(K)), dtype=torch.float32, device=rec.device)
    for f in (0, 3):
        rows[:, f * S:(f + 1) * S] = torch.randn((M, S), generator=gen, device=rec.device) * 400 + 1500
        rows[:, (f + 1) * S:(f + 2) * S] = torch.rand((M, S), generator=gen, device=rec.device) * 300 + 50
    rows.view(torch.int32)[:, 5 * S + 1] = (rec[:, S + 1] >> 2) & 1  # afk_any -> status AFK
    return rows


def rated_roster(P, dev):
    """Every track of every player rated, so no match is inconsistent."""
    roster = Roster.empty(P).to(dev)
    roster.state[:, 0::4] = 1500.0
    roster.state[:, 2::4] = 200.0
    return roster


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
    ap.add_argument("--only", choices=["both", "native"], default="both",
                    help="native: the scorecard alone, no careers (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("scorecard_bench needs a GPU: nothing was measured", file=sys.stderr)
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
        card = Scorecard(rated_roster(P, dev))
        priors = match_priors(card.chain.clone(), rec, rows).view(M, 4 * S)
        beta2, us = float(card.cfg.beta) ** 2, float(card.cfg.unknown_player_sigma)
        cases["priors_" + name] = lambda card=card, rec=rec, rows=rows: match_priors(card.chain, rec, rows)
        cases["score_" + name] = lambda card=card, rec=rec, rows=rows, priors=priors, P=P: native().score_add(
            card.table, rec, priors, rows, card.attrs, card.vst, P, beta2, us, TRACKS.index("mode"), card.modes, False)
        cases["add_" + name] = lambda card=card, rec=rec, rows=rows: card.add(rec, rows)
        if args.only == "both":
            table = CareerTable(P, dev)
            cases["careers_" + name] = lambda table=table, rec=rec, rows=rows: table.add(rec, rows, 0) and None
        card.add(rec, rows)
        summ = card.summary()
        lines[name] = {"window": name, "matches": M, "team_size": K, "players": P, "runs": args.runs,
                       "scored": summ["n"], "inconsistent": summ["inconsistent"]}
    for _ in range(args.warmup):
        for fn in cases.values():
            timed(fn)
    times = {k: [] for k in cases}
    for _ in range(args.runs):  # interleaved: every run times each case once
        for k, fn in cases.items():
            times[k].append(timed(fn))
    for name, line in lines.items():
        for label in ("priors", "score", "add", "careers"):
            v = times.get(label + "_" + name)
            if v:
                line[label + "_ms"] = round(statistics.median(v), 4)
                line[label + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        line["ns_per_slot"] = round(line["add_ms"] * 1e6 / (M * S), 4)
        if "careers_ms" in line:
            line["add_over_careers"] = round(line["add_ms"] / line["careers_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
