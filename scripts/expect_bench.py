"""K19 expectations against K14 scorecard, K13 careers and K17 profiles on the same windows, and
the torch composition a user would write without it.

    python scripts/expect_bench.py [--matches 10000000] [--team 3] [--runs 9]
    python scripts/expect_bench.py --runs 3 --only native   # under a kernel trace

Windows of M KvK matches:

* ``uniform_1M`` / ``uniform_10M``: players drawn uniformly from 1M / 10M;
* ``hot``: one player in slot 0 of every match, the rest uniform over 1M.

The records come from the counter-RNG stream (AFK and tie rates of the re-rate); rows are
synthetic (``careers_bench.synthetic_rows`` plus mode-track fields), since only the folds are
timed.  Timed, interleaved run by run in one process with device events:

* ``expect``         ``Expectations.add``: priors_add + score_add(keep) + expect_add;
* ``add_scored``     ``Expectations.add_scored`` on priors and pred made once: expect_add alone;
* ``scorecard``      ``Scorecard.add`` (what ``expect`` runs before its own kernels);
* ``careers``        ``CareerTable.add``;
* ``profiles``       ``ProfileTable.add``: the same keys / sort / fold with LDS cells and 32-B
                     stat loads instead of the 32-B term store;
* ``torch``          the composition: int64 terms and one ``index_add_`` per column on the same
                     priors and pred (the integer log through ``native().nlog2_q20``).

The composition's table must be equal to ``add_scored``'s, bit for bit: the script asserts it.
The medians are printed as one JSON line per window.  ``ns_per_slot`` = add_scored / (M * 2K).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.ops.careers import CareerTable  # noqa: E402
from analyzer_amd.ops.expectations import COUNTERS, SUMS, Expectations  # noqa: E402
from analyzer_amd.ops.native import native  # noqa: E402
from analyzer_amd.ops.profiles import ProfileTable  # noqa: E402
from analyzer_amd.ops.scorecard import FLAG_SCORED, TRACKS, Scorecard  # noqa: E402
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream  # noqa: E402

from careers_bench import synthetic_rows, timed  # noqa: E402
from profiles_bench import synthetic_stats  # noqa: E402

ONE = 1 << 24


def rows_with_modes(rec, K, seed):
    """``synthetic_rows`` with (m_mu, m_sig) filled in as well: the mode track resolves."""
    S = 2 * K
    rows = synthetic_rows(rec, K, seed)
    gen = torch.Generator(device=rec.device).manual_seed(seed + 1)
    rows[:, 3 * S:4 * S] = torch.randn((rec.shape[0], S), generator=gen, device=rec.device) * 400 + 1500
    rows[:, 4 * S:5 * S] = torch.rand((rec.shape[0], S), generator=gen, device=rec.device) * 300 + 50
    return rows


def torch_expect(rec, priors, pred, P, K, track):
    """(counters [P, 7], sums [P, 8], bad) with torch ops alone (occupied slots are all in range
    and on a mode in these windows)."""
    S, M = 2 * K, rec.shape[0]
    dev = rec.device
    ids = rec[:, :S].to(torch.int64)
    pos = torch.arange(S, device=dev)
    team1 = pos >= K
    n = torch.where(team1[None, :], ((rec[:, S] >> 16) & 0xFF)[:, None], ((rec[:, S] >> 8) & 0xFF)[:, None])
    p = pred[:, 1].contiguous().view(torch.float32)
    scored = ((pred[:, 0] & FLAG_SCORED) != 0) & (p >= 0) & (p <= 1)
    game = scored[:, None] & (torch.where(team1, pos - K, pos)[None, :] < n)
    win = torch.where(team1[None, :], ((rec[:, S + 1] >> 1) & 1)[:, None], (rec[:, S + 1] & 1)[:, None]).to(torch.int64)
    p24 = torch.round(torch.where(scored, p, 0.0).to(torch.float64) * ONE).to(torch.int64)  # ties to even
    q = torch.where(team1[None, :], ONE - p24[:, None], p24[:, None])
    var = (q * (ONE - q)) >> 16
    surprise = native().nlog2_q20(pred[:, 2].contiguous())[:, None].expand(M, S)
    pri = priors.view(M, 4, S)
    raw = pri[:, 0] if track == "shared" else torch.where(torch.isnan(pri[:, 2]), pri[:, 0], pri[:, 2])
    off = torch.isinf(raw) | (raw.abs() > 2.0 ** 20)
    known = game & ~torch.isnan(raw) & ~off
    t = torch.where(known, torch.round(torch.where(known, raw, 0.0).to(torch.float64) * 256), 0.0).to(torch.int64)
    k64 = known.to(torch.int64)
    tsum = torch.stack([t[:, :K].sum(1), t[:, K:].sum(1)], dim=1)
    tcnt = torch.stack([k64[:, :K].sum(1), k64[:, K:].sum(1)], dim=1)
    me = team1.to(torch.int64)
    fav, dog = (q > ONE // 2).to(torch.int64), (q < ONE // 2).to(torch.int64)
    cols = [torch.ones_like(q), win, fav, fav * win, dog, dog * win, k64, q, var, surprise, t,
            tsum[:, me] - t, tcnt[:, me] - k64, tsum[:, 1 - me], tcnt[:, 1 - me]]
    who = torch.where(game, ids, P).reshape(-1)
    g = game.reshape(-1).to(torch.int64)
    out = torch.zeros((len(cols), P + 1), dtype=torch.int64, device=dev)
    for c, col in enumerate(cols):  # one index_add_ per column
        out[c].index_add_(0, who, col.reshape(-1) * g)
    return out[:7, :P].t().contiguous(), out[7:, :P].t().contiguous(), int((game & off).sum())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=float, default=1e7)
    ap.add_argument("--team", type=int, default=3)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", default="uniform_1M,uniform_10M,hot")
    ap.add_argument("--track", default="mode", choices=list(TRACKS))
    ap.add_argument("--only", choices=["both", "native"], default="both",
                    help="native: no torch comparator (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("expect_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    M, K = int(args.matches), args.team
    S = 2 * K
    shapes = {"uniform_1M": (1_000_000, False), "uniform_10M": (10_000_000, False), "hot": (1_000_000, True)}
    labels = ("expect", "add_scored", "scorecard", "careers", "profiles", "torch")
    for name in args.windows.split(","):  # one window at a time: the comparator's int64 columns are large
        P, hot = shapes[name]
        roster = make_roster(RosterSpec(num_players=P, seed=40), device=dev)
        rec = make_stream(StreamSpec(team_size=K, seed=41), M, P, K=K, device=dev)
        if hot:
            rec[:, 0] = 0
        rows = rows_with_modes(rec, K, seed=43)
        stats = synthetic_stats(M, K, 47, dev)
        card = Scorecard(roster, track=args.track)
        chunks = list(card.scored_chunks(rec, rows))
        priors, pred = torch.cat([c[2] for c in chunks]), torch.cat([c[3] for c in chunks])
        del chunks
        line = {"window": name, "matches": M, "team_size": K, "players": P, "runs": args.runs, "track": args.track}
        one = Expectations(roster, track=args.track).add_scored(rec, priors, pred)
        cols = one.columns()
        line["games"] = int(cols["games"].sum())
        line["scored_matches"] = int(((pred[:, 0] & FLAG_SCORED) != 0).sum())
        line["max_games"] = int(cols["games"].max())
        line["bad"] = one.bad
        if args.only == "both":
            cnt, sums, bad = torch_expect(rec, priors, pred, P, K, args.track)
            equal = (all(torch.equal(cols[n].to(torch.int64), cnt[:, i]) for i, n in enumerate(COUNTERS))
                     and all(torch.equal(cols[n], sums[:, i]) for i, n in enumerate(SUMS)) and bad == one.bad)
            assert equal, "the torch composition and Expectations disagree on window %s" % name
            line["torch_tables_equal"] = bool(equal)
            del cnt, sums
        del one, cols
        torch.cuda.empty_cache()
        # timed: the window added to tables that exist (again and again: the cost is the same)
        full, scored = Expectations(roster, track=args.track), Expectations(roster, track=args.track)
        plain, career, prof = Scorecard(roster, track=args.track), CareerTable(P, dev), ProfileTable(P, dev)
        cases = {"expect": lambda: full.add(rec, rows),
                 "add_scored": lambda: scored.add_scored(rec, priors, pred) and None,
                 "scorecard": lambda: plain.add(rec, rows),
                 "careers": lambda: career.add(rec, rows, 0) and None,
                 "profiles": lambda: prof.add(rec, rows, stats) and None}
        if args.only == "both":
            cases["torch"] = lambda: torch_expect(rec, priors, pred, P, K, args.track)
        for _ in range(args.warmup):
            for fn in cases.values():
                timed(fn)
        times = {k: [] for k in cases}
        for _ in range(args.runs):  # interleaved: every run times each case once
            for k, fn in cases.items():
                times[k].append(timed(fn))
        for label in labels:
            v = times.get(label)
            if v:
                line[label + "_ms"] = round(statistics.median(v), 4)
                line[label + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
        line["ns_per_slot"] = round(line["add_scored_ms"] * 1e6 / (M * S), 4)
        line["add_scored_over_profiles"] = round(line["add_scored_ms"] / line["profiles_ms"], 3)
        line["expect_minus_scorecard_ms"] = round(line["expect_ms"] - line["scorecard_ms"], 4)
        if "torch_ms" in line:
            line["torch_over_add_scored"] = round(line["torch_ms"] / line["add_scored_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del full, scored, plain, career, prof, cases, rec, rows, stats, priors, pred, roster
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
