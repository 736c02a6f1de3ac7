"""K15 pairs against the torch composition a user would write without it.

    python scripts/pairs_bench.py [--matches 10000000] [--team 3] [--runs 7]
    python scripts/pairs_bench.py --runs 3 --only native   # under a kernel trace

Windows of M KvK matches, each turned into a pair table (``PairTable.add`` plus the
compaction of its segments: a 10M-match 3v3 window is 300M entries, two kernel calls):

* ``uniform_1M`` / ``uniform_10M``: players drawn uniformly from 1M / 10M;
* ``skew2``: ``StreamSpec(skew=2)`` over 10M players (power-law activity);
* ``party``: teams are fixed blocks of K consecutive ids out of 1M players, so pairs really
  repeat;
* ``filtered``: the uniform_1M window with a filter of 1,000 players.

The records come from the counter-RNG stream; the rows are synthetic -- only the status byte
matters, rated unless the record says AFK.  The comparator is plain torch on the same inputs:
the int64 keys of all entries, ``torch.unique`` with the inverse, and ``index_add_`` of the
four counters; it is checked to be equal to the table before anything is timed.  All cases
are timed with device events in the same process, interleaved run by run; the medians are
printed as one JSON line per window.  ``ns_per_entry`` = time / (M * 2K(2K - 1)).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.ops.pairs import PairTable  # noqa: E402
from analyzer_amd.ops.rate import RateResult  # noqa: E402
from analyzer_amd.ops.synth import StreamSpec, make_stream  # noqa: E402


def synthetic_rows(rec, K):
    """Packed rows [M, W] for ``rec``: rated unless the record says AFK; everything else zero."""
    S = 2 * K
    rows = torch.zeros((rec.shape[0], RateResult.row_floats(K)), dtype=torch.float32, device=rec.device)
    rows.view(torch.int32)[:, 5 * S + 1] = (rec[:, S + 1] >> 2) & 1  # afk_any -> status AFK
    return rows


def party_stream(rec, K, P, seed):
    """``rec`` with every roster replaced by a fixed block of K consecutive ids."""
    gen = torch.Generator(device=rec.device).manual_seed(seed)
    teams = torch.randint(P // K, (rec.shape[0], 2), generator=gen, device=rec.device, dtype=torch.int32) * K
    rec = rec.clone()
    rec[:, :2 * K] = (teams[:, :, None] + torch.arange(K, device=rec.device, dtype=torch.int32)).reshape(-1, 2 * K)
    return rec


def torch_pairs(rec, rows, P, K, member=None):
    """(keys, counts) with torch ops alone; ``member``: bool [P], the filter on a."""
    S, dev = 2 * K, rec.device
    pos = torch.arange(S, device=dev)
    ja = pos.repeat_interleave(S - 1)
    jb = torch.cat([torch.cat([pos[:j], pos[j + 1:]]) for j in range(S)])
    ids = rec[:, :S].to(torch.int64)
    m0, m1 = rec[:, S], rec[:, S + 1]
    n = torch.where(pos < K, ((m0 >> 8) & 0xFF)[:, None], ((m0 >> 16) & 0xFF)[:, None])
    rated = ((rows.view(torch.int32)[:, 5 * S + 1] & 0xFF) == 0) & ((m0 & 0xFF) < 6)
    live = (torch.where(pos < K, pos, pos - K) < n) & (ids >= 0) & (ids < P) & rated[:, None]
    if member is not None:
        first = live & member[ids.clamp(0, P - 1)]
    else:
        first = live
    a, b = ids[:, ja], ids[:, jb]
    ok = first[:, ja] & live[:, jb] & (a != b)
    vs = ((ja < K) != (jb < K))[None, :].expand_as(ok)
    win = torch.where(ja < K, (m1 & 1)[:, None], ((m1 >> 1) & 1)[:, None]).to(torch.int32)
    key = ((a << 32) | b)[ok]
    vs, win = vs[ok], win[ok]
    one = torch.ones_like(win)
    zero = torch.zeros_like(win)
    vals = torch.stack([torch.where(vs, zero, one), torch.where(vs, zero, win), torch.where(vs, one, zero),
                        torch.where(vs, win, zero)], dim=1)
    keys, inverse = torch.unique(key, return_inverse=True)
    counts = torch.zeros((keys.shape[0], 4), dtype=torch.int32, device=dev).index_add_(0, inverse, vals)
    return keys, counts


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
    ap.add_argument("--windows", default="uniform_1M,uniform_10M,skew2,party,filtered")
    ap.add_argument("--only", choices=["both", "native"], default="both",
                    help="native: no comparator (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("pairs_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    M, K = int(args.matches), args.team
    E = 2 * K * (2 * K - 1)
    shapes = {"uniform_1M": (1_000_000, 1), "uniform_10M": (10_000_000, 1), "skew2": (10_000_000, 2),
              "party": (1_000_000, 1), "filtered": (1_000_000, 1)}
    windows = {}
    for name in args.windows.split(","):
        P, skew = shapes[name]
        rec = make_stream(StreamSpec(team_size=K, seed=41, skew=skew), M, P, K=K, device=dev)
        if name == "party":
            rec = party_stream(rec, K, P, seed=47)
        players = None
        if name == "filtered":
            players = torch.randperm(P, generator=torch.Generator().manual_seed(53))[:1000].tolist()
        windows[name] = (rec, synthetic_rows(rec, K), P, players)

    def table_of(w):
        t = PairTable(w[2], dev, players=w[3]).add(w[0], w[1])
        return t.keys, t.counts

    def member_of(w):
        if w[3] is None:
            return None
        member = torch.zeros(w[2], dtype=torch.bool, device=dev)
        member[torch.tensor(w[3], device=dev)] = True
        return member

    cases = {name: (lambda w=w: table_of(w)) for name, w in windows.items()}
    lines = {name: {"window": name, "matches": M, "team_size": K, "players": w[2], "entries": M * E,
                    "runs": args.runs} for name, w in windows.items()}
    if args.only == "both":
        for name, w in windows.items():
            member = member_of(w)
            cases["torch_" + name] = lambda w=w, member=member: torch_pairs(w[0], w[1], w[2], K, member)
            keys, counts = table_of(w)
            rkeys, rcounts = torch_pairs(w[0], w[1], w[2], K, member)
            lines[name]["torch_equal"] = bool(torch.equal(keys, rkeys) and torch.equal(counts, rcounts))
            lines[name]["rows"] = int(keys.numel())
            lines[name]["max_games"] = int(counts.max()) if keys.numel() else 0
            del keys, counts, rkeys, rcounts
            torch.cuda.empty_cache()
    for _ in range(args.warmup):
        for fn in cases.values():
            timed(fn)
    times = {k: [] for k in cases}
    for _ in range(args.runs):  # interleaved: every run times each case once
        for k, fn in cases.items():
            times[k].append(timed(fn))
    for name, line in lines.items():
        for key, label in ((name, "pairs"), ("torch_" + name, "torch")):
            if key not in times:
                continue
            v = times[key]
            line[label + "_ms"] = round(statistics.median(v), 3)
            line[label + "_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
        line["ns_per_entry"] = round(line["pairs_ms"] * 1e6 / (M * E), 4)
        if "torch_ms" in line:
            line["torch_over_pairs"] = round(line["torch_ms"] / line["pairs_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
