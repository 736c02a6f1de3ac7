"""K12 matchmaking against the torch composition a user would write without it.

    python scripts/matchmake_bench.py [--players 10000000] [--lobbies 1000000] [--teams 3,5] [--runs 25]
    python scripts/matchmake_bench.py --runs 3 --only native   # under a kernel trace

Per team size: ``balance_lobbies`` and ``preview_matches`` over L lobbies of player ids drawn
uniformly from a P-player roster, the torch comparator, and ``index_select`` of whole roster
rows (the device's random 128-B gather rate, the floor the kernels can approach) are timed
with device events in the same process, interleaved run by run; the medians are printed as
one JSON line per team size.

The comparator is plain torch: ``index_select`` of the rows, a +-1 sign matrix [C, 2K] times
the mus, ``abs``, ``argmin``, and the closed-form quality and win probability.  Its fp32
matmul sums in another order than the kernel, so its choice is not bit-comparable:
``split_agreement`` is the share of lobbies on which both choose the same split (the GPU
tests are the correctness yardstick; the comparator is only for time).

``line_rate_GBps`` = L * 2K * 128 B / time: every player costs one roster line.
"""
import argparse
import itertools
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from analyzer_amd.config import RaterConfig  # noqa: E402
from analyzer_amd.ops.matchmake import balance_lobbies, preview_matches  # noqa: E402
from analyzer_amd.ops.synth import RosterSpec, make_roster  # noqa: E402

MODE = 1  # ranked


def sign_matrix(K, device):
    """[C, 2K] of +-1: the splits (K-subsets containing slot 0) in ascending mask order."""
    subsets = sorted((sum(1 << j for j in c), c) for c in itertools.combinations(range(2 * K), K) if 0 in c)
    m = -torch.ones((len(subsets), 2 * K), dtype=torch.float32)
    for i, (_, c) in enumerate(subsets):
        m[i, list(c)] = 1.0
    return m.to(device)


def torch_balance(state, lobbies, signs, beta2):
    """(split, quality, p_win0, quality_given) with torch ops alone; the roster is fully rated,
    so the priors are the stored values."""
    L, S = lobbies.shape
    rows = state.index_select(0, lobbies.reshape(-1).to(torch.int64)).view(L, S, 32)
    mu, sig = rows[:, :, 4 * (1 + MODE)], rows[:, :, 4 * (1 + MODE) + 2]
    d = mu @ signs.t()
    split = d.abs().argmin(dim=1)
    den = S * beta2 + (sig * sig).sum(dim=1)
    db = d.gather(1, split[:, None])[:, 0]
    scale = torch.sqrt(S * beta2 / den)
    q = scale * torch.exp(-db * db / (2 * den))
    qg = scale * torch.exp(-d[:, 0] * d[:, 0] / (2 * den))
    p = 0.5 * torch.erfc(-db / torch.sqrt(den) * 0.7071067811865476)
    return split, q, p, qg


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
    ap.add_argument("--players", type=float, default=1e7)
    ap.add_argument("--lobbies", type=float, default=1e6)
    ap.add_argument("--teams", default="3,5")
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["both", "native"], default="both",
                    help="native: no comparator and no gather (kernel-trace runs)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("matchmake_bench needs a GPU: nothing was measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    P, L = int(args.players), int(args.lobbies)
    cfg = RaterConfig()
    beta2 = float(cfg.beta) ** 2
    roster = make_roster(RosterSpec(num_players=P, seed=5, p_rated=1.0, p_mode_rated=1.0), device=dev)
    for K in [int(k) for k in args.teams.split(",")]:
        S = 2 * K
        gen = torch.Generator(device=dev).manual_seed(100 + K)
        lobbies = torch.randint(0, P, (L, S), generator=gen, device=dev, dtype=torch.int32)
        bal = balance_lobbies(roster, lobbies, "ranked", cfg=cfg)
        rec = bal.records
        flat = lobbies.reshape(-1).to(torch.int64)
        cases = {"balance": lambda: balance_lobbies(roster, lobbies, "ranked", cfg=cfg),
                 "preview": lambda: preview_matches(roster, rec, cfg=cfg)}
        line = {"team_size": K, "players": P, "lobbies": L, "runs": args.runs,
                "status": {str(int(v)): int(c) for v, c in zip(*torch.unique(bal.status, return_counts=True))}}
        if args.only == "both":
            signs = sign_matrix(K, dev)
            cases["torch"] = lambda: torch_balance(roster.state, lobbies, signs, beta2)
            cases["gather"] = lambda: roster.state.index_select(0, flat)
            split, q, p, qg = torch_balance(roster.state, lobbies, signs, beta2)
            ok = bal.status == 0
            line["split_agreement"] = round(float((split[ok] == bal.split[ok]).double().mean()), 6)
            line["max_quality_diff"] = float((q[ok] - bal.quality[ok]).abs().max())
            del split, q, p, qg
        for _ in range(args.warmup):
            for fn in cases.values():
                timed(fn)
        times = {k: [] for k in cases}
        for _ in range(args.runs):  # interleaved: every run times each case once
            for k, fn in cases.items():
                times[k].append(timed(fn))
        gathered = L * S * 128
        for k, v in times.items():
            med = statistics.median(v)
            line[k + "_ms"] = round(med, 4)
            line[k + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
            line[k + "_line_rate_GBps"] = round(gathered / med / 1e6, 1)
        if args.only == "both":
            line["torch_over_balance"] = round(line["torch_ms"] / line["balance_ms"], 3)
            line["balance_over_gather"] = round(line["balance_ms"] / line["gather_ms"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        del cases, lobbies, bal, rec, flat
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
