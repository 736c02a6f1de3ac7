"""Profiles: every player's stat totals and the baselines of each skill bracket, folded from
the match stream joined with its output rows and its telemetry stat vectors (K17,
csrc/profile.hip, csrc/profile_core.h).

A *game* of a player is an occupied slot of a rated match on one of the selected modes; AFK,
invalid and unsupported matches are no games here, because their stats mean nothing.  A game
is won when its own roster carries the winner bit.  Each of the slot's 8 stat values
(``ops/telemetry.py`` ``STAT_NAMES``) adds the integer rint(x * 256) when it is finite with
0 <= x <= 2^30; any other value adds nothing and counts as ``bad``.

The *score* of a game is ``conservative`` = mu - sigma or ``mu`` (ops/ladder.py) of the slot's
record on the ``shared`` track or the match's ``mode`` track.  ``edges`` (up to 31 finite,
strictly ascending fp32 values) cut the scores into B = len(edges) + 1 brackets: the bracket
of a score is the number of edges <= it.  A NaN score has no bracket: the game counts for its
player, not for the baselines, and is counted as ``unbracketed``.

    prof = ProfileTable(P, device)
    prof.add(rec, res.packed, stats)               # any window, any order
    mine = prof.lookup([17, 4242])                 # games, wins, sums, win_rate, per_game
    base = prof.baselines()                        # per (mode, bracket, lost / won)
    prof.compare([17], [1480.0])                   # a player against its bracket

Every sum is an integer, so both tables are the same bits on every run, on the device and in
the host mirror, in any window order and however a window is cut.

    python -m analyzer_amd.ops.profiles --matches N --players P [--team-size K] [--ids a,b]
"""
from __future__ import annotations

import json
from typing import Dict, Iterable, Optional, Sequence, Union

import numpy as np
import torch

from ..config import MODES
from ..models.tiers import vst_table
from .careers import TRACKS, _table_options, _window_chunks, modes_mask
from .ladder import SCORES
from .native import native
from .telemetry import STAT_NAMES

STAT_ONE = 256  # the sums count rint(x * 256) per stat value
MAX_EDGES = 31
WORDS = 20  # a player row: games, wins, 0, 0 and 8 sums as (lo, hi)
CELL = 1 + len(STAT_NAMES)  # a baseline cell: games and 8 sums


def default_edges() -> list:
    """The ``vst_table()`` points of tiers 3, 6, ..., 27: conservative skill is seeded on that
    scale."""
    table = vst_table()
    return [table[t + 1] for t in range(3, 28, 3)]


def _edges(edges) -> torch.Tensor:
    if edges is None:
        edges = default_edges()
    e = np.asarray(list(edges), dtype=np.float64).reshape(-1)
    if e.size > MAX_EDGES:
        raise ValueError("at most %d edges, got %d" % (MAX_EDGES, e.size))
    with np.errstate(over="ignore"):
        f = e.astype(np.float32)
    if not np.isfinite(f).all():
        raise ValueError("edges must be finite fp32 values")
    if f.size > 1 and not (f[1:] > f[:-1]).all():
        raise ValueError("edges must be strictly ascending (as fp32)")
    return torch.from_numpy(f.copy())


def _sums(words: torch.Tensor) -> torch.Tensor:
    w = words[:, 4:].to(torch.int64).reshape(words.shape[0], len(STAT_NAMES), 2)
    return (w[:, :, 0] & 0xFFFFFFFF) | (w[:, :, 1] << 32)


def _per_game(sums: torch.Tensor, games: torch.Tensor) -> torch.Tensor:
    g = games.to(torch.float64).unsqueeze(-1)
    nan = torch.full_like(sums, float("nan"), dtype=torch.float64)
    return torch.where(g > 0, sums.to(torch.float64) / STAT_ONE / g, nan)


class ProfileTable:
    """The profile rows of ``num_players`` players and the baseline table on ``device``,
    initially zero.  ``track``: ``shared`` or ``mode``; ``score``: ``conservative`` or ``mu``;
    ``modes``: names of the modes whose matches count (None: all); ``edges``: the bracket
    edges (None: ``default_edges()``; an empty list: one bracket)."""

    def __init__(self, num_players: int, device, track: str = "shared", score: str = "conservative",
                 modes: Optional[Iterable[str]] = None, edges: Optional[Sequence[float]] = None):
        self.num_players = _table_options("profile", num_players, track, score)
        self.device = torch.device(device)
        self.track, self.score = track, score
        self.modes = modes_mask(modes)
        self.edges = _edges(edges)  # fp32, on the CPU
        self.brackets = int(self.edges.numel()) + 1
        self.max_slots = int(native().MAX_SLOTS)  # slots per kernel call; ``add`` splits above it
        if int(native().PROFILE_WORDS) != WORDS:
            raise RuntimeError("the native library lays a profile row out differently")
        self.table = torch.zeros((self.num_players, WORDS), dtype=torch.int32, device=self.device)
        # [6, B, 2, 9] and the two counters, flat
        self.cells = torch.zeros(len(MODES) * self.brackets * 2 * CELL + 2, dtype=torch.int64, device=self.device)

    def _options(self):
        return (self.num_players, self.track, self.score, self.modes, self.edges.tolist())

    def add(self, rec: torch.Tensor, rows: torch.Tensor, stats: torch.Tensor,
            K: Optional[int] = None) -> "ProfileTable":
        """Fold in one window: its records ``rec`` [M, 2K+2], packed output rows ``rows``
        [M, W] and stat vectors ``stats`` [M, 2K, 8] fp32.  Windows may come in any order.  A
        window above the kernels' slot limit is split into chunks, which is exact."""
        k, chunks = _window_chunks(rec, rows, K, self.max_slots)
        if tuple(stats.shape) != (int(rec.shape[0]), 2 * k, len(STAT_NAMES)):
            raise ValueError("stats must be [M, 2K, %d]" % len(STAT_NAMES))
        for a, b in chunks:
            native().profiles_add(self.table, self.cells, rec[a:b], rows[a:b], stats[a:b], self.num_players,
                                  TRACKS.index(self.track), SCORES.index(self.score), self.modes, self.edges)
        return self

    def merge(self, other: "ProfileTable") -> "ProfileTable":
        """Add the sums of ``other``, a table built with the same options, to this one."""
        if self._options() != other._options():
            raise ValueError("the tables were built with different options")
        sums = _sums(self.table) + _sums(other.table.to(self.device))
        self.table[:, :2] += other.table[:, :2].to(self.device)
        pairs = torch.stack([sums & 0xFFFFFFFF, sums >> 32], dim=2).reshape(self.num_players, -1)
        self.table[:, 4:] = ((pairs + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
        self.cells += other.cells.to(self.device)
        return self

    # ------------------------------------------------------------------ players
    def columns(self) -> Dict[str, torch.Tensor]:
        """``games``, ``wins`` int32 [P]; ``sums`` int64 [P, 8] in units of 1/256, in the
        order of ``STAT_NAMES``."""
        return {"games": self.table[:, 0].contiguous(), "wins": self.table[:, 1].contiguous(),
                "sums": _sums(self.table)}

    def lookup(self, ids: Union[Sequence[int], torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The columns of the given players, plus ``win_rate`` = wins / games and ``per_game``
        = sums / 256 / games [n, 8] (fp64; NaN without a game)."""
        idx = torch.as_tensor(ids, device=self.device).to(torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.num_players):
            raise ValueError("player ids must lie in [0, %d)" % self.num_players)
        words = self.table.index_select(0, idx)
        out = {"games": words[:, 0].contiguous(), "wins": words[:, 1].contiguous(), "sums": _sums(words)}
        games = out["games"].to(torch.float64)
        out["win_rate"] = torch.where(games > 0, out["wins"].to(torch.float64) / games,
                                      torch.full_like(games, float("nan")))
        out["per_game"] = _per_game(out["sums"], out["games"])
        return out

    # ------------------------------------------------------------------ baselines
    @property
    def bad(self) -> int:
        """Stat values of games that were no finite number in [0, 2^30]."""
        return int(self.cells[-2])

    @property
    def unbracketed(self) -> int:
        """Games whose score was a NaN."""
        return int(self.cells[-1])

    def baselines(self) -> Dict[str, torch.Tensor]:
        """``games`` int64 [6, B, 2] and ``sums`` int64 [6, B, 2, 8] per (mode, bracket, lost /
        won), ``per_game`` = sums / 256 / games (fp64; NaN for an empty cell) and ``edges``."""
        cells = self.cells[:-2].view(len(MODES), self.brackets, 2, CELL)
        games, sums = cells[..., 0].contiguous(), cells[..., 1:].contiguous()
        return {"games": games, "sums": sums, "per_game": _per_game(sums, games), "edges": self.edges.clone()}

    def bracket_of(self, scores) -> torch.Tensor:
        """The bracket of each score (fp32): the number of edges <= it; -1 for a NaN."""
        with np.errstate(over="ignore"):
            s = np.asarray(torch.as_tensor(scores).detach().cpu().numpy(), dtype=np.float32).reshape(-1)
        b = np.searchsorted(self.edges.numpy(), s, side="right").astype(np.int64)
        b[np.isnan(s)] = -1
        return torch.from_numpy(b)

    def compare(self, ids, scores, modes: Optional[Iterable[str]] = None) -> Dict[str, torch.Tensor]:
        """Each player's ``per_game`` against the baseline of the bracket holding its score,
        pooled over ``modes`` (None: the table's modes) and both results: ``bracket`` [n],
        ``player`` and ``baseline`` [n, 8] and ``ratio`` = player / baseline (fp64; NaN where a
        side has no game or the score no bracket)."""
        mask = self.modes if modes is None else modes_mask(modes)
        look = self.lookup(ids)
        bracket = self.bracket_of(scores)
        if bracket.numel() != look["games"].numel():
            raise ValueError("one score per player")
        pick = torch.tensor([(mask >> m) & 1 for m in range(len(MODES))], dtype=torch.int64, device=self.device)
        cells = self.cells[:-2].view(len(MODES), self.brackets, 2, CELL)
        pooled = (cells * pick.view(-1, 1, 1, 1)).sum(dim=(0, 2))  # [B, 9]
        at = pooled.index_select(0, bracket.clamp(min=0).to(self.device))
        base = _per_game(at[:, 1:], at[:, 0])
        base[(bracket < 0).to(self.device)] = float("nan")
        return {"bracket": bracket, "player": look["per_game"], "baseline": base, "ratio": look["per_game"] / base}


def profile_lines(table: ProfileTable, ids) -> list:
    """One JSON-ready dict per player of ``ids``."""
    look = {k: v.cpu() for k, v in table.lookup(ids).items()}
    lines = []
    for i, p in enumerate(ids):
        win_rate = float(look["win_rate"][i])
        line = {"profile": int(p), "track": table.track, "score": table.score,
                "games": int(look["games"][i]), "wins": int(look["wins"][i]),
                "win_rate": None if win_rate != win_rate else win_rate}
        for k, name in enumerate(STAT_NAMES):
            v = float(look["per_game"][i, k])
            line["sum_" + name] = int(look["sums"][i, k])
            line[name] = None if v != v else v
        lines.append(line)
    return lines


def baseline_line(table: ProfileTable) -> dict:
    """The non-empty baseline cells as one JSON-ready dict."""
    base = {k: v.cpu() for k, v in table.baselines().items()}
    cells = []
    for m, b, w in base["games"].nonzero().tolist():
        cells.append({"mode": MODES[m], "bracket": b, "won": bool(w), "games": int(base["games"][m, b, w]),
                      "sums": base["sums"][m, b, w].tolist()})
    return {"baselines": cells, "edges": base["edges"].tolist(), "bad": table.bad, "unbracketed": table.unbracketed}


def synthetic_profile(matches: int, players: int, team_size: int, device, seed: int = 2024, **kw) -> ProfileTable:
    """A synthetic roster, stream and telemetry, rated with telemetry and folded."""
    from .rate import BatchRater
    from .synth import RosterSpec, StreamSpec, make_roster, make_stream
    from .telemetry import TelemetrySpec, allocate_stats, make_telemetry

    roster = make_roster(RosterSpec(num_players=players, seed=seed), device=device)
    rec = make_stream(StreamSpec(team_size=team_size, seed=seed + 1), matches, players, device=device)
    tel = make_telemetry(TelemetrySpec(seed=seed + 2), rec, team_size)
    stats = allocate_stats(matches, team_size, device)
    res = BatchRater().rate(roster, rec, team_size, telemetry=(tel.evoff, tel.events, stats))
    return ProfileTable(players, device, **kw).add(rec, res.packed, stats)


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(description="player profiles and bracket baselines of a synthetic stream (K17)")
    ap.add_argument("--matches", type=int, required=True)
    ap.add_argument("--players", type=int, required=True)
    ap.add_argument("--team-size", type=int, default=3)
    ap.add_argument("--ids", default="", metavar="ID[,ID...]", help="players to print (JSON lines)")
    ap.add_argument("--device", default=None, choices=["cpu", "cuda"], help="default: cuda when there is one")
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args(argv)
    ids = [int(p) for p in args.ids.split(",") if p.strip()]
    if args.matches < 0 or args.players < 1 or not 1 <= args.team_size <= 5:
        ap.error("--matches >= 0, --players >= 1 and --team-size in 1..5")
    if any(p < 0 or p >= args.players for p in ids):
        ap.error("--ids must lie in [0, %d)" % args.players)
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    table = synthetic_profile(args.matches, args.players, args.team_size, device, seed=args.seed)
    for line in profile_lines(table, ids):
        print(json.dumps(line))
    print(json.dumps(baseline_line(table)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
