"""Pairs: who plays with and against whom, and how it goes (K15, csrc/pairs.hip,
csrc/pair_core.h).

A *live slot* of a match is an occupied slot whose id lies in [0, P), in a rated match on one
of the selected modes (AFK and invalid-roster matches have no result and are not counted).
An *entry* is an ordered pair of two different live slots holding two different players
(a, b); it is *with* when both slots are on one roster, else *against*, and it is won when
a's roster carries the winner bit.  The pair table holds one row per distinct (a, b), in
ascending order of ``key = a << 32 | b``, with four int32 counters from a's side:
``[with_games, with_wins, vs_games, vs_wins]``.  (b, a) is a row of its own, and a player's
rows are one contiguous range.

    table = PairTable(P, device)                   # or arena.pairs(P, rec_of)
    table.add(rec, rows)                           # any window, in any order
    table.pair(17, 4242)                           # the four counters of one pair
    table.partners(17, "against", top=5)           # whom 17 meets most
    table.duos(20), table.suspects(20, 0.9)        # parties, one-sided rivalries

With ``players`` the table holds the rows of those players only (a filter on a), which is
what keeps a query over a long history small: the unfiltered table has up to 2K(2K - 1) rows
per match, 24 B each.  Every counter is an integer sum, so the table is the same bits on
every run, on the device and in the host mirror, and however the history is cut.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence

import torch

from .careers import modes_mask
from .native import native

COUNTERS = ("with_games", "with_wins", "vs_games", "vs_wins")  # csrc/pair_core.h
RELATIONS = {"with": 0, "against": 2}  # the column of the relation's games; its wins follow
ORDERS = ("games", "win_rate")
MAX_SEGMENTS = 8  # window tables held before they are compacted
MAX_MATCHES = (1 << 31) - 1  # the counters are int32


def _bitmap(player_ids, num_players: int, device) -> torch.Tensor:
    """int32 [ceil(P / 32)] words with bit p & 31 of word p >> 5 set for every player of
    ``player_ids`` inside [0, P)."""
    ids = torch.as_tensor(player_ids, dtype=torch.int64, device=device).reshape(-1)
    ids = torch.unique(ids[(ids >= 0) & (ids < num_players)])
    words = torch.zeros((num_players + 31) // 32, dtype=torch.int64, device=device)
    words.index_add_(0, ids >> 5, torch.ones_like(ids) << (ids & 31))  # distinct bits of a word add up to their OR
    return torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32)


class PairTable:
    """The pair table of ``num_players`` players on ``device``, initially empty.  ``modes``:
    names of the modes whose matches count (None: all); ``players``: keep only the rows of
    these players (None: everybody's); ``max_entries``: entries per kernel call, above which
    ``add`` splits a window (default: the kernels' limit)."""

    def __init__(self, num_players: int, device, modes: Optional[Iterable[str]] = None,
                 players: Optional[Sequence[int]] = None, max_entries: Optional[int] = None):
        self.num_players = int(num_players)
        if not 0 <= self.num_players < 1 << 31:
            raise ValueError("a pair table holds fewer than 2^31 players")
        self.device = torch.device(device)
        self.modes = modes_mask(modes)
        if int(native().PAIR_WORDS) != len(COUNTERS):
            raise RuntimeError("the native library lays a pair row out differently")
        self.max_entries = int(native().MAX_SLOTS) if max_entries is None else int(max_entries)
        if self.max_entries < 1:
            raise ValueError("max_entries must be positive")
        self.bitmap = None if players is None else _bitmap(players, self.num_players, self.device)
        self.matches = 0  # added so far
        self._segments: List[tuple] = []

    # ------------------------------------------------------------ building
    def add(self, rec: torch.Tensor, rows: torch.Tensor, K: Optional[int] = None) -> "PairTable":
        """Add one window: its records ``rec`` [M, 2K+2] and packed output rows ``rows``
        [M, W].  The window's own table is kept as a segment; segments are compacted on a
        query, and at once when more than ``MAX_SEGMENTS`` are held.  A window above
        ``max_entries`` entries is split, which is exact: the counters are sums."""
        if rec.dim() != 2 or rec.shape[1] < 4 or rec.shape[1] % 2:
            raise ValueError("rec must be [M, 2K+2]")
        k = (int(rec.shape[1]) - 2) // 2
        if K is not None and int(K) != k:
            raise ValueError("rec has team size %d, not %d" % (k, int(K)))
        M = int(rec.shape[0])
        if rows.shape[0] != M:
            raise ValueError("rows must hold one row per record")
        if self.matches + M > MAX_MATCHES:
            raise OverflowError("a pair table counts in int32: it holds fewer than 2^31 matches")
        step = max(1, self.max_entries // int(native().PAIR_ENTRIES(k)))
        for a in range(0, M, step):
            b = min(M, a + step)
            keys, counts = native().pairs_window(rec[a:b], rows[a:b], self.num_players, self.modes, self.bitmap)
            if keys.numel():
                self._segments.append((keys, counts))
            if len(self._segments) > MAX_SEGMENTS:
                self.compact()
        self.matches += M
        return self

    def compact(self) -> "PairTable":
        """Merge the segments held into one table (``pairs_merge``)."""
        if len(self._segments) > 1:
            keys, counts = native().pairs_merge([s[0] for s in self._segments], [s[1] for s in self._segments],
                                                max(1, self.num_players))
            self._segments = [(keys, counts)]
        return self

    def _table(self):
        self.compact()
        if not self._segments:
            return (torch.empty(0, dtype=torch.int64, device=self.device),
                    torch.empty((0, len(COUNTERS)), dtype=torch.int32, device=self.device))
        return self._segments[0]

    @property
    def keys(self) -> torch.Tensor:
        """int64 [U], ascending: ``a << 32 | b`` of every distinct pair."""
        return self._table()[0]

    @property
    def counts(self) -> torch.Tensor:
        """int32 [U, 4]: with_games, with_wins, vs_games, vs_wins of the row's a."""
        return self._table()[1]

    # ------------------------------------------------------------ queries
    def _check(self, p: int) -> int:
        p = int(p)
        if not 0 <= p < self.num_players:
            raise ValueError("player ids must lie in [0, %d)" % self.num_players)
        return p

    def _range(self, p: int):
        """[lo, hi): the rows of player p."""
        edges = torch.tensor([p << 32, (p + 1) << 32], dtype=torch.int64, device=self.device)
        lo, hi = torch.searchsorted(self.keys, edges).tolist()
        return lo, hi

    def pair(self, a: int, b: int) -> Dict[str, int]:
        """The four counters of (a, b): zeros if the two never met."""
        a, b = self._check(a), self._check(b)
        keys = self.keys
        key = torch.tensor([(a << 32) | b], dtype=torch.int64, device=self.device)
        i = int(torch.searchsorted(keys, key))
        row = self.counts[i].tolist() if i < keys.numel() and int(keys[i]) == int(key) else [0] * len(COUNTERS)
        return dict(zip(COUNTERS, row))

    def partners(self, p: int, relation: str = "with", top: int = 10, min_games: int = 1,
                 by: str = "games") -> Dict[str, torch.Tensor]:
        """The ``top`` players p played ``with`` or ``against`` at least ``min_games`` times:
        ``player``, ``games`` and ``wins`` (p's), ordered by descending games or win_rate =
        wins / games, ties by ascending partner id."""
        if relation not in RELATIONS:
            raise ValueError("unknown relation %r: one of %s" % (relation, ", ".join(RELATIONS)))
        if by not in ORDERS:
            raise ValueError("unknown order %r: one of %s" % (by, ", ".join(ORDERS)))
        lo, hi = self._range(self._check(p))
        col = RELATIONS[relation]
        ids = (self.keys[lo:hi] & 0xFFFFFFFF).to(torch.int32)
        games, wins = self.counts[lo:hi, col], self.counts[lo:hi, col + 1]
        keep = (games >= max(1, int(min_games))).nonzero().reshape(-1)
        ids, games, wins = ids[keep], games[keep], wins[keep]
        score = games.to(torch.float64) if by == "games" else wins.to(torch.float64) / games.to(torch.float64)
        # the rows ascend in partner id and the sort is stable: ties keep that order
        order = torch.sort(score, descending=True, stable=True).indices[:max(0, int(top))]
        return {"player": ids[order], "games": games[order], "wins": wins[order]}

    def n_partners(self, p: int) -> int:
        """Distinct players p shared a rated match with."""
        lo, hi = self._range(self._check(p))
        return hi - lo

    def _rows(self, keep: torch.Tensor, col: int) -> Dict[str, torch.Tensor]:
        idx = keep.nonzero().reshape(-1)
        games = self.counts[idx, col]
        idx = idx[torch.sort(games, descending=True, stable=True).indices]  # ties by ascending key
        keys = self.keys[idx]
        return {"a": (keys >> 32).to(torch.int32), "b": (keys & 0xFFFFFFFF).to(torch.int32),
                "games": self.counts[idx, col], "wins": self.counts[idx, col + 1]}

    def duos(self, min_games: int = 1) -> Dict[str, torch.Tensor]:
        """The pairs a < b that played together at least ``min_games`` times: ``a``, ``b``,
        ``games`` and ``wins`` (together), most games first, ties by ascending (a, b)."""
        keys, counts = self.keys, self.counts
        keep = ((keys >> 32) < (keys & 0xFFFFFFFF)) & (counts[:, 0] >= max(1, int(min_games)))
        return self._rows(keep, 0)

    def suspects(self, min_games: int, min_win_rate: float) -> Dict[str, torch.Tensor]:
        """The ordered pairs (a, b) that met as opponents at least ``min_games`` times with a
        winning at least ``min_win_rate`` of them: ``a``, ``b``, ``games``, ``wins`` (a's),
        most games first, ties by ascending (a, b)."""
        counts = self.counts
        games = counts[:, 2]
        keep = (games >= max(1, int(min_games))) & (
            counts[:, 3].to(torch.float64) / games.to(torch.float64) >= float(min_win_rate))  # 0 / 0: no
        return self._rows(keep, 2)
