"""Careers: every player's games, peak and streaks, folded from the match stream joined
with its output rows (K13, csrc/career.hip, csrc/career_core.h).

A *game* of a player is an occupied slot of a match with records (rated, AFK or invalid
rosters) on one of the selected modes.  Only rated games have a score, a result and a
quality; AFK and invalid games are counted and otherwise ignored (they neither extend nor
break a streak).  The score is ``conservative`` = mu - sigma or ``mu`` (ops/ladder.py) of
the slot's record on the ``shared`` track (s_mu, s_sig) or the match's ``mode`` track
(m_mu, m_sig); a NaN score counts as a game but not for peak and trough.  A game is won
when its own roster carries the winner bit.

    table = CareerTable(P, device)                 # or arena.careers(P, rec_of)
    table.add(rec, rows, base)                     # windows in chronological order
    cols = table.columns()                         # games, wins, ..., peak, streak, ...
    mine = table.lookup([17, 4242])                # + win_rate, mean_quality

The table is ``[P, 16]`` int32 words, 64 B per player: integers and copied fp32 bit
patterns only, so it is the same bits on every run, on the device and in the host
mirror, and however the history is cut into windows.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence, Union

import torch

from .ladder import SCORES
from .matchmake import mode_index
from .native import native

TRACKS = ("shared", "mode")  # in the order of csrc/career_core.h CareerTrack
QUALITY_ONE = 1 << 24  # quality_sum counts rint(quality * 2^24) per rated game
# the empty row: no game, no first / last / peak match (-1), peak and trough NaN
EMPTY_ROW = (0, 0, 0, 0, -1, -1, -1, -1, 0x7FC00000, -1, -1, 0x7FC00000, 0, 0, 0, 0)


def modes_mask(modes: Optional[Iterable[str]]) -> int:
    """Bit per mode of ``modes`` (names as ``config.MODES`` spells them); None: every mode."""
    if modes is None:
        return (1 << 6) - 1
    if isinstance(modes, str):
        modes = (modes,)
    mask = 0
    for m in modes:
        mask |= 1 << mode_index(m)
    if not mask:
        raise ValueError("no mode given")
    return mask


def _table_options(noun: str, num_players: int, track: str, score: str) -> int:
    """The options a per-player table (``noun``: career, profile) is built with, checked; the
    player count as an int."""
    if track not in TRACKS:
        raise ValueError("unknown track %r: one of %s" % (track, ", ".join(TRACKS)))
    if score not in SCORES:
        raise ValueError("unknown score %r: one of %s" % (score, ", ".join(SCORES)))
    num_players = int(num_players)
    if not 0 <= num_players < 1 << 31:
        raise ValueError("a %s table holds fewer than 2^31 players" % noun)
    return num_players


def _window_chunks(rec: torch.Tensor, rows: torch.Tensor, K: Optional[int], max_slots: int):
    """The team size of a window ``rec`` [M, 2K+2] with one row of ``rows`` per record, and
    the match ranges (a, b) that cut it into chunks of at most ``max_slots`` slots."""
    if rec.dim() != 2 or rec.shape[1] < 4 or rec.shape[1] % 2:
        raise ValueError("rec must be [M, 2K+2]")
    k = (int(rec.shape[1]) - 2) // 2
    if K is not None and int(K) != k:
        raise ValueError("rec has team size %d, not %d" % (k, int(K)))
    M = int(rec.shape[0])
    if rows.shape[0] != M:
        raise ValueError("rows must hold one row per record")
    step = max(1, max_slots // (2 * k))
    return k, [(a, min(M, a + step)) for a in range(0, M, step)]


def _int64(words: torch.Tensor, lo: int) -> torch.Tensor:
    return (words[:, lo].to(torch.int64) & 0xFFFFFFFF) | (words[:, lo + 1].to(torch.int64) << 32)


def _columns(words: torch.Tensor) -> Dict[str, torch.Tensor]:
    floats = words.view(torch.float32)
    return {"games": words[:, 0].contiguous(), "wins": words[:, 1].contiguous(),
            "afk": words[:, 2].contiguous(), "invalid": words[:, 3].contiguous(),
            "first": _int64(words, 4), "last": _int64(words, 6),
            "peak": floats[:, 8].contiguous(), "peak_match": _int64(words, 9),
            "trough": floats[:, 11].contiguous(),
            "streak": words[:, 12].contiguous(), "best_win": words[:, 13].contiguous(),
            "quality_sum": _int64(words, 14)}


class CareerTable:
    """The career rows of ``num_players`` players on ``device``, initially empty.
    ``track``: ``shared`` or ``mode``; ``score``: ``conservative`` or ``mu``; ``modes``:
    names of the modes whose matches count (None: all)."""

    def __init__(self, num_players: int, device, track: str = "shared", score: str = "conservative",
                 modes: Optional[Iterable[str]] = None):
        self.num_players = _table_options("career", num_players, track, score)
        self.device = torch.device(device)
        self.track, self.score = track, score
        self.modes = modes_mask(modes)
        self.max_slots = int(native().MAX_SLOTS)  # slots per kernel call; ``add`` splits above it
        if int(native().CAREER_WORDS) != len(EMPTY_ROW):
            raise RuntimeError("the native library lays a career row out differently")
        self.table = torch.tensor(EMPTY_ROW, dtype=torch.int64).to(torch.int32).to(self.device).repeat(
            self.num_players, 1)

    def add(self, rec: torch.Tensor, rows: torch.Tensor, base: int, K: Optional[int] = None) -> "CareerTable":
        """Fold in one window: its records ``rec`` [M, 2K+2] and packed output rows
        ``rows`` [M, W], ``base`` the global index of match 0.  Windows are added in
        chronological order.  A window above the kernels' slot limit is split into
        chunks, which is exact: a career does not depend on how its games are cut."""
        for a, b in _window_chunks(rec, rows, K, self.max_slots)[1]:
            native().careers_add(self.table, rec[a:b], rows[a:b], int(base) + a, self.num_players,
                                 TRACKS.index(self.track), SCORES.index(self.score), self.modes)
        return self

    def columns(self) -> Dict[str, torch.Tensor]:
        """Columnar tensors [P]: ``games``, ``wins``, ``afk``, ``invalid``, ``streak``,
        ``best_win`` int32; ``first``, ``last``, ``peak_match``, ``quality_sum`` int64 (-1:
        no such match); ``peak``, ``trough`` fp32 (NaN: none)."""
        return _columns(self.table)

    def lookup(self, ids: Union[Sequence[int], torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The columns of the given players, plus ``win_rate`` = wins / games and
        ``mean_quality`` = quality_sum / 2^24 / games (fp64; NaN without a rated game)."""
        idx = torch.as_tensor(ids, device=self.device).to(torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.num_players):
            raise ValueError("player ids must lie in [0, %d)" % self.num_players)
        out = _columns(self.table.index_select(0, idx))
        games = out["games"].to(torch.float64)
        nan = torch.full_like(games, float("nan"))
        some = games > 0
        out["win_rate"] = torch.where(some, out["wins"].to(torch.float64) / games, nan)
        out["mean_quality"] = torch.where(some, out["quality_sum"].to(torch.float64) / QUALITY_ONE / games, nan)
        return out
