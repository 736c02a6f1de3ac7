"""The ladder: every player's rank by score on a track (K11, csrc/ladder.hip).

A track is ``shared`` (``trueskill``) or one of ``config.MODES`` (``ranked`` or
``trueskill_ranked``, as ``Roster.track`` spells them).  The score is computed in
fp32 -- ``conservative`` = mu - sigma, the quantity whose change the reference
records as ``trueskill_delta`` (rater.py:151), or ``mu`` -- with -0 read as +0.  A
player is ranked iff the score is not NaN and ``sigma <= max_sigma`` (inclusive; a
NaN sigma fails), so NULL tracks drop out.  The order is descending score, ties by
ascending player id: a total order, the same on every run and device.  The roster is
only read; its tag words never matter.

    lad = build_ladder(roster, tracks=("shared", "ranked"))
    ids, mu, sigma, score = lad.top("ranked", 10)
    rank, score, pct = lad.lookup("shared", [17, 4242])
    bar = lad.cutoff("shared", 0.01)        # the score that puts a player in the top 1 %

Device rosters run the HIP kernels (one roster read for all requested tracks, a
32-bit radix sort per track); CPU rosters run the bit-identical host mirror.
"""
from __future__ import annotations

from typing import Dict, Iterable, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from ..config import MODES
from .native import native

SCORES = ("conservative", "mu")


def track_index(name: str) -> int:
    """Granule of a track name: 0 = ``shared`` / ``trueskill``, 1.. = ``config.MODES``."""
    if not isinstance(name, str):
        raise ValueError("a track is named by a string, got %r" % (name,))
    if name in ("shared", "trueskill"):
        return 0
    mode = name[len("trueskill_"):] if name.startswith("trueskill_") else name
    if mode not in MODES:
        raise ValueError("unknown track %r: shared or one of %s" % (name, ", ".join(MODES)))
    return 1 + MODES.index(mode)


class _Track(NamedTuple):
    order: torch.Tensor  # int32 [R], best first
    score: torch.Tensor  # fp32 [R], in that order
    rank: torch.Tensor   # int32 [P], -1 = unranked


class Ladder:
    """The ladders ``build_ladder`` built: per track ``order`` (int32 [R], player ids
    from best to worst), ``score`` (fp32 [R], in that order) and ``rank`` (int32 [P], 0
    for the best, -1 for unranked), so ``rank[order[i]] == i``."""

    def __init__(self, state: torch.Tensor, score: str, max_sigma: float, tracks: Dict[int, _Track]):
        self._state = state
        self.score_name = score
        self.max_sigma = max_sigma
        self._tracks = tracks

    @property
    def num_players(self) -> int:
        return int(self._state.shape[0])

    @property
    def tracks(self) -> Tuple[str, ...]:
        return tuple("shared" if t == 0 else MODES[t - 1] for t in sorted(self._tracks))

    def _get(self, track: str) -> _Track:
        t = track_index(track)
        if t not in self._tracks:
            raise ValueError("track %r is not part of this ladder (built: %s)" % (track, ", ".join(self.tracks)))
        return self._tracks[t]

    def ranked(self, track: str) -> int:
        """R: the number of ranked players."""
        return int(self._get(track).order.shape[0])

    def order(self, track: str) -> torch.Tensor:
        return self._get(track).order

    def score(self, track: str) -> torch.Tensor:
        return self._get(track).score

    def rank(self, track: str) -> torch.Tensor:
        return self._get(track).rank

    def top(self, track: str, k: int):
        """The best ``min(k, R)`` players: (ids int32, mu, sigma, score fp32)."""
        tr = self._get(track)
        k = max(0, min(int(k), self.ranked(track)))
        ids = tr.order[:k]
        g = 4 * track_index(track)
        rows = self._state.index_select(0, ids.to(torch.int64))
        return ids, rows[:, g], rows[:, g + 2], tr.score[:k]

    def lookup(self, track: str, ids: Union[Sequence[int], torch.Tensor]):
        """(rank int32, score fp32, percentile fp64) of the given players; percentile =
        1 - rank / R; an unranked player has rank -1, score and percentile NaN."""
        tr = self._get(track)
        dev = tr.rank.device
        idx = torch.as_tensor(ids, device=dev).to(torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.num_players):
            raise ValueError("player ids must lie in [0, %d)" % self.num_players)
        rank = tr.rank.index_select(0, idx)
        ok = rank >= 0
        pos = rank.clamp(min=0).to(torch.int64)
        nan32 = torch.full((idx.numel(),), float("nan"), dtype=torch.float32, device=dev)
        nan64 = nan32.to(torch.float64)
        R = self.ranked(track)
        if R == 0:
            return rank, nan32, nan64
        score = torch.where(ok, tr.score.index_select(0, pos), nan32)
        pct = torch.where(ok, 1.0 - rank.to(torch.float64) / float(R), nan64)
        return rank, score, pct

    def cutoff(self, track: str, q: float) -> float:
        """The score at position floor(q * R): a player needs at least this score to be in
        the top fraction ``q``.  NaN when nobody is ranked; q = 1 gives the last score."""
        if not 0.0 <= q <= 1.0:
            raise ValueError("q must lie in [0, 1]")
        R = self.ranked(track)
        if R == 0:
            return float("nan")
        return float(self._get(track).score[min(int(q * R), R - 1)])


def build_ladder(roster, tracks: Iterable[str] = ("shared",), score: str = "conservative",
                 max_sigma: Optional[float] = None) -> Ladder:
    """Rank every player of ``roster`` (a ``Roster`` or its ``state`` [P, 32]) on each of
    ``tracks``.  ``max_sigma`` (default +inf): players with a larger sigma are unranked."""
    state = roster.state if hasattr(roster, "state") else roster
    if isinstance(tracks, str):
        tracks = (tracks,)
    idx = [track_index(t) for t in tracks]
    if not idx:
        raise ValueError("no track given")
    if score not in SCORES:
        raise ValueError("unknown score %r: one of %s" % (score, ", ".join(SCORES)))
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float32:
        raise ValueError("the roster state must be a float32 tensor")
    if state.dim() != 2 or state.shape[1] != 32:
        raise ValueError("the roster state must be [P, 32], got %s" % (tuple(state.shape),))
    if not state.is_contiguous():
        raise ValueError("the roster state must be contiguous")
    if state.shape[0] >= 1 << 31:
        raise ValueError("the ladder ranks fewer than 2^31 players")
    bound = float("inf") if max_sigma is None else float(max_sigma)
    mask = 0
    for t in idx:
        mask |= 1 << t
    out = native().ladder(state, mask, SCORES.index(score), bound)
    built = {t: _Track(*out[3 * j:3 * j + 3]) for j, t in enumerate(sorted(set(idx)))}
    return Ladder(state, score, bound, built)
