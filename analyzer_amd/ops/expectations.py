"""Expectations: every player's results held up against the model's own pre-match predictions
(K19, csrc/expect.hip, csrc/expect_core.h).

``Scorecard`` says how good the predictions are per mode; this is the same ledger per player:
how many wins the pre-match beliefs gave a player, how many it took, and how strong its team
mates and its opponents were.  A player far above its expectation is what a smurf, a boosted
account or a win trade looks like; ``edge`` answers "are my team mates weaker than my
opponents?"; the surplus by kind of player shows where a ``TAU`` or ``UNKNOWN_PLAYER_SIGMA``
mispredicts.

    exp = Expectations(roster)                    # BEFORE rating: owns a Scorecard (exp.card)
    res = BatchRater().rate(roster, rec)
    exp.add(rec, res.packed)                      # windows in chronological order
    exp.lookup([17, 4242])                        # expected, surplus, sd, z, bits, own / mates / opp means, edge
    exp.outliers(min_games=20, z=3.0)             # who wins far more often than predicted
    exp.fairness(min_games=20)                    # the spread of edge and of the mean win chance

A *game* is a live slot (``ops/scorecard.py``) of a scored match -- rated, on one of the card's
modes, exactly one winner, priors resolved.  Twins are two games.  With P24 = rint(p_win0 *
2^24), a slot of roster 0 has q24 = P24 and one of roster 1 q24 = 2^24 - P24; a game adds

* ``exp`` += q24, ``var`` += (q24 * (2^24 - q24)) >> 16 (2^-32 wins^2), ``surprise`` +=
  ``nlog2_q20(p_outcome)``, ``games``, ``wins``, ``fav`` / ``fav_wins`` (q24 > 2^23) and ``dog``
  / ``dog_wins`` (q24 < 2^23);
* the *strength* rint(mu * 256) of its own slot (``own``, ``own_known``), of the other live
  slots of its roster (``mates``, ``mate_slots``) and of the other roster's (``opp``,
  ``opp_slots``).  The mu is the slot's raw prior on the card's track -- the shared mu, or the
  mode mu and the shared one where that is NULL; there is no seeding.  A NULL (NaN) mu has no
  strength; an infinite mu or one beyond +-2^20 has none either and counts in ``bad``, once per
  game whose own value it is.

Every sum is an integer and nothing is recomputed from the roster, so the table is the same
bits on every run, on the device and in the host mirror, in any order of ``add_scored`` calls
and however a window is cut.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Sequence, Union

import numpy as np
import torch

from ..config import RaterConfig
from .native import native
from .scorecard import TRACKS, Prediction, Scorecard

WORDS = 24  # a player row: 7 counters, 0, and 8 sums as (lo, hi)
COUNTERS = ("games", "wins", "fav", "fav_wins", "dog", "dog_wins", "own_known")
SUMS = ("exp", "var", "surprise", "own", "mates", "mate_slots", "opp", "opp_slots")
Q_ONE = 1 << 24        # exp counts q in 2^-24 wins
VAR_ONE = 1 << 32      # var counts q (1 - q) in 2^-32 wins^2
LOG_ONE = 1 << 20      # surprise counts -log2 p in 2^-20 bits
MU_ONE = 256           # the strengths count rint(mu * 256)
QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)


def _sums(words: torch.Tensor) -> torch.Tensor:
    w = words[:, 8:].to(torch.int64).reshape(words.shape[0], len(SUMS), 2)
    return (w[:, :, 0] & 0xFFFFFFFF) | (w[:, :, 1] << 32)


def _columns(words: torch.Tensor) -> Dict[str, torch.Tensor]:
    out = {name: words[:, i].contiguous() for i, name in enumerate(COUNTERS)}
    sums = _sums(words)
    out.update({name: sums[:, i].contiguous() for i, name in enumerate(SUMS)})
    return out


def _ratio(num: torch.Tensor, den: torch.Tensor, one: float = 1.0) -> torch.Tensor:
    """num / one / den in fp64, NaN where den is 0."""
    d = den.to(torch.float64)
    return torch.where(d != 0, num.to(torch.float64) / one / d, torch.full_like(d, float("nan")))


def _derived(cols: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = dict(cols)
    out["expected"] = cols["exp"].to(torch.float64) / Q_ONE
    out["surplus"] = cols["wins"].to(torch.float64) - out["expected"]
    out["sd"] = torch.sqrt(cols["var"].to(torch.float64) / VAR_ONE)
    out["z"] = _ratio(out["surplus"], out["sd"])
    out["bits"] = _ratio(cols["surprise"], cols["games"], LOG_ONE)
    out["own_mean"] = _ratio(cols["own"], cols["own_known"], MU_ONE)
    out["mates_mean"] = _ratio(cols["mates"], cols["mate_slots"], MU_ONE)
    out["opp_mean"] = _ratio(cols["opp"], cols["opp_slots"], MU_ONE)
    out["edge"] = out["mates_mean"] - out["opp_mean"]
    return out


class Expectations:
    """The expectation rows of the players of ``roster`` (a ``Roster`` or its state tensor, as
    it was *before* the history is rated), initially zero.  ``track``: ``mode`` or ``shared``,
    ``modes``, ``cfg``: as ``Scorecard`` takes them; the card the predictions come from is
    ``card``."""

    def __init__(self, roster, track: str = "mode", modes: Optional[Iterable[str]] = None,
                 cfg: Optional[RaterConfig] = None):
        self.card = Scorecard(roster, track=track, modes=modes, cfg=cfg)
        self.device = self.card.device
        self.num_players = self.card.num_players
        self.track, self.modes = track, self.card.modes
        self.max_slots = self.card.max_slots
        if int(native().EXPECT_WORDS) != WORDS:
            raise RuntimeError("the native library lays an expectation row out differently")
        self.table = torch.zeros((self.num_players, WORDS), dtype=torch.int32, device=self.device)
        self._bad = torch.zeros(1, dtype=torch.int64, device=self.device)

    def add(self, rec: torch.Tensor, rows: torch.Tensor, keep: bool = False) -> Optional[Prediction]:
        """Fold in one window: its records ``rec`` [M, 2K+2] and packed output rows ``rows``
        [M, W] (``RateResult.packed``).  Windows are added in chronological order; the card
        scores them on the way.  ``keep``: return the per-match ``Prediction``."""
        preds = []
        for a, b, priors, pred in self.card.scored_chunks(rec, rows, keep=True):
            native().expect_add(self.table, self._bad, rec[a:b], priors, pred, self.num_players,
                                TRACKS.index(self.track))
            if keep:
                preds.append(pred)
        return self.card.prediction(preds) if keep else None

    def add_scored(self, rec: torch.Tensor, priors: torch.Tensor, pred: torch.Tensor) -> "Expectations":
        """Fold in tensors the caller already has: ``rec`` [M, 2K+2], the raw ``priors``
        [M, 4, 2K] of ``match_priors`` and the pred rows ``pred`` [M, 4] int32 of
        ``score_add(keep=True)``, in any order.  The card is not touched."""
        if rec.dim() != 2 or rec.shape[1] < 4 or rec.shape[1] % 2:
            raise ValueError("rec must be [M, 2K+2]")
        M, K = int(rec.shape[0]), (int(rec.shape[1]) - 2) // 2
        if priors.shape[0] != M or pred.shape[0] != M:
            raise ValueError("priors and pred must hold one row per record")
        step = max(1, self.max_slots // (2 * K))
        for a in range(0, M, step):
            b = min(M, a + step)
            native().expect_add(self.table, self._bad, rec[a:b], priors[a:b], pred[a:b], self.num_players,
                                TRACKS.index(self.track))
        return self

    def merge(self, other: "Expectations") -> "Expectations":
        """Add the sums and counters of ``other``, built with the same options, to this one
        (the cards' tables too; a chain cannot be merged and stays this one's)."""
        if (self.num_players, self.track, self.modes) != (other.num_players, other.track, other.modes):
            raise ValueError("the tables were built with different options")
        sums = _sums(self.table) + _sums(other.table.to(self.device))
        self.table[:, :8] += other.table[:, :8].to(self.device)
        pairs = torch.stack([sums & 0xFFFFFFFF, sums >> 32], dim=2).reshape(self.num_players, -1)
        self.table[:, 8:] = ((pairs + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
        self._bad += other._bad.to(self.device)
        self.card.table += other.card.table.to(self.device)
        return self

    @property
    def bad(self) -> int:
        """Games whose own prior mu was infinite or beyond +-2^20."""
        return int(self._bad[0])

    # ------------------------------------------------------------------ players
    def columns(self) -> Dict[str, torch.Tensor]:
        """The raw integer columns, one entry per player: the int32 counters ``games``,
        ``wins``, ``fav``, ``fav_wins``, ``dog``, ``dog_wins``, ``own_known`` and the int64 sums
        ``exp``, ``var``, ``surprise``, ``own``, ``mates``, ``mate_slots``, ``opp``,
        ``opp_slots``."""
        return _columns(self.table)

    def lookup(self, ids: Union[Sequence[int], torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The columns of the given players, plus (fp64) ``expected`` = exp / 2^24, ``surplus``
        = wins - expected, ``sd`` = sqrt(var / 2^32), ``z`` = surplus / sd (NaN at sd 0),
        ``bits`` = surprise / 2^20 / games, ``own_mean``, ``mates_mean``, ``opp_mean`` (sum /
        256 / count, NaN at count 0) and ``edge`` = mates_mean - opp_mean."""
        idx = torch.as_tensor(ids, device=self.device).to(torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.num_players):
            raise ValueError("player ids must lie in [0, %d)" % self.num_players)
        return _derived(_columns(self.table.index_select(0, idx)))

    def outliers(self, min_games: int = 20, z: float = 3.0, top: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """The players with ``games`` >= ``min_games`` and a z score >= ``z``, best first, ties
        by id (``z`` < 0: the other tail, z score <= ``z``, worst first): ``ids`` int64 and
        their ``z``, ``surplus``, ``games``; ``top``: at most that many."""
        d = _derived(self.columns())
        zs = d["z"]
        hit = (d["games"] >= int(min_games)) & ((zs <= z) if z < 0 else (zs >= z))
        ids = hit.nonzero().reshape(-1)  # ascending: a stable sort keeps ties by id
        order = torch.sort(zs[ids], stable=True, descending=not z < 0).indices
        ids = ids[order] if top is None else ids[order][:max(0, int(top))]
        return {"ids": ids, "z": zs[ids], "surplus": d["surplus"][ids], "games": d["games"][ids]}

    def fairness(self, min_games: int = 20) -> Dict:
        """Over the players with ``games`` >= ``min_games``: ``players``, and for ``edge``
        (mean team mate minus mean opponent strength; the players that have both) and
        ``mean_q`` (the mean win chance the model gave the player) the quantiles 5, 25, 50, 75,
        95 %, the mean and the Pearson correlation with ``games`` (None where undefined)."""
        d = {k: v.cpu().numpy() for k, v in _derived(self.columns()).items()}
        keep = d["games"] >= int(min_games)
        games = d["games"][keep].astype(np.float64)
        out = {"min_games": int(min_games), "players": int(keep.sum())}
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_q = d["expected"][keep] / games
        for name, x in (("edge", d["edge"][keep]), ("mean_q", mean_q)):
            ok = ~np.isnan(x)
            x, g = x[ok], games[ok]
            entry = {"n": int(x.size), "mean": float(x.mean()) if x.size else None,
                     "quantiles": {("q%02d" % round(q * 100)): (float(np.quantile(x, q)) if x.size else None)
                                   for q in QUANTILES}}
            corr = None
            if x.size > 1 and x.std() > 0 and g.std() > 0:
                corr = float(np.corrcoef(x, g)[0, 1])
            entry["games_corr"] = corr
            out[name] = entry
        return out


def _num(v: float):
    return None if v != v or math.isinf(v) else v


def expectation_lines(exp: Expectations, ids) -> list:
    """One JSON-ready dict per player of ``ids``."""
    look = {k: v.cpu() for k, v in exp.lookup(ids).items()}
    lines = []
    for i, p in enumerate(ids):
        line = {"expect": int(p), "track": exp.track}
        for name in COUNTERS + SUMS:
            line[name] = int(look[name][i])
        for name in ("expected", "surplus", "sd", "z", "bits", "own_mean", "mates_mean", "opp_mean", "edge"):
            line[name] = _num(float(look[name][i]))
        lines.append(line)
    return lines


def outliers_line(exp: Expectations, top: int, min_games: int = 20, z: float = 3.0) -> dict:
    """The ``top`` best outliers as one JSON-ready dict."""
    out = {k: v.cpu().tolist() for k, v in exp.outliers(min_games=min_games, z=z, top=top).items()}
    return {"outliers": [{"player": p, "z": _num(zz), "surplus": _num(s), "games": g}
                         for p, zz, s, g in zip(out["ids"], out["z"], out["surplus"], out["games"])],
            "min_games": min_games, "z": z, "track": exp.track, "bad": exp.bad}


__all__ = ["Expectations", "expectation_lines", "outliers_line", "WORDS", "COUNTERS", "SUMS"]
