"""Hindsight: how good was this player at that time, given everything known now?  (K16,
csrc/hindsight.hip, csrc/hindsight_core.h)

Everything the engine emits is a *filtered* belief: the (mu, sigma) of a player's 10th match
knows nothing of the 500 matches that followed.  The engine's own model of a track between
two rated matches is a random walk with variance tau^2, which makes smoothing cheap: with
P = sigma^2 and G = P / (P + tau^2), walking a player's rated matches backwards from the
newest one (which is its own smoothed value),

    mu_s[t] = mu[t] + G[t] (mu_s[t+1] - mu[t])
    P_s[t]  = P[t] + G[t]^2 (P_s[t+1] - P[t] - tau^2)

This is the Rauch-Tung-Striebel smoother of each player's own chain, conditional on the
filtered posteriors.  It is **not** TrueSkill-Through-Time: the match factors are not run
again, so a later match tells an earlier one only what it told the player's own track, and
nothing through team mates and opponents.  ``ThroughTime`` (K20, ``ops/through_time.py``) is
that; with zero sweeps it returns what this returns.

    hs = Hindsight(P, device)                       # or track="ranked", ...
    sm = hs.add(rec, rows)                          # windows NEWEST FIRST; fp32 [M, 2K, 2]
    hs.bad                                          # slots skipped for their values
    hs.carry                                        # fp64 [P, 2]: (mu_s, P_s) at the oldest added match

An *element* is a slot that writes in the scorecard's sense (``ops/scorecard.py``): live, its
row rated, the player's last slot in the record.  ``track="shared"`` smooths (s_mu, s_sig) over
the matches of every mode -- tau^2 is added at every rated match whatever its mode --, a mode
name smooths (m_mu, m_sig) over the matches of that mode.  A slot whose (mu, sigma) is not
finite or whose sigma < 0 is skipped and counted in ``bad``.  Every slot that is not an
element gets (NaN, NaN).

The arithmetic is fp64 and the result is rounded once to fp32, so the contract is an error
budget, not bit identity (derived in csrc/hindsight_core.h; docs/ARCHITECTURE.md, K16).  Exact are: a
chain's newest element equals its filtered (mu, sigma); with tau = 0 every element equals the
next newer one; the NaNs; ``bad``.  Device tensors run the HIP kernels, which compose the
steps as affine maps in a segmented scan; CPU tensors run the host mirror, the plain backward
loop.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ..config import RaterConfig
from .careers import _window_chunks
from .matchmake import mode_index
from .native import native

SHARED = "shared"


def track_of(track: str) -> Tuple[int, int]:
    """(HsTrack, mode) of a track name: ``shared`` or a mode."""
    return (0, 0) if track == SHARED else (1, mode_index(track))


class Hindsight:
    """The smoother of ``num_players`` players' chains on ``device``.  ``track``: ``shared`` or
    a mode name; ``cfg``: its ``tau`` is the random walk's step."""

    def __init__(self, num_players: int, device, track: str = SHARED, cfg: Optional[RaterConfig] = None):
        self.num_players = int(num_players)
        if not 0 <= self.num_players < 1 << 31:
            raise ValueError("a hindsight table holds fewer than 2^31 players")
        self.track = track
        self._track, self._mode = track_of(track)
        self.cfg = cfg or RaterConfig()
        self.tau = float(self.cfg.tau)
        if not (math.isfinite(self.tau) and self.tau >= 0.0):
            raise ValueError("tau must be finite and >= 0, got %r" % (self.tau,))
        self.device = torch.device(device)
        self.max_slots = int(native().MAX_SLOTS)  # slots per kernel call; ``add`` splits above it
        self.carry = torch.full((self.num_players, 2), float("nan"), dtype=torch.float64, device=self.device)
        self._bad = torch.zeros(1, dtype=torch.int64, device=self.device)

    @property
    def bad(self) -> int:
        """Slots skipped so far because their (mu, sigma) was not finite or sigma < 0."""
        return int(self._bad.item())

    def add(self, rec: torch.Tensor, rows: torch.Tensor, K: Optional[int] = None,
            max_slots: Optional[int] = None) -> torch.Tensor:
        """Smooth one window: its records ``rec`` [M, 2K+2] and packed output rows ``rows``
        [M, W].  Windows are added NEWEST FIRST.  Returns fp32 [M, 2K, 2], (mu, sigma) per
        slot, NaN where the slot is no element.  A window above the kernels' slot limit is
        split into chunks and the last chunk runs first."""
        k, chunks = _window_chunks(rec, rows, K, int(max_slots or self.max_slots))
        parts = []
        for a, b in reversed(chunks):
            out, bad = native().hindsight_add(self.carry, rec[a:b], rows[a:b], self.tau, self._track, self._mode)
            self._bad += bad
            parts.append(out)
        parts.reverse()
        if len(parts) == 1:
            return parts[0]
        return torch.cat(parts) if parts else torch.empty((0, 2 * k, 2), dtype=torch.float32, device=self.device)


__all__ = ["Hindsight", "track_of", "SHARED"]
