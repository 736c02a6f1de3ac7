"""Through time: how good was this player then, given everything known now -- answered jointly.
(K20, csrc/ttt.hip, csrc/ttt_core.h)

``Hindsight`` (K16) smooths every player's own chain and never runs a match factor again, so a
later match reaches an earlier one only through that player.  This is the full answer,
TrueSkill-Through-Time: expectation propagation over the whole history, where every match
factor is re-run against the smoothed beliefs of everyone in it until the curves stop moving.

    tt = ThroughTime(roster)                          # BEFORE rating: copies the chain table
    res = BatchRater().rate(roster, rec)
    fit = tt.fit(rec, res.packed, sweeps=8)
    fit.smoothed                                      # fp32 [M, 2K, 2], NaN where no element
    fit.residual, fit.sweeps                          # max |d mu| per sweep; sweeps run
    tt.final()                                        # fp64 [P, 2] at each player's newest element
    tt.bad, tt.flat, tt.inconsistent

The model.  Elements are ``Hindsight``'s: live, the row rated, the player's last slot of the
record, on a mode track the match of that mode, finite values (else ``bad``).  A player's chain
is its elements in order: s_0 ~ N(m0, sigma0^2) -- the resolved pre-match prior of its first
element, as the scorecard resolves it -- and a random walk of variance tau^2 before every
element.  A rated match whose priors do not resolve has no elements and counts in
``inconsistent`` (the object was not started from the roster the history started from); a
match with a bad slot keeps the filter's own messages for its other elements.  Every element
holds a likelihood message; it starts as the filter's own (posterior over walked prior;
``flat`` counts those that come out negative and start at nothing).  A *sweep* is a chain pass
-- forward and backward messages of every chain, hence every element's cavity and marginal --
followed by a match pass, where every match recomputes the messages of its elements from the
cavities with the rater's closed-form two-team update (no tau there: it is in the chain).  All
matches read the cavities of the same chain pass (a Jacobi schedule).  ``fit(sweeps=S)`` runs S
sweeps and a final chain pass; ``residual[k]`` is the largest move of a marginal mean between
chain pass k and k + 1; ``tol`` stops after the chain pass whose residual is below it.
Convergence of the parallel schedule is not proven -- the residuals are there to be looked at
--, ``damping`` in (0, 1] mixes old and new messages in natural parameters.

With ``sweeps=0`` the result is ``Hindsight``'s up to rounding.  One history per ``fit``, at
most ``MAX_SLOTS`` slots.  Device tensors run the HIP kernels (both chain directions as
segmented scans over a Kalman element), CPU tensors the host mirror (the plain recursions);
the arithmetic is fp64, the curves are rounded once to fp32 (docs/ARCHITECTURE.md, K20).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional

import torch

from ..config import RaterConfig
from .hindsight import SHARED, track_of
from .matchmake import _operands
from .native import native
from .scorecard import _window, chain_of


class Fit(NamedTuple):
    smoothed: torch.Tensor   # fp32 [M, 2K, 2]: (mu, sigma) per slot, NaN where the slot is no element
    residual: List[float]    # per sweep run: max |d mu| of a marginal between two chain passes
    sweeps: int              # sweeps actually run


class ThroughTime:
    """The joint re-estimate of a history that starts from ``roster`` (a ``Roster`` or its state
    tensor, on the device the history lives on), taken BEFORE it is rated.  ``track``:
    ``shared`` or a mode name; ``cfg``: its ``beta``, ``tau`` and ``unknown_player_sigma``."""

    def __init__(self, roster, track: str = SHARED, cfg: Optional[RaterConfig] = None):
        if not isinstance(track, str):
            raise ValueError("track must be a name: %r or a mode" % SHARED)
        self.track = track
        self._track, self._mode = track_of(track)
        state = roster.state if hasattr(roster, "state") else roster
        state, attrs, self.vst, self.cfg = _operands(roster, cfg, state.device)
        self.device = state.device
        self.num_players = int(state.shape[0])
        self.attrs = None if attrs is None else attrs.clone()
        self.tau = float(self.cfg.tau)
        if not (math.isfinite(self.tau) and self.tau >= 0.0):
            raise ValueError("tau must be finite and >= 0, got %r" % (self.tau,))
        self.max_slots = int(native().MAX_SLOTS)
        self.chain = chain_of(state)
        self.bad = self.flat = self.inconsistent = 0
        self._last = None

    def fit(self, rec: torch.Tensor, rows: torch.Tensor, sweeps: int = 8, tol: Optional[float] = None,
            damping: float = 1.0) -> Fit:
        """Re-estimate one history: its records ``rec`` [M, 2K+2] and packed output rows
        ``rows`` [M, W] (``RateResult.packed``), the whole of it in one call."""
        K = _window(rec, rows)
        if rec.device != self.device or rows.device != self.device:
            raise ValueError("the history is on %s / %s but the roster on %s" % (rec.device, rows.device, self.device))
        M = int(rec.shape[0])
        if M * 2 * K > self.max_slots:
            raise ValueError("a history of %d slots is above the limit of %d slots (MAX_SLOTS) of one fit"
                             % (M * 2 * K, self.max_slots))
        if isinstance(sweeps, bool) or not isinstance(sweeps, int) or not 0 <= sweeps <= 1 << 20:
            raise ValueError("sweeps must be an int in 0..2^20, got %r" % (sweeps,))
        damping = float(damping)
        if not 0.0 < damping <= 1.0:
            raise ValueError("damping must lie in (0, 1], got %r" % (damping,))
        if tol is not None and not (float(tol) >= 0.0):
            raise ValueError("tol must be >= 0 or None, got %r" % (tol,))
        chain = self.chain.clone()  # one history per fit: every fit starts from the roster
        priors = native().priors_add(chain, rec, rows)
        out, resid, cav, msg, counters = native().ttt_fit(
            rec, rows, priors, self.attrs, self.vst, self.num_players, float(self.cfg.beta) ** 2, self.tau,
            float(self.cfg.unknown_player_sigma), self._track, self._mode, sweeps,
            -1.0 if tol is None else float(tol), damping)
        self.bad, self.flat, self.inconsistent = (int(c) for c in counters.tolist())
        self._last = (rec, out, cav, msg)
        residual = [float(x) for x in resid.tolist()]
        return Fit(out, residual, len(residual))

    def final(self) -> torch.Tensor:
        """fp64 [P, 2]: the marginal (mu, sigma) at each player's newest element of the last
        ``fit``, NaN for a player without one."""
        res = torch.full((self.num_players, 2), float("nan"), dtype=torch.float64, device=self.device)
        if self._last is None:
            return res
        rec, out, cav, msg = self._last
        S = int(out.shape[1])
        slot = (~torch.isnan(out[:, :, 0]).reshape(-1)).nonzero().reshape(-1)
        if slot.numel() == 0:
            return res
        player = rec[:, :S].reshape(-1)[slot].long()
        newest = torch.full((self.num_players,), -1, dtype=torch.int64, device=self.device)
        newest.scatter_reduce_(0, player, slot, "amax")
        who = (newest >= 0).nonzero().reshape(-1)
        at = newest[who]
        pc = 1.0 / cav[at, 1]
        pm = pc + msg[at, 1]
        res[who, 0] = (cav[at, 0] * pc + msg[at, 0]) / pm
        res[who, 1] = torch.sqrt(1.0 / pm)
        return res


__all__ = ["ThroughTime", "Fit"]
