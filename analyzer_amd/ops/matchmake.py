"""Matchmaking: questions about the match not yet played (K12, csrc/matchmake.hip).

    pv  = preview_matches(roster, rec)                     # .status .quality .p_win0
    bal = balance_lobbies(roster, lobbies, mode="ranked")  # .status .split .team0 .records
                                                           # .quality .p_win0 .quality_given
    bal, unmatched = make_lobbies(roster, queue_ids, mode="ranked", K=3)

``preview_matches`` gives, per record of a stream ``rec`` [M, 2K+2] (as for
``BatchRater.rate``), the status and quality ``rate`` would write against the stored
state, and team 0's win probability ``p_win0 = Phi(d / sqrt(n beta^2 + sum sigma^2))`` on
the mode track (NaN unless the status is rated); the winner bits are ignored.
``kErrNumeric`` is reported where a prior or the quality is not finite; the update itself
is not run.

``balance_lobbies`` splits each lobby of 2K players (``lobbies`` [L, 2K], all slots
filled) into two teams of K with the smallest ``|d|``, which is the split of the highest
quality (csrc/matchmake_core.h: splits are K-subsets containing slot 0, ordered by mask;
a tie keeps the lower index; index 0 is the lobby as given).  ``records`` [L, 2K+2] are
ready-to-rate stream records (``fill_winners`` sets the outcome); ``quality_given`` is the
quality of split 0.  Status 8: an id outside [0, P) or a player in two slots; 4 / 5 as in
rating; 7: a prior or ``d`` is not finite; in that precedence.  On an error row split is
-1, team0 0, the floats NaN and the record carries the ids as given.

``make_lobbies`` orders a queue by descending mode-track prior mu (stable: ties keep
queue order), forms lobbies from consecutive runs of 2K, best first, and balances them.

Everything only reads the roster; tag words never matter.  ``roster`` is a ``Roster`` or,
where no seeding is needed, its state tensor (a NULL shared track then gives status 4).
``mode`` is a name of ``config.MODES``, bare or with the ``trueskill_`` prefix.  Device
tensors run the HIP kernels on the current stream, CPU tensors the host mirror (split
choice bit-identical, quality and p_win0 in fp64).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from ..config import MODES, RaterConfig
from ..models.tiers import vst_table
from .native import native

_VST = {}


class Preview(NamedTuple):
    status: torch.Tensor   # uint8 [M]
    quality: torch.Tensor  # fp32 [M]: 0 for AFK / invalid rosters, NaN = not written
    p_win0: torch.Tensor   # fp32 [M]: NaN unless rated


class Balanced(NamedTuple):
    status: torch.Tensor         # uint8 [L]
    split: torch.Tensor          # int32 [L], -1 on error
    team0: torch.Tensor          # int32 [L] bit j = slot j plays in team 0; 0 on error
    records: torch.Tensor        # int32 [L, 2K+2]
    quality: torch.Tensor        # fp32 [L] of the chosen split
    p_win0: torch.Tensor         # fp32 [L]
    quality_given: torch.Tensor  # fp32 [L] of the lobby as given (split 0)


def mode_index(mode: str) -> int:
    """0..5 of a mode name (``ranked`` or ``trueskill_ranked``); ``shared`` is not a mode."""
    if not isinstance(mode, str):
        raise ValueError("a mode is named by a string, got %r" % (mode,))
    name = mode[len("trueskill_"):] if mode.startswith("trueskill_") else mode
    if name not in MODES:
        raise ValueError("unknown mode %r: one of %s" % (mode, ", ".join(MODES)))
    return MODES.index(name)


def geometry(K: int) -> Tuple[int, int, int]:
    """(lanes that share a lobby, lobbies per wave, lobbies per workgroup) of the kernels."""
    return tuple(native().matchmake_geometry(int(K)))


def split_masks(K: int):
    """The team-0 masks of the C(2K-1, K-1) splits of a 2K lobby, in index order."""
    return list(native().split_masks(int(K)))


def fill_winners(records: torch.Tensor, winner: int = 0) -> torch.Tensor:
    """A copy of ``records`` with team ``winner`` (0 or 1; 2: a tie with both bits set) winning."""
    if winner not in (0, 1, 2):
        raise ValueError("winner must be 0, 1 or 2 (tie)")
    out = records.clone()
    out[:, -1] = (out[:, -1] & ~3) | (1, 2, 3)[winner]
    return out


def _operands(roster, cfg: Optional[RaterConfig], dev: torch.device):
    state = roster.state if hasattr(roster, "state") else roster
    attrs = roster.attrs if hasattr(roster, "attrs") else None
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float32:
        raise ValueError("the roster state must be a float32 tensor")
    if state.dim() != 2 or state.shape[1] != 32:
        raise ValueError("the roster state must be [P, 32], got %s" % (tuple(state.shape),))
    if not state.is_contiguous():
        raise ValueError("the roster state must be contiguous")
    if state.shape[0] >= 1 << 31:
        raise ValueError("the roster holds fewer than 2^31 players")
    if state.device != dev:
        raise ValueError("the roster is on %s but the input is on %s" % (state.device, dev))
    if attrs is not None:
        if not isinstance(attrs, torch.Tensor) or attrs.dtype != torch.float32 or attrs.dim() != 2 \
                or tuple(attrs.shape) != (state.shape[0], 4):
            raise ValueError("the roster attrs must be a float32 [P, 4] tensor")
        if not attrs.is_contiguous():
            raise ValueError("the roster attrs must be contiguous")
        if attrs.device != dev:
            raise ValueError("the roster attrs are on %s but the input is on %s" % (attrs.device, dev))
    cfg = cfg or RaterConfig.from_env()
    key = str(dev)
    if key not in _VST:
        _VST[key] = torch.tensor(vst_table(), dtype=torch.float32, device=dev)
    return state, attrs, _VST[key], cfg


def _ids(t, name: str, dim: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise ValueError("%s must be an int32 tensor" % name)
    if t.dim() != dim:
        raise ValueError("%s must have %d dimension%s, got shape %s" % (name, dim, "s" * (dim > 1), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _team_size(K) -> int:
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 5:
        raise ValueError("K must be 1..5, got %r" % (K,))
    return K


def _f32(col: torch.Tensor) -> torch.Tensor:
    return col.contiguous().view(torch.float32)


def preview_matches(roster, rec: torch.Tensor, K: Optional[int] = None,
                    cfg: Optional[RaterConfig] = None) -> Preview:
    """Status, quality and team 0's win probability of every record of ``rec`` against the
    stored roster, which is left untouched."""
    rec = _ids(rec, "rec", 2)
    if K is None:
        if rec.shape[1] < 4 or rec.shape[1] % 2:
            raise ValueError("rec must be [M, 2K+2], got %s" % (tuple(rec.shape),))
        K = (rec.shape[1] - 2) // 2
    K = _team_size(K)
    if rec.shape[1] != 2 * K + 2:
        raise ValueError("rec must be [M, %d] for K = %d, got %s" % (2 * K + 2, K, tuple(rec.shape)))
    state, attrs, vst, cfg = _operands(roster, cfg, rec.device)
    if rec.shape[0] == 0:
        f = torch.empty(0, dtype=torch.float32, device=rec.device)
        return Preview(torch.empty(0, dtype=torch.uint8, device=rec.device), f, f.clone())
    out = native().preview(rec, K, state, attrs, vst, float(cfg.beta) ** 2, float(cfg.unknown_player_sigma))
    return Preview(out[:, 0].to(torch.uint8), _f32(out[:, 1]), _f32(out[:, 2]))


def _empty_balanced(K: int, dev) -> Balanced:
    i = torch.empty(0, dtype=torch.int32, device=dev)
    f = torch.empty(0, dtype=torch.float32, device=dev)
    return Balanced(torch.empty(0, dtype=torch.uint8, device=dev), i, i.clone(),
                    torch.empty((0, 2 * K + 2), dtype=torch.int32, device=dev), f, f.clone(), f.clone())


def balance_lobbies(roster, lobbies: torch.Tensor, mode: str = "ranked",
                    cfg: Optional[RaterConfig] = None) -> Balanced:
    """The best split of every lobby of ``lobbies`` [L, 2K] on ``mode``."""
    lobbies = _ids(lobbies, "lobbies", 2)
    if lobbies.shape[1] % 2 or not 2 <= lobbies.shape[1] <= 10:
        raise ValueError("lobbies must be [L, 2K] with K = 1..5, got %s" % (tuple(lobbies.shape),))
    K = lobbies.shape[1] // 2
    m = mode_index(mode)
    state, attrs, vst, cfg = _operands(roster, cfg, lobbies.device)
    if lobbies.shape[0] == 0:
        return _empty_balanced(K, lobbies.device)
    out, records = native().balance(lobbies, K, state, attrs, vst, m, float(cfg.beta) ** 2,
                                    float(cfg.unknown_player_sigma))
    return Balanced(out[:, 0].to(torch.uint8), out[:, 1].contiguous(), out[:, 2].contiguous(), records,
                    _f32(out[:, 3]), _f32(out[:, 4]), _f32(out[:, 5]))


def queue_order(roster, queue_ids: torch.Tensor, mode: str = "ranked",
                cfg: Optional[RaterConfig] = None) -> Tuple[torch.Tensor, int]:
    """(positions int32 [Q], R): the queue's positions ordered by descending mode-track prior
    mu, ties in queue order; the first R are the players with a valid prior, the rest (ids
    outside [0, P), seeding or sigma errors) keep queue order."""
    queue_ids = _ids(queue_ids, "queue_ids", 1)
    m = mode_index(mode)
    state, attrs, vst, cfg = _operands(roster, cfg, queue_ids.device)
    if queue_ids.shape[0] == 0:
        return queue_ids.clone(), 0
    keys, pos = native().queue_order(queue_ids, state, attrs, vst, m, float(cfg.unknown_player_sigma))
    return pos, int((keys != -1).sum())


def make_lobbies(roster, queue_ids: torch.Tensor, mode: str = "ranked", K: int = 3,
                 cfg: Optional[RaterConfig] = None) -> Tuple[Balanced, torch.Tensor]:
    """Balanced lobbies of 2K from a queue of distinct player ids: ``floor(R / 2K)`` lobbies of
    consecutive players in descending-mu order, best first; ``unmatched`` holds the queue ids of
    the ``R mod 2K`` weakest and then of every failed player.  A repeated id surfaces as status
    8 on the lobby it lands in."""
    K = _team_size(K)
    pos, R = queue_order(roster, queue_ids, mode, cfg)
    S = 2 * K
    n = R // S
    ids = queue_ids.index_select(0, pos.to(torch.int64))
    lobbies = ids[:n * S].reshape(n, S).contiguous()
    return balance_lobbies(roster, lobbies, mode, cfg), ids[n * S:].clone()


__all__ = ["Preview", "Balanced", "preview_matches", "balance_lobbies", "make_lobbies", "queue_order",
           "fill_winners", "mode_index", "geometry", "split_masks"]
