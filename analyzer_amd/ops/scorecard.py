"""Scorecard: are the ratings any good at predicting who wins?  (K14, csrc/score.hip,
csrc/score_core.h)

Scoring a prediction needs the belief *before* each match; the output rows hold only the
state after it.  ``match_priors`` reconstructs the pre-match state of every slot of a window
from the rows themselves -- the previous rated game of the same player supplies it, the
roster the history starts from the rest -- and the scorecard turns the priors into team 0's
win probability (``p_win0`` as ``preview_matches`` defines it) and scores it against the
outcome.

    card = Scorecard(roster)                         # copies the roster's (mu, sigma): the chain table
    res = BatchRater().rate(roster, rec)
    pred = card.add(rec, res.packed, keep=True)      # windows in chronological order
    card.summary()                                   # bits per match, Brier, accuracy, calibration, ECE

``roster`` is the roster the history starts from, *before* it is rated.  The chain table
``[P, 16]`` holds (mu, sigma) per granule, NaN mu = NULL; after every ``add`` it equals the
rated roster's mu / sigma.  A *live* slot is occupied, has its id in [0, P) and a supported
mode; it *writes* the chain when its row is rated and the same player has no later slot in
the record.  The prior of a live slot is the chain state of its player before its match (all
slots of one match see the state before that match): raw shared (mu, sigma) and mode-track
(mu, sigma), NaN where NULL and for slots that are not live.

A match is *scored* when its row is rated, its mode is among ``modes`` and exactly one roster
won; ties are counted, not scored.  A rated match whose priors do not resolve (seeding fails,
a sigma is 0 or the prediction is not finite) is *inconsistent*: the card was not started
from the roster the history started from.

The table is ``[6, 33, 4]`` int64, integer sums only, so it is the same bits on every run and
however the history is cut into windows: per mode 32 calibration bins ``(n, team0_wins,
sum rint(p_win0 * 2^24), spare)`` by ``min(31, int(p_win0 * 32))`` and a last row ``(sum
rint((p_win0 - y)^2 * 2^24), sum nlog2_q20(p_outcome), favourite_won, ties)``; the spare word
of bin 0 counts inconsistent matches, that of bin 1 scored matches with ``p_outcome == 0.5``.
``nlog2_q20(p)`` is -log2(p) * 2^20 by integer operations (``nlog2_q20`` below is the plain
``int`` form).  Device tensors run the HIP kernels, CPU tensors the host mirror (priors bit
identical; p in fp64 there, as ``preview_matches``).
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, NamedTuple, Optional

import torch

from ..config import MODES, RaterConfig
from .careers import modes_mask
from .matchmake import _operands
from .native import native

TRACKS = ("shared", "mode")  # in the order of csrc/score_core.h ScoreTrack
BINS = 32
P_ONE = 1 << 24      # sums of p and of squared errors count in 2^-24
LOG_ONE = 1 << 20    # sums of -log2 p count in 2^-20 bits
NLOG2_CAP = 150 << 20
SPARE_INCONSISTENT, SPARE_COIN = 0, 1
FLAG_SCORED, FLAG_TIE, FLAG_INCONSISTENT, FLAG_COIN, FLAG_TEAM0_WON = (1 << 24 << i for i in range(5))


def nlog2_q20(bits: int) -> int:
    """-log2(p) * 2^20 of the fp32 bit pattern ``bits`` of a p in (0, 1], in plain ``int``
    arithmetic: csrc/score_core.h nlog2_q20, step for step."""
    bits &= 0xFFFFFFFF
    if bits >= 0x3F800000:
        return 0
    e = bits >> 23
    if e == 0:
        return NLOG2_CAP
    x = (0x800000 | (bits & 0x7FFFFF)) << 8
    n = 0
    for _ in range(20):
        y = x * x
        two = y >> 63
        n = (n << 1) | two
        x = y >> 32 if two else y >> 31
    return ((127 - e) << 20) - n


def chain_of(state: torch.Tensor) -> torch.Tensor:
    """The chain table [P, 16] of a roster state [P, 32]: (mu, sigma) of the 8 granules."""
    return state.reshape(-1, 8, 4)[:, :, 0::2].reshape(-1, 16).contiguous()


def _window(rec: torch.Tensor, rows: torch.Tensor) -> int:
    if not isinstance(rec, torch.Tensor) or rec.dtype != torch.int32 or rec.dim() != 2 or rec.shape[1] < 4 \
            or rec.shape[1] % 2:
        raise ValueError("rec must be an int32 [M, 2K+2] tensor")
    K = (int(rec.shape[1]) - 2) // 2
    if not 1 <= K <= 5:
        raise ValueError("K must be 1..5, got %d" % K)
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() != 2 \
            or rows.shape[0] != rec.shape[0]:
        raise ValueError("rows must hold one packed fp32 row per record")
    return K


def match_priors(chain: torch.Tensor, rec: torch.Tensor, rows: torch.Tensor,
                 max_slots: Optional[int] = None) -> torch.Tensor:
    """The priors [M, 4, 2K] fp32 (shared mu, sigma, mode mu, sigma per slot) of one window:
    its records ``rec`` [M, 2K+2] and packed output rows ``rows`` [M, W].  ``chain`` [P, 16]
    is advanced in place to the state after the window.  A window above the kernels' slot
    limit is split into chunks, which is exact."""
    K = _window(rec, rows)
    M = int(rec.shape[0])
    step = max(1, int(max_slots or native().MAX_SLOTS) // (2 * K))
    parts = [native().priors_add(chain, rec[a:min(M, a + step)], rows[a:min(M, a + step)])
             for a in range(0, M, step)]
    out = parts[0] if len(parts) == 1 else torch.cat(parts) if parts else \
        torch.empty((0, 8 * K), dtype=torch.float32, device=chain.device)
    return out.view(M, 4, 2 * K)


class Prediction(NamedTuple):
    status: torch.Tensor     # uint8 [M]: what the priors resolve to (``preview_matches``' status)
    p_win0: torch.Tensor     # fp32 [M]: NaN unless that status is rated
    p_outcome: torch.Tensor  # fp32 [M]: the probability given to the roster that won (NaN: no single winner)
    scored: torch.Tensor     # bool [M]
    flags: torch.Tensor      # int32 [M]: status | mode << 8 | bin << 16 | FLAG_* bits


class Scorecard:
    """The scorecard of a history that starts from ``roster`` (a ``Roster`` or its state
    tensor, on the device the windows live on).  ``track``: ``mode`` -- the track ``quality``
    and ``preview_matches`` use -- or ``shared``; ``modes``: names of the modes whose matches
    count (None: all)."""

    def __init__(self, roster, track: str = "mode", modes: Optional[Iterable[str]] = None,
                 cfg: Optional[RaterConfig] = None):
        if track not in TRACKS:
            raise ValueError("unknown track %r: one of %s" % (track, ", ".join(TRACKS)))
        state = roster.state if hasattr(roster, "state") else roster
        state, self.attrs, self.vst, self.cfg = _operands(roster, cfg, state.device)
        self.device = state.device
        self.num_players = int(state.shape[0])
        self.track = track
        self.modes = modes_mask(modes)
        self.max_slots = int(native().MAX_SLOTS)  # slots per kernel call; ``add`` splits above it
        if int(native().SCORE_BINS) != BINS or int(native().NLOG2_CAP) != NLOG2_CAP:
            raise RuntimeError("the native library lays the scorecard out differently")
        self.chain = chain_of(state)
        self.table = torch.zeros((len(MODES), BINS + 1, 4), dtype=torch.int64, device=self.device)

    def add(self, rec: torch.Tensor, rows: torch.Tensor, keep: bool = False) -> Optional[Prediction]:
        """Score one window: its records ``rec`` [M, 2K+2] and packed output rows ``rows``
        [M, W] (``RateResult.packed``).  Windows are added in chronological order.
        ``keep``: return the per-match ``Prediction``."""
        preds = [pred for _, _, _, pred in self.scored_chunks(rec, rows, keep)]
        return self.prediction(preds) if keep else None

    def scored_chunks(self, rec: torch.Tensor, rows: torch.Tensor, keep: bool = True):
        """``add`` chunk by chunk: for each chunk of at most ``max_slots`` slots, in order, the
        match range and what the kernels made of it, ``(a, b, priors [b - a, 8K], pred rows
        [b - a, 4] int32)`` (``pred`` empty unless ``keep``).  The chain and the table advance
        as the chunks are drawn (K19 folds each chunk's priors and pred before the next)."""
        K = _window(rec, rows)
        M = int(rec.shape[0])
        step = max(1, self.max_slots // (2 * K))
        for a in range(0, M, step):
            b = min(M, a + step)
            priors = native().priors_add(self.chain, rec[a:b], rows[a:b])
            pred = native().score_add(self.table, rec[a:b], priors, rows[a:b], self.attrs, self.vst,
                                      self.num_players, float(self.cfg.beta) ** 2,
                                      float(self.cfg.unknown_player_sigma), TRACKS.index(self.track),
                                      self.modes, bool(keep))
            yield a, b, priors, pred

    def prediction(self, preds) -> Prediction:
        """The ``Prediction`` of the pred rows of consecutive chunks."""
        out = preds[0] if len(preds) == 1 else torch.cat(preds) if preds else \
            torch.empty((0, 4), dtype=torch.int32, device=self.device)
        flags = out[:, 0].contiguous()
        return Prediction((flags & 0xFF).to(torch.uint8), out[:, 1].contiguous().view(torch.float32),
                          out[:, 2].contiguous().view(torch.float32), (flags & FLAG_SCORED) != 0, flags)

    def summary(self) -> Dict:
        """Totals and per mode (the modes with any counted match): ``n`` scored matches,
        ``ties``, ``inconsistent``, ``coin``, ``accuracy`` (favourite won / n), ``brier``,
        ``log_loss`` (nats), ``bits`` per match, the calibration ``bins`` (n, mean p, win
        rate of team 0; the non-empty ones) and ``ece``."""
        t = self.table.cpu().tolist()
        per = {MODES[m]: _summarise([t[m]]) for m in range(len(MODES)) if any(any(r) for r in t[m])}
        out = _summarise(t)
        out["track"] = self.track
        out["modes"] = per
        return out


def _summarise(tables) -> Dict:
    bins = [[sum(t[b][c] for t in tables) for c in range(3)] for b in range(BINS)]
    tail = [sum(t[BINS][c] for t in tables) for c in range(4)]
    n = sum(b[0] for b in bins)
    out = {"n": n, "ties": tail[3], "inconsistent": sum(t[SPARE_INCONSISTENT][3] for t in tables),
           "coin": sum(t[SPARE_COIN][3] for t in tables)}
    if n:
        bits = tail[1] / LOG_ONE / n
        out.update(accuracy=tail[2] / n, brier=tail[0] / P_ONE / n, log_loss=bits * math.log(2.0), bits=bits,
                   ece=sum(abs(b[2] / P_ONE - b[1]) for b in bins) / n)
    else:
        out.update(accuracy=None, brier=None, log_loss=None, bits=None, ece=None)
    out["bins"] = [{"bin": i, "n": b[0], "mean_p": b[2] / P_ONE / b[0], "win_rate": b[1] / b[0]}
                   for i, b in enumerate(bins) if b[0]]
    return out


__all__ = ["Scorecard", "Prediction", "match_priors", "chain_of", "nlog2_q20", "TRACKS", "BINS"]
