"""Device-resident record arena of a re-rate and player-history queries over it.

The product of a full-history re-rate (runtime/rerate.py) is the per-participant
record of every rated match: shared mu / sigma / delta, mode mu / sigma and the match
quality, one packed row per match (``RateResult.row_floats``: 128 B for K <= 3, 256 B
for K = 4, 5).  ``records="resident"`` keeps them where the executor writes them:

* ``RecordArena`` is one ``[matches, W]`` fp32 tensor (``torch.empty``, never
  zero-filled, indexed by int64 rows: 1B matches x 32 floats exceed 2^31 elements).
  ``result(lo, hi)`` hands out ``RateResult`` views of its own memory, so a window is
  rated straight into its slice -- no copy, no double buffer.  The arena tracks its
  filled extent; reading rows that were never filled raises.
* On N ranks (time-axis sharding) rank r rates block r of every global window
  (``window_slice``); its arena stores its blocks back to back, and ``global_match`` /
  ``local_row`` map between a local row and the global match index.
* ``history(player_ids, num_players, rec_of)`` answers "what did these players' ratings
  do over time".  The rows hold no player ids -- those live in the match stream -- so
  each filled window's records (``rec_of(lo, hi)``: regenerated from the counter-RNG
  stream, nothing but the arena is kept) are joined with its rows by the
  ``records_select`` kernel (csrc/select.hip, K10) against a bitmap of the queried
  players; hits come out in ascending (match, slot) order, the same bits on every run.
  On N ranks it returns the local hits (merging across ranks is up to the caller).
* ``careers(num_players, rec_of)`` folds the same join into one 64-B row per player
  (``ops/careers.py`` ``CareerTable``, csrc/career.hip, K13): games, wins, first and
  last match, peak and trough, streaks and the quality sum of every player at once,
  without the hits ever leaving the device.  On N ranks it covers the local blocks.
* ``pairs(num_players, rec_of)`` counts, for every two players who shared a rated match, how
  often they played with and against each other and how it went (``ops/pairs.py``
  ``PairTable``, csrc/pairs.hip, K15); with ``players=`` only those players' rows are kept.
* ``scorecard(roster0, rec_of)`` scores the ratings as predictions (``ops/scorecard.py``
  ``Scorecard``, csrc/score.hip, K14): the belief before every match is reconstructed from
  the rows and the roster the history started from, and the win probability it gives is
  scored against the outcome.  One rank only.
* ``expectations(roster0, rec_of)`` holds every player up against those predictions
  (``ops/expectations.py`` ``Expectations``, csrc/expect.hip, K19): expected against actual
  wins, and the strength of team mates against opponents.  One rank only.
* ``hindsight(num_players, rec_of, players)`` smooths every player's skill curve backwards
  over the filled windows (``ops/hindsight.py`` ``Hindsight``, csrc/hindsight.hip, K16) and
  returns the filtered and the smoothed curve of the listed players.  One rank only.
* ``through_time(roster0, rec_of, players)`` re-estimates the whole history jointly
  (``ops/through_time.py`` ``ThroughTime``, csrc/ttt.hip, K20) -- every match factor run again
  against everyone's smoothed belief -- and returns the listed players' curves.  One rank only.
* ``export`` / ``load`` move the filled rows through two pinned slots on a copy stream
  into one flat file plus a small JSON header; the round trip is bit-identical.  This
  is how an arena is persisted: checkpoints do not hold arena rows, so a resumed run
  gets a fresh arena that holds the windows from the resume point on
  (``first_match``), and ``history`` over it returns only what it holds.
* ``plan`` is the sizing report (row / arena / roster bytes against the device's free
  memory) a run prints before it allocates.
"""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, Iterator, Optional, Sequence, Tuple, Union

import torch

from ..ops.careers import CareerTable
from ..ops.expectations import Expectations
from ..ops.hindsight import SHARED, Hindsight
from ..ops.islands import Islands
from ..ops.native import native
from ..ops.pairs import PairTable
from ..ops.rate import RateResult, Roster
from ..ops.scorecard import Scorecard
from ..ops.through_time import ThroughTime

# an arena fits when, beside the roster, it leaves at least this fraction of the device's
# total memory free (the executor's workspaces, the next windows' records and schedules, the
# allocator's slack): a condition of the plan, not a tuned number
RESERVE_FRACTION = 0.10
ROSTER_BYTES_PER_PLAYER = 4 * (Roster.ROW + 4)  # state row + attributes
EXPORT_SLOT_BYTES = 64 << 20                    # one pinned slot of export / load
HEADER_SUFFIX = ".json"
FORMAT = 1
HIT_FLOATS = ("s_mu", "s_sig", "delta", "m_mu", "m_sig", "quality")

Index = Union[int, torch.Tensor]


def local_extent(total_matches: int, window: int, rank: int = 0, size: int = 1, first_match: int = 0) -> int:
    """Matches of global [first_match, total_matches) that fall into rank's blocks
    (``first_match`` a multiple of ``window * size``: the start of a global window)."""
    rest = max(0, int(total_matches) - int(first_match))
    per = int(window) * int(size)
    full, rem = divmod(rest, per)
    return full * int(window) + min(max(rem - int(rank) * int(window), 0), int(window))


def player_bitmap(player_ids, num_players: int, device) -> torch.Tensor:
    """int32 [ceil(P / 32)] bit patterns (bit p & 31 of word p >> 5 set for every queried
    player; ids outside [0, P) are dropped), built with torch ops on ``device``."""
    P = int(num_players)
    ids = torch.as_tensor(player_ids, dtype=torch.int64, device=device).reshape(-1)
    ids = torch.unique(ids[(ids >= 0) & (ids < P)])
    words = torch.zeros((P + 31) // 32, dtype=torch.int64, device=device)
    # distinct bits of one word add up to their OR
    words.index_add_(0, ids >> 5, torch.ones_like(ids) << (ids & 31))
    return torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32)


def records_select(rec: torch.Tensor, rows: torch.Tensor, base: int, num_players: int,
                   bitmap: torch.Tensor) -> torch.Tensor:
    """K10: ``hits`` [n, 12] int32 of the bitmap's players in ``rec`` [M, 2K+2] joined
    with the packed output rows ``rows`` [M, W] of the same matches (csrc/select.hip on a
    device, its bit-identical host mirror on the CPU):

        [match_lo, match_hi, player, slot | status << 8,
         s_mu, s_sig, delta, m_mu, m_sig, quality (bit patterns), meta0, meta1]

    in ascending (match, slot) order; ``base`` is the global index of match 0."""
    return native().records_select(rec, rows, int(base), int(num_players), bitmap)


def hits_columns(hits: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Columnar view of ``hits`` [n, 12]: ``match`` int64, ``player``, ``slot``, ``status``,
    the six floats (NaN = NULL preserved) and ``meta`` [n, 2]."""
    out = {"match": (hits[:, 0].to(torch.int64) & 0xFFFFFFFF) | (hits[:, 1].to(torch.int64) << 32),
           "player": hits[:, 2].contiguous(),
           "slot": hits[:, 3] & 0xFF,
           "status": (hits[:, 3] >> 8) & 0xFF}
    floats = hits[:, 4:10].contiguous().view(torch.float32)
    for i, name in enumerate(HIT_FLOATS):
        out[name] = floats[:, i].contiguous()
    out["meta"] = hits[:, 10:12].contiguous()
    return out


class RecordArena:
    """The packed output rows of one rank's matches, resident on ``device`` (module
    docstring).  ``matches``: rows of this rank; ``first_match``: global index of the
    first match held (the start of a global window; > 0 for the arena of a resumed run);
    ``window``: matches per rank per window (``None``: one block, one rank)."""

    def __init__(self, matches: int, K: int, device, first_match: int = 0, rank: int = 0, size: int = 1,
                 window: Optional[int] = None):
        self.matches = int(matches)
        self.K = int(K)
        self.W = RateResult.row_floats(self.K)
        self.device = torch.device(device)
        self.first_match = int(first_match)
        self.rank, self.size = int(rank), int(size)
        if window is None:
            if self.size != 1:
                raise ValueError("an arena of %d ranks needs the window length" % self.size)
            window = max(1, self.matches)
        self.window = int(window)
        if self.matches < 0 or self.window < 1 or not 0 <= self.rank < self.size or self.first_match < 0:
            raise ValueError("bad arena geometry")
        if self.first_match % (self.window * self.size):
            raise ValueError("first_match must be the start of a global window")
        self.rows = torch.empty((self.matches, self.W), dtype=torch.float32, device=self.device)
        self.filled = 0       # local rows [0, filled) are final
        self._claimed = 0     # ... [filled, _claimed) handed out for writing

    # ------------------------------------------------------------ geometry
    def global_match(self, local: Index) -> Index:
        """Global match index of local row(s) ``local``."""
        g, o = local // self.window, local % self.window
        return self.first_match + g * (self.window * self.size) + self.rank * self.window + o

    def local_row(self, match: Index) -> Index:
        """Local row(s) of global match index ``match`` (raises for a match that is not
        in this rank's blocks or before ``first_match``)."""
        rel = match - self.first_match
        per = self.window * self.size
        g, within = rel // per, rel % per
        bad = (rel < 0) | (within // self.window != self.rank)
        if bool(bad.any() if isinstance(bad, torch.Tensor) else bad):
            raise IndexError("match outside the blocks this arena holds (rank %d of %d, from match %d)"
                             % (self.rank, self.size, self.first_match))
        return g * self.window + within % self.window

    def _span(self, lo: int, hi: int) -> Tuple[int, int]:
        lo, hi = int(lo), int(hi)
        if hi < lo:
            raise IndexError("empty range [%d, %d)" % (lo, hi))
        if hi == lo:
            return self._claimed, self._claimed
        a = int(self.local_row(lo))
        b = a + (hi - lo)
        if (a % self.window) + (hi - lo) > self.window or b > self.matches:
            raise IndexError("[%d, %d) is not within one block of the arena" % (lo, hi))
        return a, b

    def windows(self) -> Iterator[Tuple[int, int]]:
        """Global [lo, hi) of every filled block, in order."""
        for a in range(0, self.filled, self.window):
            lo = int(self.global_match(a))
            yield lo, lo + min(self.window, self.filled - a)

    # ------------------------------------------------------------ rows
    def result(self, lo: int, hi: int, fill: bool = False) -> RateResult:
        """``RateResult`` views (``RateResult.from_packed``) of the rows of global matches
        [lo, hi), one block of this rank.  ``fill``: the rows are about to be written --
        they must follow the filled extent, and count as filled from ``commit()`` on;
        otherwise they must be filled already."""
        a, b = self._span(lo, hi)
        if fill:
            if a != self.filled:
                raise IndexError("windows are filled in order: expected local row %d, got %d" % (self.filled, a))
            self._claimed = b
        elif b > self.filled:
            raise IndexError("matches [%d, %d) were never filled (filled extent: %d rows)" % (lo, hi, self.filled))
        return RateResult.from_packed(self.rows[a:b], self.K)

    def commit(self) -> None:
        """The rows handed out by ``result(..., fill=True)`` are final (stream-ordered)."""
        self.filled = self._claimed

    def filled_rows(self) -> torch.Tensor:
        return self.rows[:self.filled]

    # ------------------------------------------------------------ history
    def history(self, player_ids: Sequence[int], num_players: int,
                rec_of: Callable[[int, int], torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The records of ``player_ids`` in the filled windows, chronologically:
        columnar tensors ``match`` (int64 global index), ``player``, ``slot``, ``status``,
        ``s_mu``, ``s_sig``, ``delta``, ``m_mu``, ``m_sig``, ``quality`` and ``meta``
        [n, 2].  ``rec_of(lo, hi)`` returns the records [hi - lo, 2K+2] of global matches
        [lo, hi) on the arena's device.  Only what the arena holds is searched: the
        arena of a resumed run starts at ``first_match``; on N ranks these are the
        local hits."""
        bitmap = player_bitmap(player_ids, num_players, self.device)
        parts = []
        for lo, hi in self.windows():
            rec = rec_of(lo, hi)
            a = int(self.local_row(lo))
            parts.append(records_select(rec, self.rows[a:a + hi - lo], lo, num_players, bitmap))
        hits = torch.cat(parts) if parts else torch.empty((0, 12), dtype=torch.int32, device=self.device)
        return hits_columns(hits)

    def careers(self, num_players: int, rec_of: Callable[[int, int], torch.Tensor], **kw) -> CareerTable:
        """The career table (``ops/careers.py``) of all ``num_players`` players over the
        filled windows, walked as ``history`` walks them; ``kw``: ``track``, ``score``,
        ``modes`` of ``CareerTable``.  On N ranks it covers this rank's blocks only."""
        table = CareerTable(num_players, self.device, **kw)
        for lo, hi in self.windows():
            a = int(self.local_row(lo))
            table.add(rec_of(lo, hi), self.rows[a:a + hi - lo], lo, K=self.K)
        return table

    def pairs(self, num_players: int, rec_of: Callable[[int, int], torch.Tensor], **kw) -> PairTable:
        """The pair table (``ops/pairs.py``, K15) of the filled windows, walked as ``careers``
        walks them; ``kw``: ``modes``, ``players``, ``max_entries`` of ``PairTable``.  On N
        ranks it covers this rank's blocks only."""
        table = PairTable(num_players, self.device, **kw)
        for lo, hi in self.windows():
            a = int(self.local_row(lo))
            table.add(rec_of(lo, hi), self.rows[a:a + hi - lo], K=self.K)
        return table

    def islands(self, num_players: int, rec_of: Callable[[int, int], torch.Tensor], modes=None) -> Islands:
        """The islands (``ops/islands.py``, K18) of the match graph of the filled windows, walked
        as ``careers`` walks them; ``modes`` as ``Islands`` takes them.  On N ranks it covers this
        rank's blocks only; ``Islands.merge`` unites the ranks' forests."""
        isl = Islands(num_players, self.device, modes=modes)
        for lo, hi in self.windows():
            a = int(self.local_row(lo))
            isl.add(rec_of(lo, hi), self.rows[a:a + hi - lo], K=self.K)
        return isl

    def scorecard(self, roster0, rec_of: Callable[[int, int], torch.Tensor], **kw) -> Scorecard:
        """The scorecard (``ops/scorecard.py``, K14) of the filled windows, walked as
        ``careers`` walks them.  ``roster0``: the roster the arena's history starts from, as
        it was before ``first_match`` (on a resumed run the checkpoint's roster); ``kw``:
        ``track``, ``modes``, ``cfg`` of ``Scorecard``.  A chain needs the whole history in
        order, so on N > 1 ranks this raises."""
        if self.size > 1:
            raise ValueError("a scorecard chains the whole history in order: it needs a one-rank arena, this is "
                             "rank %d of %d" % (self.rank, self.size))
        card = Scorecard(roster0, **kw)
        for lo, hi in self.windows():
            a = int(self.local_row(lo))
            card.add(rec_of(lo, hi), self.rows[a:a + hi - lo])
        return card

    def expectations(self, roster0, rec_of: Callable[[int, int], torch.Tensor], **kw) -> Expectations:
        """The expectation table (``ops/expectations.py``, K19) of the filled windows, walked
        as ``scorecard`` walks them, from the same ``roster0``; ``kw``: ``track``, ``modes``,
        ``cfg`` of ``Expectations``.  Its card chains the whole history in order, so on N > 1
        ranks this raises."""
        if self.size > 1:
            raise ValueError("expectations chain the whole history in order: they need a one-rank arena, this is "
                             "rank %d of %d" % (self.rank, self.size))
        exp = Expectations(roster0, **kw)
        for lo, hi in self.windows():
            a = int(self.local_row(lo))
            exp.add(rec_of(lo, hi), self.rows[a:a + hi - lo])
        return exp

    def hindsight(self, num_players: int, rec_of: Callable[[int, int], torch.Tensor], players: Sequence[int],
                  **kw) -> Dict[str, torch.Tensor]:
        """The filtered and the smoothed skill curve (``ops/hindsight.py``, K16) of ``players``
        over the filled windows, which are walked newest first; ``kw``: ``track``, ``cfg`` of
        ``Hindsight``.  Columnar tensors in chronological order, one entry per rated match of a
        listed player on the track: ``match`` (int64 global index), ``player``, ``slot``,
        ``mu``, ``sigma`` (filtered), ``mu_s``, ``sigma_s`` (smoothed).  A chain needs the whole
        history, so on N > 1 ranks this raises."""
        if self.size > 1:
            raise ValueError("hindsight chains the whole history: it needs a one-rank arena, this is rank %d of %d"
                             % (self.rank, self.size))
        hs = Hindsight(num_players, self.device, **kw)
        mu_name, sigma_name = ("s_mu", "s_sig") if hs.track == SHARED else ("m_mu", "m_sig")
        bitmap = player_bitmap(players, num_players, self.device)
        names = ("match", "player", "slot", "mu", "sigma", "mu_s", "sigma_s")
        parts = []
        for lo, hi in reversed(list(self.windows())):
            rec = rec_of(lo, hi)
            a = int(self.local_row(lo))
            rows = self.rows[a:a + hi - lo]
            smooth = hs.add(rec, rows, K=self.K).reshape(-1, 2)
            cols = hits_columns(records_select(rec, rows, lo, num_players, bitmap))
            at = (cols["match"] - lo) * (2 * self.K) + cols["slot"].to(torch.int64)
            pair = smooth.index_select(0, at)
            keep = ~torch.isnan(pair[:, 1])  # the hits that are elements of the track
            parts.append((cols["match"][keep], cols["player"][keep], cols["slot"][keep], cols[mu_name][keep],
                          cols[sigma_name][keep], pair[keep, 0], pair[keep, 1]))
        parts.reverse()
        if not parts:
            dt = (torch.int64, torch.int32, torch.int32) + (torch.float32,) * 4
            return {n: torch.empty(0, dtype=d, device=self.device) for n, d in zip(names, dt)}
        return {n: torch.cat([p[i] for p in parts]) for i, n in enumerate(names)}

    def through_time(self, roster0, rec_of: Callable[[int, int], torch.Tensor], players: Sequence[int],
                     sweeps: int = 8, tol: Optional[float] = None, damping: float = 1.0,
                     **kw) -> Dict[str, torch.Tensor]:
        """The filtered curve of ``players`` and their curve re-estimated jointly through time
        (``ops/through_time.py`` ``ThroughTime``, K20) over the filled windows, which are
        joined into one history: a fit takes the whole of it, so above the slot limit of one
        fit this raises ``ValueError``.  ``roster0``: the roster the arena's history starts
        from, as for ``scorecard``; ``sweeps``, ``tol``, ``damping`` of ``ThroughTime.fit``;
        ``kw``: ``track``, ``cfg``.  Columnar tensors in chronological order as ``hindsight``
        returns them, with ``mu_tt``, ``sigma_tt`` for the smoothed pair; ``residual`` and
        ``sweeps`` of the fit ride along as a fp64 tensor.  One rank only."""
        if self.size > 1:
            raise ValueError("through time chains the whole history: it needs a one-rank arena, this is rank %d of "
                             "%d" % (self.rank, self.size))
        num_players = int((roster0.state if hasattr(roster0, "state") else roster0).shape[0])
        tt = ThroughTime(roster0, **kw)
        mu_name, sigma_name = ("s_mu", "s_sig") if tt.track == SHARED else ("m_mu", "m_sig")
        names = ("match", "player", "slot", "mu", "sigma", "mu_tt", "sigma_tt")
        spans = list(self.windows())
        slots = sum(hi - lo for lo, hi in spans) * 2 * self.K
        if slots > tt.max_slots:
            raise ValueError("the arena holds %d slots, above the limit of %d slots (MAX_SLOTS) of one fit"
                             % (slots, tt.max_slots))
        if not spans:
            dt = (torch.int64, torch.int32, torch.int32) + (torch.float32,) * 4
            out = {n: torch.empty(0, dtype=d, device=self.device) for n, d in zip(names, dt)}
            out["residual"] = torch.empty(0, dtype=torch.float64)
            return out
        first = spans[0][0]
        rec = torch.cat([rec_of(lo, hi) for lo, hi in spans])
        rows = torch.cat([self.rows[int(self.local_row(lo)):int(self.local_row(lo)) + hi - lo] for lo, hi in spans]) \
            if len(spans) > 1 else self.rows[int(self.local_row(first)):int(self.local_row(first)) + spans[0][1] - first]
        fit = tt.fit(rec, rows, sweeps=sweeps, tol=tol, damping=damping)
        cols = hits_columns(records_select(rec, rows, first, num_players,
                                           player_bitmap(players, num_players, self.device)))
        at = (cols["match"] - first) * (2 * self.K) + cols["slot"].to(torch.int64)
        pair = fit.smoothed.reshape(-1, 2).index_select(0, at)
        keep = ~torch.isnan(pair[:, 1])  # the hits that are elements of the track
        out = dict(zip(names, (cols["match"][keep], cols["player"][keep], cols["slot"][keep], cols[mu_name][keep],
                               cols[sigma_name][keep], pair[keep, 0], pair[keep, 1])))
        out["residual"] = torch.tensor(fit.residual, dtype=torch.float64)
        return out

    # ------------------------------------------------------------ sizing
    @staticmethod
    def plan(total_matches: int, K: int, device=None, size: int = 1, roster_players: int = 0,
             free_bytes: Optional[int] = None, total_bytes: Optional[int] = None,
             window: Optional[int] = None) -> Dict[str, object]:
        """Sizing report of an arena for ``total_matches`` over ``size`` ranks: row bytes,
        arena bytes per rank (the largest rank's; with ``window`` exactly, else an even
        split), roster bytes, free and total device memory (``torch.cuda.mem_get_info``
        of ``device`` -- host memory for a CPU arena --, or ``free_bytes`` /
        ``total_bytes`` as given; ``total_bytes`` defaults to ``free_bytes``), and
        ``fits``: false when arena and roster would leave less than
        ``RESERVE_FRACTION`` of the total free."""
        row_bytes = 4 * RateResult.row_floats(int(K))
        size = max(1, int(size))
        per_rank = (local_extent(total_matches, window, 0, size) if window
                    else -(-int(total_matches) // size))
        if free_bytes is None:
            dev = torch.device(device) if device is not None else torch.device("cuda")
            if dev.type == "cuda":
                free, total = torch.cuda.mem_get_info(dev)
            else:  # a host arena lives in host memory
                page = os.sysconf("SC_PAGE_SIZE")
                free, total = os.sysconf("SC_AVPHYS_PAGES") * page, os.sysconf("SC_PHYS_PAGES") * page
            total_bytes = total if total_bytes is None else total_bytes
        else:
            free = int(free_bytes)
            total_bytes = free if total_bytes is None else total_bytes
        arena_bytes = per_rank * row_bytes
        roster_bytes = int(roster_players) * ROSTER_BYTES_PER_PLAYER
        reserve = -int(-RESERVE_FRACTION * int(total_bytes) // 1)  # rounded up: left >= reserve is exact
        left = int(free) - arena_bytes - roster_bytes
        return {"matches": int(total_matches), "ranks": size, "team_size": int(K), "row_bytes": row_bytes,
                "matches_per_rank": per_rank, "arena_bytes_per_rank": arena_bytes, "roster_bytes": roster_bytes,
                "free_bytes": int(free), "total_bytes": int(total_bytes), "reserve_bytes": reserve,
                "left_bytes": left, "fits": left >= reserve}

    # ------------------------------------------------------------ persistence
    def _header(self) -> Dict[str, int]:
        return {"format": FORMAT, "K": self.K, "W": self.W, "extent": self.filled, "first_match": self.first_match,
                "rank": self.rank, "size": self.size, "window": self.window}

    def _chunks(self, n: int):
        step = max(1, EXPORT_SLOT_BYTES // (4 * self.W))
        return step, [(a, min(a + step, n)) for a in range(0, n, step)]

    def export(self, path: str) -> int:
        """Write the filled rows to the flat file ``path`` and the header (K, W, extent,
        rank, size, window, first_match) to ``path + ".json"``; returns the bytes of rows.
        On a device the rows go through two pinned slots on a copy stream, the copy of
        one chunk beside the write of the previous."""
        rows = self.filled_rows()
        step, chunks = self._chunks(self.filled)
        with open(path, "wb") as f:
            if self.device.type != "cuda":
                for a, b in chunks:
                    f.write(memoryview(rows[a:b].numpy()).cast("B"))
            elif chunks:
                copy = torch.cuda.Stream(self.device)
                copy.wait_stream(torch.cuda.current_stream(self.device))
                slots = [torch.empty((step, self.W), dtype=torch.float32, pin_memory=True) for _ in range(2)]
                done = [torch.cuda.Event(), torch.cuda.Event()]

                def issue(i):
                    a, b = chunks[i]
                    with torch.cuda.stream(copy):
                        slots[i & 1][:b - a].copy_(rows[a:b], non_blocking=True)
                        done[i & 1].record(copy)

                issue(0)
                for i, (a, b) in enumerate(chunks):
                    if i + 1 < len(chunks):
                        issue(i + 1)  # its slot's previous chunk is on disk: the writes are synchronous
                    done[i & 1].synchronize()
                    f.write(memoryview(slots[i & 1][:b - a].numpy()).cast("B"))
            f.flush()
            os.fsync(f.fileno())
        with open(path + HEADER_SUFFIX, "w") as f:
            json.dump(dict(self._header(), bytes=self.filled * self.W * 4), f, indent=1, sort_keys=True)
        return self.filled * self.W * 4

    @staticmethod
    def load(path: str, device="cpu") -> "RecordArena":
        """The arena ``export`` wrote, filled, on ``device`` (bit-identical rows).  A
        file whose size does not match its header is refused."""
        with open(path + HEADER_SUFFIX) as f:
            h = json.load(f)
        if h.get("format") != FORMAT or h["W"] != RateResult.row_floats(h["K"]):
            raise ValueError("%s: not a record arena header" % (path + HEADER_SUFFIX))
        n = int(h["extent"])
        if os.path.getsize(path) != n * h["W"] * 4 or h.get("bytes") != n * h["W"] * 4:
            raise ValueError("%s holds %d bytes but its header says %d rows of %d bytes"
                             % (path, os.path.getsize(path), n, h["W"] * 4))
        arena = RecordArena(n, h["K"], device, first_match=h["first_match"], rank=h["rank"], size=h["size"],
                            window=h["window"])
        step, chunks = arena._chunks(n)

        def fill(f, t):
            mv = memoryview(t.numpy()).cast("B")
            while len(mv):
                got = f.readinto(mv)
                if not got:
                    raise ValueError("%s is truncated" % path)
                mv = mv[got:]

        with open(path, "rb", buffering=0) as f:
            if arena.device.type != "cuda":
                for a, b in chunks:
                    fill(f, arena.rows[a:b])
            elif chunks:
                copy = torch.cuda.Stream(arena.device)
                copy.wait_stream(torch.cuda.current_stream(arena.device))
                slots = [torch.empty((step, arena.W), dtype=torch.float32, pin_memory=True) for _ in range(2)]
                done = [None, None]
                for i, (a, b) in enumerate(chunks):
                    if done[i & 1] is not None:
                        done[i & 1].synchronize()  # the slot's previous chunk reached the device
                    fill(f, slots[i & 1][:b - a])
                    with torch.cuda.stream(copy):
                        arena.rows[a:b].copy_(slots[i & 1][:b - a], non_blocking=True)
                        done[i & 1] = torch.cuda.Event()
                        done[i & 1].record(copy)
                torch.cuda.current_stream(arena.device).wait_stream(copy)
                copy.synchronize()  # the pinned slots are released on return
        arena.filled = arena._claimed = n
        return arena
