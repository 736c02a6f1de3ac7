"""Full-history re-rate driver (SURVEY P4 + C5 + C4; BASELINE configs 3 and 5).

The reference is online-only: batches of <= 500 matches in arrival order, no
way to re-rate a history (/root/reference/worker.py:18,176).  This driver
streams a long synthetic history through the engine window by window:

* the history is a counter-RNG stream, so window ``g`` of rank ``r`` is
  generated on the device from its global offset -- no host I/O, and any window
  can be regenerated after a crash;
* one rank: windows are rated exactly, in order (dataflow engine, prepass of
  window g+1 overlapped with rating g -- runtime/engine.py);
* N ranks (one per GPU): time-axis sharding -- global window g is N
  consecutive blocks of ``window`` matches, rank r rates block r exactly from
  the window-start roster, then one RCCL all-reduce of natural-parameter
  messages merges the blocks (sweep mode, parallel/sweep.py);
* every ``checkpoint_every`` windows the replicated roster and the stream
  position are checkpointed atomically; a restarted run resumes from there and
  produces the same roster as an uninterrupted run (exactly-once);
* every window's per-participant output records (the reference writes them per
  match, /root/reference/rater.py:151-169, committed per batch at
  worker.py:194) are accounted for: ``records="digest"`` reduces them on the
  device to a count + fp64 column sums per window (a resumed run reproduces the
  digests of the windows it re-rates); ``records="host"`` streams them D2H into
  a ring of pinned buffers on a copy stream, overlapped with the next windows
  (double-buffered device outputs), and hands them to ``on_records``;
  ``records="resident"`` keeps them on the device: every window is rated straight
  into its slice of a ``RecordArena`` (runtime/records.py; 128 B per 3v3 match, so
  1B matches are 128 GB on one GPU, 16 GB per GPU on 8), still digested per window,
  and ``arena.history`` selects the records of a set of players out of it in
  chronological order (csrc/select.hip).  Checkpoints do not hold arena rows: a
  resumed run fills a fresh arena from the resume point on (``arena.first_match``),
  and ``arena.export`` / ``RecordArena.load`` persist one;
* status counters are accumulated on the device and reduced over ranks (C4);
  the executor's error flags are sticky over windows and checked before every
  checkpoint, so a failed middle window is never checkpointed over.

    python -m analyzer_amd.runtime.rerate --matches 1000000000 --players 10000000 \\
        --window 16000000 --team-size 3 --checkpoint-dir /tmp/ck
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --records resident --history 17,4242 --export-records /data/records.bin
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --ladder shared,ranked --ladder-top 10 --ladder-rank 17,4242
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --matchmake ranked:3:100000
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --records resident --score mode     # the scorecard of the run (ops/scorecard.py)
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --records resident --pairs 17,4242  # whom they play with and against (ops/pairs.py)
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --records resident --hindsight 17,4242 --hindsight-track ranked  # smoothed curves (ops/hindsight.py)
    python -m analyzer_amd.runtime.rerate --matches 20000000 --players 1000000 \\
        --window 16000000 --records resident --through-time 17,4242 --through-time-sweeps 12  # the joint re-estimate (ops/through_time.py)
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --records resident --islands --islands-ranks 8 # which ratings are comparable (ops/islands.py)
    python -m analyzer_amd.runtime.rerate --matches 500000000 --players 10000000 \\
        --window 16000000 --records resident --expect 17,4242 --expect-outliers 20  # wins against the odds (ops/expectations.py)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from collections import deque
from dataclasses import asdict, dataclass
from typing import Callable, Dict, Optional

import torch

from ..config import EngineConfig, RaterConfig
from ..ops import rate as R
from ..ops.expectations import expectation_lines, outliers_line
from ..ops.hindsight import track_of
from ..ops.islands import islands_line
from ..ops.ladder import build_ladder, track_index
from ..ops.matchmake import make_lobbies, mode_index, preview_matches, queue_order
from ..ops.synth import RosterSpec, StreamSpec, make_roster, make_stream
from ..parallel.comm import broadcast_roster, init_from_env, reduce_counts, world
from ..parallel.sweep import SweepMerger
from ..utils.trace import trace_range
from .checkpoint import CheckpointManager
from .engine import WindowPipeline
from .ingest import OutputSink
from .records import RecordArena, local_extent


class InjectedFault(SystemExit):
    """Raised by ``fault_kill_after`` to simulate a crash (exit code 17)."""


@dataclass
class RerateSpec:
    total_matches: int
    players: int
    team_size: int = 3
    window: int = 1_000_000          # matches per rank per window
    seed: int = 2024
    p_afk: float = 0.02
    p_rated: float = 0.0             # fraction of players with a stored rating at start

    def roster_spec(self) -> RosterSpec:
        return RosterSpec(num_players=self.players, seed=self.seed, p_rated=self.p_rated)

    def stream_spec(self) -> StreamSpec:
        return StreamSpec(team_size=self.team_size, seed=self.seed + 1, p_afk=self.p_afk)


def default_comm_dtype(sweeps: int) -> str:
    """Merge message precision when none is given: fp16 for one sweep -- BASELINE config 5
    names fp16 moments, and bench.py --config 5 merges in fp16 (8 ranks x 16M matches over
    10M players: roster Spearman 0.9988, 0 clamps, profiles/r6/fidelity_config5.log) --
    and fp32 for causal re-sweeps, whose prefixes must telescope exactly."""
    return "fp16" if int(sweeps) <= 1 else "fp32"


def n_windows(spec: RerateSpec, size: int) -> int:
    per = spec.window * size
    return (spec.total_matches + per - 1) // per


def window_slice(spec: RerateSpec, g: int, rank: int, size: int):
    """[lo, hi) global match offsets of rank's block of window g."""
    lo = g * spec.window * size + rank * spec.window
    hi = min(lo + spec.window, spec.total_matches)
    return lo, max(lo, hi)


class _Digest:
    """Per-window digests on the device: one deterministic streaming pass over the
    packed output rows (csrc/digest.hip) -- 7 torch nansum passes and a bincount
    before, 8.5 ms per 16M-match window (profiles/r6/rerate_attribution.log).  With
    ``hist`` (int64[256] on the rows' device) the pass also adds the window's status
    counts to it, in place of a strided copy + bincount of the status bytes (the host
    path counts with a bincount)."""

    def __init__(self):
        self._scratch = {}

    def device(self, res: R.RateResult) -> bool:
        return res.packed is not None and res.packed.is_cuda

    def __call__(self, res: R.RateResult, K: int, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
        rows = res.packed
        if not self.device(res):
            if hist is not None:
                hist += torch.bincount(res.status.to(torch.int64), minlength=256)
            return window_digest(res)
        from ..ops.native import native

        key = (rows.device, K)
        if key not in self._scratch:
            self._scratch[key] = torch.empty(native().records_digest_scratch(K), dtype=torch.float64,
                                             device=rows.device)
        out = torch.empty(3 + 10 * K, dtype=torch.float64, device=rows.device)
        native().records_digest(rows, K, self._scratch[key], out, hist)
        return out


def window_digest(res: R.RateResult) -> torch.Tensor:
    """[2 + 5*2K + 1] fp64: matches with records (rated / AFK / invalid),
    participant records written (non-NULL shared mu), then the column sums of the
    five per-slot outputs and quality over written values (the host / unpacked
    path; on the device ``_Digest`` computes the same in one kernel)."""
    S = res.s_mu.shape[1]
    st = res.status
    wrote = (st == R.RATED) | (st == R.AFK) | (st == R.INVALID_ROSTERS)
    parts = [wrote.sum().to(torch.float64).view(1),
             (~torch.isnan(res.s_mu)).sum().to(torch.float64).view(1)]
    for t in (res.s_mu, res.s_sig, res.delta, res.m_mu, res.m_sig):
        parts.append(torch.nansum(t, dim=0, dtype=torch.float64).view(S))
    parts.append(torch.nansum(res.quality, dtype=torch.float64).view(1))
    return torch.cat(parts)


def run(spec: RerateSpec, device=None, checkpoint_dir: Optional[str] = None,
        checkpoint_every: int = 1, fault_kill_after: Optional[int] = None,
        on_window: Optional[Callable[[int, R.RateResult], None]] = None,
        rater: Optional[R.BatchRater] = None, comm_dtype: Optional[str] = None,
        records: str = "digest", on_records: Optional[Callable[[int, dict], None]] = None,
        sweeps: int = 1, arena: Optional[RecordArena] = None):
    """Rate the whole history; returns (metrics reduced over ranks, final roster).

    ``records``: "digest" (device reduction per window, in the metrics as
    ``window_digests``), "host" (pinned D2H ring; ``on_records(base, host_dict)``
    gets every window's rows), "none", or "resident": every window is rated straight
    into its slice of ``arena`` (runtime/records.py; required in this mode --
    ``rerate_resident`` plans and allocates one) and the digests are computed from
    the arena slices, so ``window_digests`` stay comparable across modes.

    Arena rows are not written into checkpoints (the meta only names the mode and the
    arena's filled extent): a resumed resident run needs a fresh arena whose
    ``first_match`` is the resume offset; it holds the windows from the resume point
    on, and ``arena.history`` over it returns only those.  ``arena.export`` persists
    an arena."""
    if records not in ("digest", "host", "none", "resident"):
        raise ValueError("records must be digest, host, none or resident")
    resident = records == "resident"
    if resident and arena is None:
        raise ValueError("records='resident' needs an arena (rerate_resident plans and allocates one)")
    if arena is not None and not resident:
        raise ValueError("an arena is only filled with records='resident'")
    rank, size = world()
    dev = torch.device(device) if device is not None else (
        torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    rater = rater or R.BatchRater(RaterConfig())
    K = spec.team_size
    # the rating kernels only read the attributes (csrc/dataflow.hip): written with the
    # first checkpoint, hard-linked into the later ones (runtime/checkpoint.py)
    ck = CheckpointManager(checkpoint_dir, checkpoint_every, rank=0, static_attrs=True)
    start_window = 0
    restored = ck.latest(dev)
    if restored is not None:
        roster, meta = restored
        if meta.get("spec") != asdict(spec) or meta.get("world") != size:
            raise ValueError("checkpoint in %s belongs to a different run" % checkpoint_dir)
        start_window = int(meta["windows_done"])
    else:
        roster = make_roster(spec.roster_spec(), device=dev)
        broadcast_roster(roster)  # C3 (identical by construction; keeps replicas honest)
    if resident:
        first = window_slice(spec, start_window, 0, size)[0]
        if (arena.K, arena.rank, arena.size, arena.window, arena.first_match) != (K, rank, size, spec.window, first) \
                or arena.matches < local_extent(spec.total_matches, spec.window, rank, size, first) \
                or arena.filled or arena.device.type != dev.type:
            raise ValueError("the arena does not match this run: it must be empty, on %s, of team size %d, rank %d "
                             "of %d, window %d, and hold the matches from %d on"
                             % (dev.type, K, rank, size, spec.window, first))
    comm_dtype = comm_dtype or default_comm_dtype(sweeps)
    merger = (SweepMerger(spec.players, dev, rater.cfg, comm_dtype=comm_dtype, sweeps=sweeps)
              if size > 1 else None)
    pipe = WindowPipeline(rater, roster, K, merger=merger)
    total = n_windows(spec, size)
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    digests = {}
    digest = _Digest()
    sspec = spec.stream_spec()
    outs = [None, None]  # double-buffered: the sink copies one while the next is rated
    host_stats = {"windows": 0, "participant_records": 0}

    def took(base, host):
        host_stats["windows"] += 1
        host_stats["participant_records"] += int((~torch.isnan(host["s_mu"])).sum())
        if on_records is not None:
            on_records(base, host)

    sink = OutputSink(dev, took) if records == "host" else None
    if dev.type == "cuda":
        rater.clear_sticky(dev)

    def window_rec(g):
        lo, hi = window_slice(spec, g, rank, size)
        return make_stream(sspec, hi - lo, spec.players, K=K, base=lo, device=dev)

    # ANA_RERATE_GEN=tail (default): the next window's records are generated in the rating's
    # tail on the prepass stream (needs the tail-overlapped prepass, no DP merge); main: on
    # the main stream between the ratings
    gen_tail = (os.environ.get("ANA_RERATE_GEN", "tail") == "tail" and dev.type == "cuda" and merger is None
                and pipe.side is not None and pipe.side != torch.cuda.current_stream(dev) and pipe.tail > 0)
    # the checkpoint writer's pinned buffers are set up before the run, like the roster
    # (ANA_CKPT_PREPARE=0: at the first save)
    if rank == 0 and os.environ.get("ANA_CKPT_PREPARE", "1") not in ("", "0", "false"):
        ck.prepare(roster)
    t0 = time.perf_counter()
    rated = 0
    D = pipe.depth  # windows prepared ahead (runtime/engine.py)
    ahead = deque(pipe.prepare(window_rec(j)) for j in range(start_window, min(start_window + D, total)))
    for g in range(start_window, total):
        cur = ahead.popleft()
        M = cur.rec.shape[0]
        b = g & 1
        if resident:  # rated in place: the window's slice of the arena, no double buffer
            out = arena.result(*window_slice(spec, g, rank, size), fill=True)
        else:
            if outs[b] is None or outs[b].quality.shape[0] != M:
                outs[b] = R.RateResult.allocate(M, K, dev)
            elif sink is not None and sink.copied(outs[b]) is not None:
                torch.cuda.current_stream(dev).wait_event(sink.copied(outs[b]))
            out = outs[b]
        nw = g + D  # the window prepared behind this rating
        if gen_tail and nw < total:
            # window g+D is generated on the prepass stream in rate(g)'s tail, right before
            # its prepass, instead of on the main stream in front of rate(g)
            res = pipe.rate(cur, out=out)
            side = pipe.side
            with torch.cuda.stream(side):
                pipe.wait_tail(side)
                rec_next = window_rec(nw)
                made = torch.cuda.Event()
                made.record(side)
            rec_next.record_stream(torch.cuda.current_stream(dev))
            ahead.append(pipe.prepare(rec_next, produced=made))
        else:
            # window g+D is generated before rate(g) is enqueued; its prepass waits for the tail
            res, nxt = pipe.step(cur, window_rec(nw) if nw < total else None, out=out)
            if nxt is not None:
                ahead.append(nxt)
        pipe.results_ready(res)  # the DP merge's deferred record correction of these rows
        if resident:
            arena.commit()  # the slice is final (stream-ordered)
        if records == "digest" or resident:
            digests[g] = digest(res, K, counts)  # + the status counts
        else:
            counts += torch.bincount(res.status.to(torch.int64), minlength=256)
        if sink is not None:
            sink.push(window_slice(spec, g, rank, size)[0], res)
        rated += M
        if on_window is not None:
            on_window(g, res)
        if ck.due(g + 1):
            if dev.type == "cuda":  # never checkpoint over a failed window
                rater.check_errors(dev, sticky=True)
            if merger is not None:  # ... nor over a clamped merge decode
                merger.check()
            if rank == 0:
                with trace_range("checkpoint", window=g + 1):
                    ck.maybe_save(g + 1, roster, {"spec": asdict(spec), "world": size,
                                                  "next_offset": window_slice(spec, g + 1, 0, size)[0],
                                                  # the arena's rows are not saved, only how far it was filled
                                                  "records": records,
                                                  "arena_extent": arena.filled if resident else None})
        if fault_kill_after is not None and g + 1 >= fault_kill_after:
            # the simulated crash hits once the checkpoints submitted so far are
            # committed (asynchronous writes, runtime/checkpoint.py): a real crash
            # loses the ones still in flight and resumes from the one before
            ck.flush()
            if dev.type == "cuda":
                torch.cuda.synchronize()
            raise InjectedFault(17)
    if sink is not None:
        sink.flush()
    ck.flush()  # the run ends when its last checkpoint is committed
    if dev.type == "cuda":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dev.type == "cuda":
        rater.check_errors(dev, sticky=True)
    if merger is not None:
        merger.check()
    c = counts.cpu()
    local = {R.STATUS_NAMES.get(i, str(i)): float(c[i]) for i in range(256) if int(c[i])}
    local["matches"] = float(rated)
    if (records == "digest" or resident) and digests:
        d = torch.stack([digests[g] for g in sorted(digests)]).cpu()
        local["match_records"] = float(d[:, 0].sum())
        local["participant_records"] = float(d[:, 1].sum())
    elif records == "host":
        local["participant_records"] = float(host_stats["participant_records"])
        local["egress_bytes"] = float(sink.bytes)
    summed = reduce_counts(local, dev)
    summed["seconds"] = reduce_counts({"seconds": dt}, dev, op="max")["seconds"]
    summed["windows"] = float(total - start_window)
    summed["resumed_from_window"] = float(start_window)
    summed["matches_per_s"] = summed["matches"] / summed["seconds"] if summed["seconds"] > 0 else 0.0
    if rank == 0:
        summed.update({"checkpoint_" + k: v for k, v in ck.stats().items()})
    if records == "digest" or resident:
        summed["window_digests"] = {g: digests[g].cpu().tolist() for g in sorted(digests)}
    return summed, roster


class ArenaDoesNotFit(MemoryError):
    """``rerate_resident``: the planned arena would not leave the reserve free
    (``plan``: the ``RecordArena.plan`` report)."""

    def __init__(self, plan: dict):
        super().__init__("a resident record arena of %d bytes per rank (+ %d roster bytes) does not fit %d free "
                         "bytes with %d in reserve" % (plan["arena_bytes_per_rank"], plan["roster_bytes"],
                                                       plan["free_bytes"], plan["reserve_bytes"]))
        self.plan = plan


def resume_offset(spec: RerateSpec, checkpoint_dir: Optional[str], size: int) -> int:
    """Global match offset a run over ``checkpoint_dir`` starts from (0 without a checkpoint)."""
    ck = CheckpointManager(checkpoint_dir)
    if not ck.path:
        return 0
    for cand in (ck.path, ck.path + ".old"):  # CheckpointManager.latest's order
        meta, tensors = os.path.join(cand, "meta.json"), os.path.join(cand, "roster.safetensors")
        if os.path.exists(meta) and os.path.exists(tensors):
            with open(meta) as f:
                return window_slice(spec, int(json.load(f)["windows_done"]), 0, size)[0]
    return 0


def stream_records(spec: RerateSpec, device) -> Callable[[int, int], torch.Tensor]:
    """``rec_of`` for ``RecordArena.history``: the records of global matches [lo, hi),
    regenerated from the run's counter-RNG stream."""
    sspec = spec.stream_spec()
    return lambda lo, hi: make_stream(sspec, hi - lo, spec.players, K=spec.team_size, base=lo, device=device)


def rerate_resident(spec: RerateSpec, device=None, checkpoint_dir: Optional[str] = None,
                    free_bytes: Optional[int] = None, plan: Optional[dict] = None, **kwargs):
    """``run(..., records="resident")`` with an arena of its own: plans it
    (``RecordArena.plan``; ``ArenaDoesNotFit`` when it would not leave the reserve),
    allocates it for this rank from the checkpoint's resume point on and runs.
    Returns (metrics, roster, arena); the metrics carry the plan as ``arena_plan``."""
    rank, size = world()
    dev = torch.device(device) if device is not None else (
        torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    if plan is None:
        plan = RecordArena.plan(spec.total_matches, spec.team_size, dev, size=size, roster_players=spec.players,
                                free_bytes=free_bytes, window=spec.window)
    if not plan["fits"]:
        raise ArenaDoesNotFit(plan)
    first = resume_offset(spec, checkpoint_dir, size)
    arena = RecordArena(local_extent(spec.total_matches, spec.window, rank, size, first), spec.team_size, dev,
                        first_match=first, rank=rank, size=size, window=spec.window)
    metrics, roster = run(spec, dev, checkpoint_dir=checkpoint_dir, records="resident", arena=arena, **kwargs)
    metrics["arena_plan"] = plan
    return metrics, roster, arena


def start_roster(spec: RerateSpec, checkpoint_dir: Optional[str], device) -> R.Roster:
    """The roster a run over ``checkpoint_dir`` starts from, taken before the run: the
    checkpoint's roster on a resumed run (the arena then starts at its ``first_match``),
    else the generated one.  This is what ``RecordArena.scorecard`` chains from."""
    restored = CheckpointManager(checkpoint_dir).latest(device)
    return restored[0] if restored is not None else make_roster(spec.roster_spec(), device=device)


def _timeline(hist: dict, player: int) -> dict:
    """One player's rows of a ``RecordArena.history`` result as JSON-ready lists (NaN -> null)."""
    sel = (hist["player"] == player).nonzero().reshape(-1)
    line = {"player": int(player), "records": int(sel.numel())}
    for name, col in hist.items():
        if name == "player":
            continue
        vals = col.index_select(0, sel).cpu().tolist()
        if col.dtype.is_floating_point:
            vals = [None if v != v else v for v in vals]
        line[name] = vals
    return line


def career_lines(table, ids) -> list:
    """One JSON-ready dict per player of ``ids`` from a ``CareerTable`` (ops/careers.py)."""
    cols = {name: col.cpu().tolist() for name, col in table.lookup(list(ids)).items()}
    return [dict({"career": int(p), "track": table.track, "score": table.score},
                 **{name: _num(vals[i]) for name, vals in cols.items()}) for i, p in enumerate(ids)]


def hindsight_lines(curves: dict, ids, track: str) -> list:
    """One JSON-ready dict per player of ``ids`` from a ``RecordArena.hindsight`` result: the
    matches of the player's chain with the filtered and the smoothed (mu, sigma) at each."""
    lines = []
    for p in ids:
        sel = (curves["player"] == p).nonzero().reshape(-1)
        line = {"hindsight": int(p), "track": track, "records": int(sel.numel())}
        for name in ("match", "mu", "sigma", "mu_s", "sigma_s"):
            line[name] = [_num(v) for v in curves[name].index_select(0, sel).cpu().tolist()]
        lines.append(line)
    return lines


def through_time_lines(curves: dict, ids, track: str) -> list:
    """One JSON-ready dict per player of ``ids`` from a ``RecordArena.through_time`` result: the
    matches of the player's chain with the filtered and the jointly re-estimated (mu, sigma) at
    each, and the fit's sweeps and last residual."""
    resid = curves["residual"].tolist()
    lines = []
    for p in ids:
        sel = (curves["player"] == p).nonzero().reshape(-1)
        line = {"through_time": int(p), "track": track, "records": int(sel.numel()), "sweeps": len(resid),
                "residual": _num(resid[-1]) if resid else None}
        for name in ("match", "mu", "sigma", "mu_tt", "sigma_tt"):
            line[name] = [_num(v) for v in curves[name].index_select(0, sel).cpu().tolist()]
        lines.append(line)
    return lines


def pair_lines(table, ids, top: int = 5) -> list:
    """One JSON-ready dict per player of ``ids`` from a ``PairTable`` (ops/pairs.py): the number
    of distinct players it shared a rated match with, and its ``top`` most frequent team mates
    and opponents with its own wins next to them."""
    lines = []
    for p in ids:
        line = {"pairs": int(p), "partners": table.n_partners(p)}
        for name, relation in (("with", "with"), ("against", "against")):
            cols = {k: v.cpu().tolist() for k, v in table.partners(p, relation, top=top).items()}
            line[name] = [{"player": q, "games": g, "wins": w}
                          for q, g, w in zip(cols["player"], cols["games"], cols["wins"])]
        lines.append(line)
    return lines


def _num(v: float):
    return None if v != v else v  # NaN -> null


def ladder_lines(roster: R.Roster, tracks, top: int = 10, ids=(), score: str = "conservative") -> list:
    """One JSON-ready dict per track of ``tracks`` from ``roster`` (ops/ladder.py, one build for
    all tracks): the ladder's size, its best ``top`` players and the standing of ``ids``."""
    lad = build_ladder(roster, tracks, score=score)
    lines = []
    for name in tracks:
        t_ids, t_mu, t_sig, t_score = (x.cpu().tolist() for x in lad.top(name, top))
        line = {"ladder": name, "score": score, "players": lad.num_players, "ranked": lad.ranked(name),
                "top": [{"rank": i, "player": p, "mu": _num(m), "sigma": _num(sg), "score": _num(sc)}
                        for i, (p, m, sg, sc) in enumerate(zip(t_ids, t_mu, t_sig, t_score))],
                "ranks": []}
        if len(ids):
            rank, sc, pct = (x.cpu().tolist() for x in lad.lookup(name, list(ids)))
            line["ranks"] = [{"player": int(p), "rank": r, "score": _num(s_), "percentile": _num(q)}
                             for p, r, s_, q in zip(ids, rank, sc, pct)]
        lines.append(line)
    return lines


def matchmake_line(roster: R.Roster, mode: str, K: int, Q: int, seed: int = 2024) -> dict:
    """One JSON-ready dict: ``make_lobbies`` (ops/matchmake.py) on ``roster`` for a queue of the
    first Q players of a seeded ``torch.randperm(P)``: the lobbies formed, the unmatched players,
    and what balancing bought -- mean and minimum quality, mean |p_win0 - 0.5| -- against the
    lobbies as given (2K consecutive players of the descending-mu order, first K against last K)."""
    S = 2 * K
    gen = torch.Generator().manual_seed(int(seed))
    queue = torch.randperm(roster.num_players, generator=gen)[:Q].to(torch.int32).to(roster.device)
    bal, unmatched = make_lobbies(roster, queue, mode=mode, K=K)
    ok = bal.status == 0
    n = int(bal.status.numel())
    line = {"matchmake": mode, "team_size": K, "queue": int(queue.numel()), "lobbies": n,
            "balanced": int(ok.sum()), "unmatched": int(unmatched.numel())}
    if int(ok.sum()):
        # the lobbies as given, as stream records: their p_win0 comes from a preview
        pos, _ = queue_order(roster, queue, mode)
        given = bal.records.clone()
        given[:, :S] = queue.index_select(0, pos[:n * S].to(torch.int64)).reshape(n, S)
        p_given = preview_matches(roster, given).p_win0[ok].double()
        q, qg = bal.quality[ok].double(), bal.quality_given[ok].double()
        line.update(quality_given_mean=float(qg.mean()), quality_given_min=float(qg.min()),
                    quality_mean=float(q.mean()), quality_min=float(q.min()),
                    p_off_given_mean=float((p_given - 0.5).abs().mean()),
                    p_off_mean=float((bal.p_win0[ok].double() - 0.5).abs().mean()))
    return line


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matches", type=float, required=True)
    ap.add_argument("--players", type=float, required=True)
    ap.add_argument("--team-size", type=int, default=3)
    ap.add_argument("--window", type=float, default=1e6)
    ap.add_argument("--seed", type=int, default=2024)
    ecfg = EngineConfig.from_env()
    ap.add_argument("--checkpoint-dir", default=ecfg.checkpoint_dir)
    ap.add_argument("--checkpoint-every", type=int, default=ecfg.checkpoint_every)
    ap.add_argument("--fault-kill-after", type=int, default=None,
                    help="fault injection: exit(17) after this many windows")
    ap.add_argument("--device", default=None)
    ap.add_argument("--comm-dtype", default=ecfg.comm_dtype or None,
                    choices=["fp32", "fp16", "bf16"], help="sweep-merge message precision")
    ap.add_argument("--records", default="digest", choices=["digest", "host", "none", "resident"],
                    help="output records: device digest per window, pinned D2H stream, dropped, or kept in a "
                         "device-resident arena (prints the arena's sizing plan first; exit code 2 if it does not fit)")
    ap.add_argument("--history", default=None, metavar="ID[,ID...]",
                    help="with --records resident: print each player's timeline after the run (JSON lines)")
    ap.add_argument("--careers", default=None, metavar="ID[,ID...]",
                    help="with --records resident: print each player's career after the run (JSON lines): games, "
                         "wins, first / last match, peak and trough score, streaks, mean quality")
    ap.add_argument("--careers-track", default="shared", choices=["shared", "mode"],
                    help="with --careers: score the shared track or each match's mode track")
    ap.add_argument("--careers-modes", default=None, metavar="MODE[,MODE...]",
                    help="with --careers: count only the matches of these modes (default: all)")
    ap.add_argument("--hindsight", default=None, metavar="ID[,ID...]",
                    help="with --records resident: print each player's filtered and smoothed skill curve after the "
                         "run (JSON lines; one rank only): the curve smoothed backwards over the player's own rated "
                         "matches, not a re-run of the match factors")
    ap.add_argument("--hindsight-track", default=None, metavar="TRACK",
                    help="with --hindsight: the shared track (default) or a mode's")
    ap.add_argument("--through-time", default=None, metavar="ID[,ID...]",
                    help="with --records resident: print each player's filtered skill curve and the curve "
                         "re-estimated jointly through time after the run (JSON lines; one rank only): every match "
                         "factor is run again against everyone's smoothed belief (TrueSkill-Through-Time)")
    ap.add_argument("--through-time-sweeps", type=int, default=None, metavar="N",
                    help="with --through-time: sweeps over the history (default 8)")
    ap.add_argument("--through-time-track", default=None, metavar="TRACK",
                    help="with --through-time: the shared track (default) or a mode's")
    ap.add_argument("--pairs", default=None, metavar="ID[,ID...]",
                    help="with --records resident: print whom each player played with and against after the run "
                         "(JSON lines): the distinct partners and the most frequent team mates and opponents")
    ap.add_argument("--pairs-modes", default=None, metavar="MODE[,MODE...]",
                    help="with --pairs: count only the matches of these modes (default: all)")
    ap.add_argument("--pairs-top", type=int, default=None, metavar="N",
                    help="with --pairs: the N most frequent team mates and opponents (default 5)")
    ap.add_argument("--islands", action="store_true",
                    help="with --records resident: print the islands of the match graph after the run (one JSON "
                         "line): how many groups of players are connected through rated matches, and the ten largest")
    ap.add_argument("--islands-modes", default=None, metavar="MODE[,MODE...]",
                    help="with --islands: join only through the matches of these modes (default: all)")
    ap.add_argument("--islands-ranks", type=int, default=None, metavar="N",
                    help="with --islands: also deal whole islands onto N ranks and print the loads and the imbalance")
    ap.add_argument("--score", default=None, choices=["mode", "shared"],
                    help="with --records resident: score the ratings as predictions on each match's mode track or "
                         "the shared track and print the scorecard after the run (one JSON line; one rank only)")
    ap.add_argument("--score-modes", default=None, metavar="MODE[,MODE...]",
                    help="with --score: count only the matches of these modes (default: all)")
    ap.add_argument("--expect", default=None, metavar="ID[,ID...]",
                    help="with --records resident: hold each player up against the pre-match predictions after the "
                         "run (JSON lines; one rank only): expected against actual wins, z score, and the strength "
                         "of team mates against opponents; then one line of the strongest outliers")
    ap.add_argument("--expect-track", default=None, choices=["mode", "shared"],
                    help="with --expect: predict on each match's mode track (default) or the shared track")
    ap.add_argument("--expect-modes", default=None, metavar="MODE[,MODE...]",
                    help="with --expect: count only the matches of these modes (default: all)")
    ap.add_argument("--expect-outliers", type=int, default=None, metavar="N",
                    help="with --expect: the N players furthest above their expectation (default 10)")
    ap.add_argument("--export-records", default=None, metavar="PATH",
                    help="with --records resident: write the arena to PATH (+ PATH.json; .rN appended on N ranks)")
    ap.add_argument("--arena-free-bytes", type=float, default=None,
                    help="plan the arena against this many free bytes instead of the device's")
    ap.add_argument("--ladder", default=None, metavar="TRACK[,TRACK...]",
                    help="print the final roster's ladder of each track after the run (JSON lines): shared or a "
                         "mode, ranked by conservative skill mu - sigma, ties by player id")
    ap.add_argument("--ladder-top", type=int, default=10, metavar="K", help="with --ladder: the best K players")
    ap.add_argument("--ladder-rank", default=None, metavar="ID[,ID...]",
                    help="with --ladder: also the rank, score and percentile of these players")
    ap.add_argument("--matchmake", default=None, metavar="MODE:K:Q",
                    help="after the run, form balanced KvK lobbies on MODE from a queue of Q distinct players drawn "
                         "with the run's seed, and print what balancing bought (one JSON line)")
    ap.add_argument("--sweeps", type=int, default=ecfg.sweeps, help="causal sweeps per window (N ranks)")
    ap.add_argument("--digests", action="store_true", help="print every window's digest")
    args = ap.parse_args(argv)
    rank, size, dev = init_from_env()
    spec = RerateSpec(total_matches=int(args.matches), players=int(args.players),
                      team_size=args.team_size, window=int(args.window), seed=args.seed)
    resident = args.records == "resident"
    if (args.history or args.export_records) and not resident:
        ap.error("--history and --export-records need --records resident")
    if args.careers and not resident:
        ap.error("--careers needs --records resident")
    if (args.careers_modes or args.careers_track != "shared") and not args.careers:
        ap.error("--careers-track and --careers-modes need --careers")
    career_modes = [m.strip() for m in (args.careers_modes or "").split(",") if m.strip()] or None
    try:
        career_ids = [int(p) for p in (args.careers or "").split(",") if p.strip()]
        for m in career_modes or ():
            mode_index(m)
    except ValueError as e:
        ap.error("--careers: %s" % e)
    if any(p < 0 or p >= spec.players for p in career_ids):
        ap.error("--careers ids must lie in [0, %d)" % spec.players)
    if args.hindsight and not resident:
        ap.error("--hindsight needs --records resident")
    if args.hindsight_track and not args.hindsight:
        ap.error("--hindsight-track needs --hindsight")
    if args.hindsight and size > 1:
        ap.error("--hindsight chains the whole history: it runs on one rank")
    hindsight_track = args.hindsight_track or "shared"
    try:
        hindsight_ids = [int(p) for p in (args.hindsight or "").split(",") if p.strip()]
        track_of(hindsight_track)
    except ValueError as e:
        ap.error("--hindsight: %s" % e)
    if any(p < 0 or p >= spec.players for p in hindsight_ids):
        ap.error("--hindsight ids must lie in [0, %d)" % spec.players)
    if args.through_time and not resident:
        ap.error("--through-time needs --records resident")
    if (args.through_time_track or args.through_time_sweeps is not None) and not args.through_time:
        ap.error("--through-time-track and --through-time-sweeps need --through-time")
    if args.through_time and size > 1:
        ap.error("--through-time chains the whole history: it runs on one rank")
    tt_track = args.through_time_track or "shared"
    tt_sweeps = 8 if args.through_time_sweeps is None else args.through_time_sweeps
    try:
        tt_ids = [int(p) for p in (args.through_time or "").split(",") if p.strip()]
        track_of(tt_track)
        if tt_sweeps < 0:
            raise ValueError("sweeps must be >= 0, got %d" % tt_sweeps)
    except ValueError as e:
        ap.error("--through-time: %s" % e)
    if any(p < 0 or p >= spec.players for p in tt_ids):
        ap.error("--through-time ids must lie in [0, %d)" % spec.players)
    if args.pairs and not resident:
        ap.error("--pairs needs --records resident")
    if (args.pairs_modes or args.pairs_top is not None) and not args.pairs:
        ap.error("--pairs-modes and --pairs-top need --pairs")
    pair_modes = [m.strip() for m in (args.pairs_modes or "").split(",") if m.strip()] or None
    pair_top = 5 if args.pairs_top is None else args.pairs_top
    try:
        pair_ids = [int(p) for p in (args.pairs or "").split(",") if p.strip()]
        for m in pair_modes or ():
            mode_index(m)
    except ValueError as e:
        ap.error("--pairs: %s" % e)
    if any(p < 0 or p >= spec.players for p in pair_ids):
        ap.error("--pairs ids must lie in [0, %d)" % spec.players)
    if pair_top < 0:
        ap.error("--pairs-top must be >= 0")
    if args.islands and not resident:
        ap.error("--islands needs --records resident")
    if (args.islands_modes or args.islands_ranks is not None) and not args.islands:
        ap.error("--islands-modes and --islands-ranks need --islands")
    island_modes = [m.strip() for m in (args.islands_modes or "").split(",") if m.strip()] or None
    try:
        for m in island_modes or ():
            mode_index(m)
    except ValueError as e:
        ap.error("--islands-modes: %s" % e)
    if args.islands_ranks is not None and args.islands_ranks < 1:
        ap.error("--islands-ranks must be >= 1")
    if args.score and not resident:
        ap.error("--score needs --records resident")
    if args.score_modes and not args.score:
        ap.error("--score-modes needs --score")
    if args.score and size > 1:
        ap.error("--score chains the whole history in order: it runs on one rank")
    score_modes = [m.strip() for m in (args.score_modes or "").split(",") if m.strip()] or None
    try:
        for m in score_modes or ():
            mode_index(m)
    except ValueError as e:
        ap.error("--score-modes: %s" % e)
    if args.expect and not resident:
        ap.error("--expect needs --records resident")
    if (args.expect_track or args.expect_modes or args.expect_outliers is not None) and not args.expect:
        ap.error("--expect-track, --expect-modes and --expect-outliers need --expect")
    if args.expect and size > 1:
        ap.error("--expect chains the whole history in order: it runs on one rank")
    expect_modes = [m.strip() for m in (args.expect_modes or "").split(",") if m.strip()] or None
    expect_top = 10 if args.expect_outliers is None else args.expect_outliers
    try:
        expect_ids = [int(p) for p in (args.expect or "").split(",") if p.strip()]
        for m in expect_modes or ():
            mode_index(m)
    except ValueError as e:
        ap.error("--expect: %s" % e)
    if any(p < 0 or p >= spec.players for p in expect_ids):
        ap.error("--expect ids must lie in [0, %d)" % spec.players)
    if expect_top < 0:
        ap.error("--expect-outliers must be >= 0")
    if args.ladder_rank and not args.ladder:
        ap.error("--ladder-rank needs --ladder")
    ladder_tracks = [t.strip() for t in (args.ladder or "").split(",") if t.strip()]
    ladder_ids = [int(p) for p in (args.ladder_rank or "").split(",") if p.strip()]
    try:
        for t in ladder_tracks:
            track_index(t)
    except ValueError as e:
        ap.error(str(e))
    if any(p < 0 or p >= spec.players for p in ladder_ids):
        ap.error("--ladder-rank ids must lie in [0, %d)" % spec.players)
    mm = None
    if args.matchmake:
        try:
            mode, k, q = args.matchmake.split(":")
            mm = (mode, int(k), int(q))
            mode_index(mode)
            if not 1 <= mm[1] <= 5 or not 0 <= mm[2] <= spec.players:
                raise ValueError("K must be 1..5 and Q 0..%d" % spec.players)
        except ValueError as e:
            ap.error("--matchmake MODE:K:Q: %s" % e)
    arena = None
    try:
        if resident:
            plan = RecordArena.plan(spec.total_matches, spec.team_size, args.device or dev, size=size,
                                    roster_players=spec.players, window=spec.window,
                                    free_bytes=None if args.arena_free_bytes is None else int(args.arena_free_bytes))
            if rank == 0:
                print(json.dumps({"arena_plan": plan}), flush=True)
            if not plan["fits"]:
                print("the record arena does not fit: %d bytes per rank + %d roster bytes would leave %d of %d free "
                      "bytes, less than the reserve of %d; use fewer matches, more ranks or another --records mode"
                      % (plan["arena_bytes_per_rank"], plan["roster_bytes"], plan["left_bytes"], plan["free_bytes"],
                         plan["reserve_bytes"]), file=sys.stderr, flush=True)
                return 2
            roster0 = None
            if args.score or expect_ids or tt_ids:
                roster0 = start_roster(spec, args.checkpoint_dir, torch.device(args.device or dev))
            res, roster, arena = rerate_resident(spec, args.device or dev, args.checkpoint_dir, plan=plan,
                                                 checkpoint_every=args.checkpoint_every,
                                                 fault_kill_after=args.fault_kill_after, comm_dtype=args.comm_dtype,
                                                 sweeps=args.sweeps)
            res.pop("arena_plan", None)  # printed above
        else:
            res, roster = run(spec, args.device or dev, args.checkpoint_dir, args.checkpoint_every,
                              args.fault_kill_after, comm_dtype=args.comm_dtype, records=args.records,
                              sweeps=args.sweeps)
    except InjectedFault:
        if rank == 0:
            print(json.dumps({"fault_injected_after_windows": args.fault_kill_after}), flush=True)
        raise
    if rank == 0:
        digs = res.pop("window_digests", None)
        if digs is not None and not args.digests:  # a compact fingerprint instead of every window
            res["digest_fingerprint"] = float(sum(sum(v) for v in digs.values()))
        elif digs is not None:
            res["window_digests"] = digs
        import hashlib  # bit-exact: sha256 of every (mu, sigma) of the final roster

        res["roster_sha256"] = hashlib.sha256(
            roster.state[:, 0::2].contiguous().cpu().numpy().tobytes()).hexdigest()
        if arena is not None:
            res["arena_rows"], res["arena_first_match"] = arena.filled, arena.first_match
        print(json.dumps(dict(res, n_ranks=size, spec=asdict(spec))), flush=True)
    if args.history:
        ids = [int(p) for p in args.history.split(",") if p.strip()]
        hist = arena.history(ids, spec.players, stream_records(spec, arena.device))  # this rank's hits
        for p in ids:
            print(json.dumps(dict(_timeline(hist, p), rank=rank)), flush=True)
    if career_ids:
        table = arena.careers(spec.players, stream_records(spec, arena.device), track=args.careers_track,
                              modes=career_modes)  # this rank's blocks
        for line in career_lines(table, career_ids):
            print(json.dumps(dict(line, rank=rank)), flush=True)
    if pair_ids:
        # the player filter: however long the history, only these players' rows are held
        table = arena.pairs(spec.players, stream_records(spec, arena.device), modes=pair_modes,
                            players=pair_ids)  # this rank's blocks
        for line in pair_lines(table, pair_ids, pair_top):
            print(json.dumps(dict(line, rank=rank)), flush=True)
    if hindsight_ids:
        curves = arena.hindsight(spec.players, stream_records(spec, arena.device), hindsight_ids,
                                 track=hindsight_track)
        for line in hindsight_lines(curves, hindsight_ids, hindsight_track):
            print(json.dumps(line), flush=True)
    if tt_ids:
        curves = arena.through_time(roster0, stream_records(spec, arena.device), tt_ids, sweeps=tt_sweeps,
                                    track=tt_track)
        for line in through_time_lines(curves, tt_ids, tt_track):
            print(json.dumps(line), flush=True)
    if args.islands:
        isl = arena.islands(spec.players, stream_records(spec, arena.device), modes=island_modes)  # this rank's blocks
        print(json.dumps(dict(islands_line(isl, 10, args.islands_ranks), rank=rank)), flush=True)
    if args.score:
        card = arena.scorecard(roster0, stream_records(spec, arena.device), track=args.score, modes=score_modes)
        print(json.dumps({"scorecard": card.summary()}), flush=True)
    if expect_ids:
        exp = arena.expectations(roster0, stream_records(spec, arena.device), track=args.expect_track or "mode",
                                 modes=expect_modes)
        for line in expectation_lines(exp, expect_ids):
            print(json.dumps(line), flush=True)
        print(json.dumps(outliers_line(exp, expect_top)), flush=True)
    if ladder_tracks and rank == 0:  # the roster is replicated after the last merge
        for line in ladder_lines(roster, ladder_tracks, args.ladder_top, ladder_ids):
            print(json.dumps(line), flush=True)
    if mm is not None and rank == 0:
        print(json.dumps(matchmake_line(roster, *mm, seed=spec.seed)), flush=True)
    if args.export_records:
        path = args.export_records + (".r%d" % rank if size > 1 else "")
        print(json.dumps({"exported": path, "bytes": arena.export(path), "rank": rank}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
