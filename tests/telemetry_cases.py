"""Shared cases of the telemetry-aggregation tests (test_telemetry_oracle.py, CPU and
``-m gpu``): an event builder that places every event deliberately, an exact per-event
oracle of K8 written from the prose contract of csrc/telemetry_core.h, the case families
(density, wrap, values, offset, fused) and the one checker that every path goes through.

The oracle imports nothing from ``analyzer_amd``: it walks ``(evoff, events)`` event by
event, attributes an event to the match whose CSR range holds it iff its 16-bit tag
equals that match mod 2^16 and its slot is < 2K, and returns per cell the exactly
rounded sum (``math.fsum`` over the fp32 values widened to float), the number of summed
events, the sum of magnitudes and the non-finite verdict.  The error budget B and the
exactness argument for grid values are derived in docs/ARCHITECTURE.md ("Telemetry
error budget"), not fitted; nothing is classified by an output of the code under test.
"""
import functools
import math
import zlib
from typing import NamedTuple

import numpy as np
import torch

U = 2.0 ** -24
INF = float("inf")
NAN = float("nan")
FEATURES = 8
COUNT_COLS = (0, 1, 2, 7)  # kills, deaths, assists, events: exact integers
SUM_COLS = (3, 4, 5, 6)    # damage, gold, farm, healing: type t adds its value to column t
EXACT, BOUND = "exact", "bound"
FINITE, POS_INF, NEG_INF, IS_NAN = 0, 1, 2, 3

M_SMALL = 143              # two full 63-match spans + 17; eight full 16-match tiles + 15
SPAN = 63                  # matches per wave of the standalone MFMA kernel
CHUNK = 32                 # events per MFMA
WRAP_M = 65536 + 200
GRID = 2.0 ** -8           # grid values are signed multiples of this
GRID_CELL_MAX = 2.0 ** 16  # per cell sum |v| stays below: partial sums < 2^24 grid units
WIDE_CELL_MAX = 2.0 ** 120
NAN_PAYLOADS = (0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF)


class Bits(int):
    """An event value given as its 32 bits (NaN payloads)."""


def bits_of(v) -> int:
    if isinstance(v, Bits):
        return int(v) & 0xFFFFFFFF
    f = np.float32(v)
    assert math.isnan(v) or float(f) == float(v), "%r is not an fp32 value" % (v,)
    return int(f.view(np.uint32))


# ---------------------------------------------------------------- the event builder
def build_events(matches, lead=(), trail=()):
    """``evoff`` / ``events`` from per-match lists of ``(slot, type, value[, tag])``: the
    tag defaults to the match's index (mod 2^16).  ``lead`` / ``trail``: events in front
    of ``evoff[0]`` and behind ``evoff[M]``, owned by no match."""
    meta, val, off = [], [], []

    def put(ev, m):
        slot, typ, v = ev[:3]
        tag = ev[3] if len(ev) > 3 and ev[3] is not None else m
        assert 0 <= slot < 256 and 0 <= typ < 256
        meta.append(slot | (typ << 8) | ((tag & 0xFFFF) << 16))
        val.append(bits_of(v))

    for ev in lead:
        put(ev, 0)
    off.append(len(meta))
    for m, evs in enumerate(matches):
        for ev in evs:
            put(ev, m)
        off.append(len(meta))
    for ev in trail:
        put(ev, len(matches) - 1)
    events = np.empty((len(meta), 2), dtype=np.uint32)
    events[:, 0] = meta
    events[:, 1] = val
    return torch.tensor(off, dtype=torch.int64), torch.from_numpy(events.view(np.int32))


# ------------------------------------------------------------------------ the oracle
class Oracle(NamedTuple):
    exact: np.ndarray    # [M, 2K, 8] float64: counts, and the exactly rounded sums
    n: np.ndarray        # [M, 2K, 8] int64: events summed into the cell (columns 3..6)
    sabs: np.ndarray     # [M, 2K, 8] float64: sum of |v| over the finite summed values
    verdict: np.ndarray  # [M, 2K, 8] int8: FINITE, POS_INF, NEG_INF, IS_NAN
    malformed: int


def oracle(evoff: torch.Tensor, events: torch.Tensor, K: int) -> Oracle:
    off = [int(x) for x in evoff.tolist()]
    ev = events.numpy()
    meta = [int(x) & 0xFFFFFFFF for x in ev[:, 0].tolist()]
    with np.errstate(invalid="ignore"):  # signalling NaN payloads
        vals = ev[:, 1].copy().view(np.float32).astype(np.float64).tolist()
    M, S = len(off) - 1, 2 * K
    counts, terms = {}, {}
    malformed = 0
    for m in range(M):
        for e in range(off[m], off[m + 1]):
            x = meta[e]
            slot, typ, tag = x & 0xFF, (x >> 8) & 0xFF, x >> 16
            if tag != m % 65536 or slot >= S:
                malformed += 1
                continue
            counts[m, slot, 7] = counts.get((m, slot, 7), 0) + 1
            if typ <= 2:
                counts[m, slot, typ] = counts.get((m, slot, typ), 0) + 1
            elif typ <= 6:
                terms.setdefault((m, slot, typ), []).append(vals[e])
    exact = np.zeros((M, S, FEATURES))
    n = np.zeros((M, S, FEATURES), dtype=np.int64)
    sabs = np.zeros((M, S, FEATURES))
    verdict = np.zeros((M, S, FEATURES), dtype=np.int8)
    for cell, c in counts.items():
        exact[cell] = c
    for cell, vs in terms.items():
        fin = [v for v in vs if math.isfinite(v)]
        pos, neg = any(v == INF for v in vs), any(v == -INF for v in vs)
        n[cell] = len(vs)
        sabs[cell] = math.fsum(abs(v) for v in fin)
        if any(math.isnan(v) for v in vs) or (pos and neg):
            verdict[cell], exact[cell] = IS_NAN, NAN
        elif pos:
            verdict[cell], exact[cell] = POS_INF, INF
        elif neg:
            verdict[cell], exact[cell] = NEG_INF, -INF
        else:
            exact[cell] = math.fsum(fin)
    return Oracle(exact, n, sabs, verdict, malformed)


def budget(orc: Oracle) -> np.ndarray:
    """B = 1.02 (n + 2) 2^-24 sum|v| per cell (docs/ARCHITECTURE.md)."""
    return 1.02 * (orc.n + 2) * U * orc.sabs


# ----------------------------------------------------------------------- the checker
def check(got, bad, orc: Oracle, cls: str, label: str, factor: float = 1.0) -> float:
    """The assertions of every path.  ``got`` [M, 2K, 8] fp32 was pre-filled with -1
    before the launch; ``bad`` is the path's malformed count (None: the path reports
    none).  Returns the worst err / B over the finite summed cells (0 for EXACT)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == orc.exact.shape, (got.dtype, got.shape)
    g = got.astype(np.float64)
    stale = (g == -1.0) & ~(orc.exact == -1.0)
    assert not stale.any(), "%s: row never written at %s" % (label, np.argwhere(stale)[:4].tolist())
    if bad is not None:
        assert int(bad) == orc.malformed, "%s: malformed %d, oracle %d" % (label, int(bad), orc.malformed)
    cc = list(COUNT_COLS)
    wrong = g[..., cc] != orc.exact[..., cc]
    assert not wrong.any(), "%s: counts differ at %s" % (label, np.argwhere(wrong)[:4].tolist())
    sc = list(SUM_COLS)
    gs, ex, v = g[..., sc], orc.exact[..., sc], orc.verdict[..., sc]
    assert (gs[v == POS_INF] == INF).all(), label + ": +Inf cells"
    assert (gs[v == NEG_INF] == -INF).all(), label + ": -Inf cells"
    assert np.isnan(gs[v == IS_NAN]).all(), label + ": NaN cells"
    fin = v == FINITE
    if cls == EXACT:
        wrong = fin & ~(gs == ex)  # numerically: -0.0 == 0.0
        assert not wrong.any(), "%s: %d sums differ, first %s got %r exact %r" % (
            label, int(wrong.sum()), np.argwhere(wrong)[:1].tolist(), gs[wrong][:1].tolist(),
            ex[wrong][:1].tolist())
        return 0.0
    assert cls == BOUND
    B = budget(orc)[..., sc][fin]
    err = np.abs(gs[fin] - ex[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(B > 0, err / B, np.where(err == 0, 0.0, INF))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("tele-budget %s worst err/B = %.4f" % (label, worst))
    assert worst <= factor, "%s: worst err / B = %r (> %r)" % (label, worst, factor)
    return worst


def canon_bits(t: torch.Tensor) -> torch.Tensor:
    """fp32 bits with every NaN mapped to one pattern (payloads are not specified)."""
    b = t.detach().cpu().contiguous().view(torch.int32).clone()
    b[torch.isnan(t.detach().cpu())] = 0x7FC00000
    return b


# ------------------------------------------------------------------ value generators
def rng_of(name: str, K: int):
    return np.random.default_rng(zlib.crc32(name.encode()) * 8 + K)


def sign(rng) -> float:
    return 1.0 if rng.random() < 0.5 else -1.0


class GridValues:
    """Signed multiples of 2^-8.  The first summed value of a cell is, half the time, a
    full 24-bit significand (odd k in [2^23, 3 2^22): all three bf16 split parts are
    non-zero); the others are k <= 512.  Per cell sum|v| < 2^16 (asserted), so every
    partial sum, in any order and in each split column, is a multiple of 2^-8 below
    2^24 2^-8: exact in fp32."""

    def __init__(self, rng):
        self.rng = rng
        self.sabs = {}

    def __call__(self, cell) -> float:
        r = self.rng
        if cell[2] not in SUM_COLS:
            return float(r.integers(1, 513)) * GRID
        used = self.sabs.get(cell, 0.0)
        if used == 0.0 and r.random() < 0.5:
            k = int(r.integers(2 ** 23, 3 * 2 ** 22)) | 1
        else:
            k = int(r.integers(1, 513))
        v = sign(r) * k * GRID
        self.sabs[cell] = used + abs(v)
        assert self.sabs[cell] < GRID_CELL_MAX, "grid cell bound"
        return v


def full_mantissa(rng, elo: int, ehi: int) -> float:
    """A signed fp32 value with 23 random fraction bits, magnitude log-uniform in
    [2^elo, 2^ehi)."""
    return sign(rng) * (1.0 + int(rng.integers(0, 2 ** 23)) * 2.0 ** -23) * 2.0 ** int(rng.integers(elo, ehi))


def fill(rng, counts, K, value, slot=None):
    """``counts[m]`` events per match, slots uniform (or all on ``slot``), types uniform
    in 0..7, values from ``value((match, slot, type))``."""
    S = 2 * K
    out = []
    for m, c in enumerate(counts):
        evs = []
        for _ in range(int(c)):
            s = slot if slot is not None else int(rng.integers(0, S))
            t = int(rng.integers(0, 8))
            evs.append((s, t, value((m, s, t))))
        out.append(evs)
    return out


def max_row_tiles_per_chunk(evoff: torch.Tensor, K: int, span: int = SPAN) -> int:
    """The most 16-row tiles that one 32-event chunk of a span's stream reaches, first
    to last row of the matches holding its first and last event (read from evoff)."""
    off = [int(x) for x in evoff.tolist()]
    M, S, best = len(off) - 1, 2 * K, 0
    for m0 in range(0, M, span):
        m1 = min(M, m0 + span)
        owner = [m - m0 for m in range(m0, m1) for _ in range(off[m + 1] - off[m])]
        for p in range(0, len(owner), CHUNK):
            a, b = owner[p], owner[min(p + CHUNK, len(owner)) - 1]
            best = max(best, ((b + 1) * S - 1) // 16 - (a * S) // 16 + 1)
    return best


# --------------------------------------------------------------------------- the cases
class Case(NamedTuple):
    name: str
    K: int
    cls: str              # EXACT: sums compare with ==; BOUND: |got - exact| <= B
    evoff: torch.Tensor
    events: torch.Tensor

    @property
    def M(self) -> int:
        return self.evoff.numel() - 1

    @property
    def label(self) -> str:
        return "%s K=%d" % (self.name, self.K)


def span_total_counts(rng, totals):
    """Per-match counts whose sums over the consecutive 63-match spans are ``totals``
    (the last span is the partial one)."""
    counts = []
    for i, total in enumerate(totals):
        nm = min(SPAN, M_SMALL - SPAN * i)
        c = np.full(nm, total // nm)
        c[rng.permutation(nm)[: total - int(c.sum())]] += 1
        assert int(c.sum()) == total
        counts.extend(int(x) for x in c)
    assert len(counts) == M_SMALL
    return counts


def burst_counts():
    c = [0] * M_SMALL
    c[5], c[135] = 5000, 3000  # neighbours empty; the second burst in the partial span
    return c


DENSITY = {
    "zero": lambda r: [0] * M_SMALL,
    "bernoulli": lambda r: r.integers(0, 2, M_SMALL),
    "one": lambda r: [1] * M_SMALL,
    "u0_2": lambda r: r.integers(0, 3, M_SMALL),
    "u0_6": lambda r: r.integers(0, 7, M_SMALL),
    "fixed31": lambda r: [31] * M_SMALL,
    "fixed32": lambda r: [32] * M_SMALL,
    "fixed33": lambda r: [33] * M_SMALL,
    "fixed63": lambda r: [63] * M_SMALL,
    "fixed64": lambda r: [64] * M_SMALL,
    "fixed65": lambda r: [65] * M_SMALL,
    "span511_512_513": lambda r: span_total_counts(r, (511, 512, 513)),
    "span513_511_512": lambda r: span_total_counts(r, (513, 511, 512)),
    "bursty": lambda r: burst_counts(),
}
ONE_SLOT = ("one", "u0_2", "fixed33", "bursty")  # variants with every event on the last slot
MIN_TILES_ONE = {1: 4, 2: 8, 3: 12, 4: 16, 5: 18}  # K = 5: a chunk crosses >= 18 row tiles

DENSITY_NAMES = ["density/" + k for k in DENSITY] + ["density/%s/one_slot" % k for k in ONE_SLOT]
VALUE_NAMES = ["values/" + k for k in ("grid", "general", "cancel", "wide", "nonfinite", "types", "negzero")]
SMALL_NAMES = DENSITY_NAMES + VALUE_NAMES + ["offset"]
ALL_NAMES = SMALL_NAMES + ["wrap"]


def density_case(name, K, rng):
    parts = name.split("/")
    counts = DENSITY[parts[1]](rng)
    slot = 2 * K - 1 if len(parts) > 2 else None
    evoff, events = build_events(fill(rng, counts, K, GridValues(rng), slot))
    if parts[1] == "one":
        # the sparse stream must keep crossing many row tiles per chunk (the re-window
        # loop of telemetry_tile_mfma): a property of the case, read from evoff
        assert max_row_tiles_per_chunk(evoff, K) >= MIN_TILES_ONE[K]
    if parts[1].startswith("span"):
        off = evoff.tolist()
        tot = [off[min(M_SMALL, m + SPAN)] - off[m] for m in range(0, M_SMALL, SPAN)]
        assert sorted(tot) == [511, 512, 513]
    return Case(name, K, EXACT, evoff, events)


def wrap_matches(rng, K, M, grid):
    """0-2 events per match; around the 16-bit tag wrap every match has valid events
    (tagged m & 0xffff past it) and the three malformed neighbours of the issue."""
    counts = rng.integers(0, 3, M)
    counts[65530:65550] = 2
    matches = fill(rng, counts, K, grid)
    matches[65535].insert(1, (0, 3, 7.0, 0))        # names match 65536: malformed
    matches[65536].insert(1, (1, 3, 9.0, 65535))    # names match 65535: malformed
    matches[65540].insert(0, (0, 4, 11.0, 65541))   # a same-span neighbour past the wrap
    return matches


def values_case(name, K, rng):
    kind = name.split("/")[1]
    S = 2 * K
    cls = EXACT
    if kind == "grid":
        matches = fill(rng, rng.integers(0, 41, M_SMALL), K, GridValues(rng))
    elif kind == "general":
        cls = BOUND
        matches = fill(rng, rng.integers(0, 41, M_SMALL), K, lambda c: full_mantissa(rng, -20, 20))
    elif kind == "cancel":
        cls = BOUND
        matches = []
        for m in range(M_SMALL):
            evs = []
            for _ in range(int(rng.integers(0, 5))):
                s, t = int(rng.integers(0, S)), int(rng.integers(3, 7))
                a = full_mantissa(rng, 10, 20)
                evs += [(s, t, a), (s, t, -a)]
                evs += [(s, t, full_mantissa(rng, -10, 0)) for _ in range(int(rng.integers(0, 7)))]
            matches.append([evs[i] for i in rng.permutation(len(evs))])
    elif kind == "wide":
        cls = BOUND

        def wide(cell):  # per cell: only tiny values, only 2^100-scale ones, or both
            mode = sum(cell) % 3
            if mode == 1 or (mode == 2 and rng.random() < 0.5):
                return full_mantissa(rng, 100, 101)
            # 2^-100-scale, and the smallest binade whose split parts bf16 still holds:
            # the last bit of a value in [2^-110, 2^-109) is 2^-133, bf16's smallest subnormal
            e = -100 if rng.random() < 0.5 else -110
            return full_mantissa(rng, e, e + 1)
        matches = fill(rng, rng.integers(0, 41, M_SMALL), K, wide)
    elif kind == "nonfinite":
        grid = GridValues(rng)
        matches = fill(rng, rng.integers(8, 41, M_SMALL), K, grid)
        nan = lambda i: Bits(NAN_PAYLOADS[i % len(NAN_PAYLOADS)])
        for i, m in enumerate((0, 3, 20, 31, 62, 63, 64, 79, 100, 125, 126, 130, 141, 142)):
            s, t = i % S, 3 + i % 4
            o = (s + 1) % S
            add = [
                [(s, t, INF)],
                [(s, t, INF), (s, t, -INF)],
                [(s, t, nan(i)), (s, t, grid((m, s, t)))],
                [(s, t, -INF), (s, t, grid((m, s, t)))],
                [(s, t, nan(i)), (s, t, nan(i + 1)), (s, t, INF)],
            ][i % 5]
            # non-finite values on events that must not contribute them
            add += [(o, 0, nan(i)), (o, 1, INF), (o, 2, -INF), (o, 7, nan(i + 2)), (o, 200, INF),
                    (S, t, nan(i)), (255, t, INF), (o, t, INF, m + 1), (o, t, nan(i), m + 65535)]
            for ev in add:
                matches[m].insert(int(rng.integers(0, len(matches[m]) + 1)), ev)
    elif kind == "types":
        grid = GridValues(rng)
        matches = fill(rng, rng.integers(0, 11, M_SMALL), K, grid)
        for t in range(256):  # every type byte, twice; 8..255 only count
            for m in ((t * 5) % M_SMALL, (t * 7 + 3) % M_SMALL):
                s = int(rng.integers(0, S))
                matches[m].insert(int(rng.integers(0, len(matches[m]) + 1)), (s, t, grid((m, s, t))))
        assert {(ev[1]) for evs in matches for ev in evs} == set(range(256))
    elif kind == "negzero":
        grid = GridValues(rng)
        matches = fill(rng, rng.integers(0, 21, M_SMALL), K, grid, slot=S - 1)
        for m in range(0, M_SMALL, 3):  # slot 0: cells whose only summed values are -0.0
            t = 3 + m % 4
            for _ in range(1 + m % 3):
                matches[m].insert(int(rng.integers(0, len(matches[m]) + 1)), (0, t, -0.0))
            if m % 2:
                matches[m].append((0, 3 + (m + 1) % 4, 0.0))
                matches[m].append((0, 3 + (m + 1) % 4, -0.0))
    else:
        raise KeyError(name)
    assert max(len(evs) for evs in matches) <= 60
    return Case(name, K, cls, *build_events(matches))


def offset_case(K, rng):
    """evoff[0] = 7: seven unowned events in front and five behind evoff[M], NaN values
    and valid-looking tags; neither counted nor malformed."""
    matches = fill(rng, rng.integers(0, 7, M_SMALL), K, GridValues(rng))
    nan = Bits(NAN_PAYLOADS[0])
    lead = [(i % (2 * K), 3 + i % 4, nan, 0) for i in range(7)]
    trail = [(i % (2 * K), 3 + i % 4, nan, M_SMALL - 1) for i in range(5)]
    evoff, events = build_events(matches, lead, trail)
    assert int(evoff[0]) == 7 and events.shape[0] == int(evoff[-1]) + 5
    return Case("offset", K, EXACT, evoff, events)


@functools.lru_cache(maxsize=None)
def case(name: str, K: int) -> Case:
    rng = rng_of(name, K)
    if name.startswith("density/"):
        c = density_case(name, K, rng)
    elif name.startswith("values/"):
        c = values_case(name, K, rng)
    elif name == "offset":
        c = offset_case(K, rng)
    elif name == "wrap":
        c = Case(name, K, EXACT, *build_events(wrap_matches(rng, K, WRAP_M, GridValues(rng))))
    else:
        raise KeyError(name)
    if name == "values/wide":
        assert float(oracle_of(c).sabs.max()) < WIDE_CELL_MAX
    return c


_ORACLES = {}


def oracle_of(c: Case) -> Oracle:
    """The oracle of a case, computed once and shared (read-only) by every test."""
    key = (c.name, c.K)
    if key not in _ORACLES:
        o = oracle(c.evoff, c.events, c.K)
        for a in o[:4]:
            a.setflags(write=False)
        _ORACLES[key] = o
    return _ORACLES[key]


# ---------------------------------------------------------------- the fused family
FUSED_P = 50
FUSED_SIZES = (2000, WRAP_M)
# events per match placed on rated and on tele-only matches alike: none, one, around the
# inline path's kTeleInline = 64 remainder loop, around the 8 loads per lane of a 2-lane
# (1v1: 16 events) and a 10-lane (5v5: 70 events, capped by 64) group, and many
FUSED_COUNTS = (0, 1, 63, 64, 65, 200, 15, 16, 17, 69, 70, 71)


class FusedCase(NamedTuple):
    case: Case
    clean: Case           # the same window without its malformed events (a second launch)
    rec: torch.Tensor     # [M, 2K + 2] stream records (CPU)
    status: np.ndarray    # per match, from the host rater: 0 = rated, else tele-only


def fused_roster(device="cpu"):
    from analyzer_amd.ops.synth import RosterSpec, make_roster

    return make_roster(RosterSpec(num_players=FUSED_P, seed=9), device=device)


def stream_for(K: int, M: int) -> torch.Tensor:
    """A window of M matches over few players (long dependency chains, stale retries on
    the device) with AFK, invalid-roster, unsupported and tied matches."""
    from analyzer_amd.ops.synth import StreamSpec, make_stream

    spec = StreamSpec(team_size=K, seed=60 + K, p_afk=0.1, p_bad_rosters=0.05, p_unsupported=0.05,
                      p_tie=0.05)
    return make_stream(spec, M, FUSED_P, K=K)


@functools.lru_cache(maxsize=None)
def fused_case(K: int, M: int, values: str) -> FusedCase:
    from analyzer_amd.ops import rate as R

    name = "fused/%s/M%d" % (values, M)
    rng = rng_of(name, K)
    rec = stream_for(K, M)
    status = R.BatchRater().rate(fused_roster(), rec, K).status.numpy().copy()
    grid = GridValues(rng)
    value = grid if values == "grid" else (lambda c: full_mantissa(rng, -20, 20))
    counts = rng.integers(0, 3, M)
    L = len(FUSED_COUNTS)
    placed = {}
    for grp in (np.flatnonzero(status == 0), np.flatnonzero(status != 0)):
        cand = np.concatenate([grp[: 2 * L], grp[grp >= M - 230][: 2 * L]])
        assert len(cand) == 4 * L, "too few matches of one kind"
        for i, m in enumerate(cand):
            counts[m] = FUSED_COUNTS[i % L]
            placed.setdefault((status[m] == 0, FUSED_COUNTS[i % L]), []).append(int(m))
    # zero-event rated and zero-event tele-only matches, and every other count on both
    assert all((r, c) in placed for r in (True, False) for c in FUSED_COUNTS)
    if M > 65536:
        counts[65530:65550] = np.maximum(counts[65530:65550], 2)
    matches = fill(rng, counts, K, value)
    clean = [list(evs) for evs in matches]
    S = 2 * K
    for m in range(3, M, 97):  # malformed: wrong tag, slot out of range
        matches[m].insert(0, (0, 3, 5.0, m + 1))
        matches[m].append((S + m % 3, 4, 6.0))
    if M > 65536:
        matches[65535].insert(1, (0, 3, 7.0, 0))
        matches[65536].insert(1, (1, 3, 9.0, 65535))
        matches[65540].insert(0, (0, 4, 11.0, 65541))
    if values == "grid":  # non-finite values, on summed types and where they must not count
        for i, m in enumerate(range(5, M, 211)):
            s, t = i % S, 3 + i % 4
            add = [[(s, t, INF)], [(s, t, INF), (s, t, -INF)], [(s, t, Bits(NAN_PAYLOADS[i % 5]))],
                   [(s, t, -INF)]][i % 4]
            add += [(s, i % 3, INF), (s, 7, NAN), (s, 200, -INF), (S, t, NAN), (s, t, INF, m + 2)]
            for ev in add:
                matches[m].insert(int(rng.integers(0, len(matches[m]) + 1)), ev)
                if not (ev[0] >= S or len(ev) > 3):
                    clean[m].append(ev)
    cls = EXACT if values == "grid" else BOUND
    return FusedCase(Case(name, K, cls, *build_events(matches)),
                     Case(name + "/clean", K, cls, *build_events(clean)), rec, status)
