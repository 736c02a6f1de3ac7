"""Shared cases of the posterior-merge tests (test_merge.py, CPU and ``-m gpu``):
hand-built rosters and summed messages, an fp64 oracle of K9 written from its prose
specification (the comments of csrc/sweep_core.h, the docstring of parallel/sweep.py,
docs/ARCHITECTURE.md), the per-element error budgets of every output, and a numpy-fp32
transcription of the per-track functions that the CPU tests hold to the same budgets (and
whose mutations they must catch).

The oracle imports nothing from ``analyzer_amd`` but ``RaterConfig``, ``vst_table`` and
the roster container.  It takes the fp32 inputs as exact and evaluates in fp64: every
budget below is relative to the magnitudes of the operands that cancel, against which an
fp64 rounding is 2^-29 of the budget, so no formula needs more digits.  The budgets are
derived in docs/ARCHITECTURE.md ("Merge error budget"), not fitted.  The oracle alone
decides the branch of a case (idle, no base, natural sum, variance space, clamp,
non-finite); nothing is classified by an output of the code under test."""
import functools
import math

import numpy as np
import torch

from analyzer_amd.config import RaterConfig
from analyzer_amd.models.tiers import vst_table
from analyzer_amd.ops.rate import Roster

U = 2.0 ** -24
NAN = float("nan")
INF = float("inf")
UNKNOWN_SIGMA = float(RaterConfig().unknown_player_sigma)
VST = [float(v) for v in vst_table()]
SIGMAS = (1.0, 30.0, 166.667, 500.0, 2000.0)
MUS = (-3000.0, 0.0, 1500.0, 6000.0)
FLOOR_SCALED = float(np.float32(1e-6))
FLOOR_RAW = float(np.float32(1e-12))
TRACKS = 7
SIZES = (1, 31, 32, 33, 8 * 32 + 5)
SEEDS = {"none": (NAN, NAN, NAN), "points": (1800.0, 0.0, NAN), "tier": (NAN, NAN, 12.0)}
WIRE = {"fp16": torch.float16, "bf16": torch.bfloat16}


def f32(x):
    return float(np.float32(x))


def g(k):
    """gamma_k: the relative error bound of k chained fp32 roundings."""
    return k * U / (1.0 - k * U)


def amp(e):
    """e / (1 - e): a first-order relative error e with its higher orders (e < 1)."""
    return e / (1.0 - e) if e < 1.0 else INF


# ------------------------------------------------------------------ the oracle
def seed_of(attr):
    """The prior of a player with no shared rating, as the rating stores it (fp32):
    the larger of the non-NULL, non-zero rank points + 2/3 of the unknown-player sigma,
    else the tier table + that sigma; None where neither exists."""
    rr, rb, tier = (float(x) for x in attr[:3])
    rp = None
    if not math.isnan(rr) and rr != 0.0:
        rp = rr
    if not math.isnan(rb) and rb != 0.0 and (rp is None or rb > rp):
        rp = rb
    if rp is not None:
        sig = f32(np.float32(UNKNOWN_SIGMA) * np.float32(2.0 / 3.0))
        return f32(np.float32(rp) + np.float32(sig)), sig
    if math.isnan(tier) or tier != int(tier) or not -1 <= tier <= 29:
        return None
    return f32(np.float32(VST[int(tier) + 1]) + np.float32(UNKNOWN_SIGMA)), f32(UNKNOWN_SIGMA)


def base_of(t, c, c0, sd):
    """The common base of track t: its window-start value; NULL there: the seed for the
    shared track, the window-start shared value (else the seed) for a mode track."""
    if c is not None:
        return c
    if t > 0 and c0 is not None:
        return c0
    return sd


def oracle_message(t, c, c0, a, b, sd, scaled):
    """One rank's message of track t: start c, start shared c0, prior a, after b, seed sd
    (each (mu, sigma) or None).  -> (d_pi, d_tau, touched, B_d_pi, B_d_tau)."""
    had = a is not None
    changed = (b != a) if had else (b is not None)
    B = base_of(t, c, c0, sd)
    if not changed or B is None:
        return 0.0, 0.0, changed, 0.0, 0.0
    Bm, Bs = B
    if scaled:
        x1 = (Bs / b[1]) ** 2
        x0 = (Bs / a[1]) ** 2 if had else 1.0
        T1 = x1 * (b[0] - Bm)
        T0 = x0 * (a[0] - Bm) if had else 0.0
        return x1 - x0, T1 - T0, True, g(4) * (x1 + x0), g(6) * (abs(T1) + abs(T0))
    p1 = 1.0 / b[1] ** 2
    pm, ps = a if had else B
    p0 = 1.0 / ps ** 2
    t1, t0 = b[0] * p1, pm * p0
    return p1 - p0, t1 - t0, True, g(3) * (p1 + p0), g(4) * (abs(t1) + abs(t0))


def oracle_decode(t, c, c0, sd, dpi, dtau, m, scaled, e_dp=0.0, e_dt=0.0):
    """The decode of track t: start c, summed message (dpi, dtau) of m contributing ranks
    (``e_dp``, ``e_dt``: absolute errors the message carries, for the round-trip
    properties).  -> dict(out=(mu, sigma) or None, branch, clamp, B_mu, B_sg, rho)."""
    r = dict(out=c, branch="idle", clamp=False, B_mu=0.0, B_sg=0.0, rho=0.0)
    if not (math.isfinite(dpi) and math.isfinite(dtau)):
        return dict(r, branch="nonfinite", clamp=True)   # left at the start value, counted
    live = (dpi != 0.0 or dtau != 0.0) if c is not None else m != 0
    if not live:
        return r
    B = base_of(t, c, c0, sd)
    if B is None:
        return dict(r, branch="nobase")
    Bm, Bs = B
    pb = 1.0 if scaled else 1.0 / Bs ** 2
    S = dpi / pb
    floor = FLOOR_SCALED if scaled else FLOOR_RAW
    if S < 0.0 and m >= 2 and 1.0 + S / m > 0.0:
        # net loss over m >= 2 ranks: variance space, every rank lost the mean x
        x = 1.0 + S / m
        ex = g(1 if scaled else 4) * abs(S) / m + g(1) * x
        D = x + m * (1.0 - x)
        ratio = x / D
        rho = amp(ex / x + ((1 + m) * ex + g(2) * m * (1.0 - x)) / D + g(2))
        if scaled:
            num, e_num = dtau, 0.0
        else:
            A, Bt = dtau / pb, S * Bm
            num, e_num = A - Bt, g(5) * (abs(A) + abs(Bt))
        if scaled and not ratio > floor:
            q = dtau / floor
            mu, sg = Bm + q, Bs / math.sqrt(floor)
            return dict(out=(mu, sg), branch="clamp", clamp=True, rho=0.0,
                        B_mu=g(1) * abs(q) + g(1) * (abs(mu) + g(1) * abs(q)), B_sg=g(2) * sg)
        q = num / x
        e_q = (e_num + abs(num) * ex / x) / (x * (1.0 - ex / x)) + g(1) * abs(q) if ex < x else INF
        mu, sg = Bm + q, Bs / math.sqrt(ratio)
        return dict(out=(mu, sg), branch="var", clamp=False, rho=rho,
                    B_mu=e_q + g(1) * (abs(mu) + e_q), B_sg=sg * (rho / 2 * (1 + g(2)) + g(2)))
    # the natural-parameter sum: mu = mu_B + T / P (scaled), T / P (raw); sigma = sigma_B / sqrt(P), 1 / sqrt(P)
    if scaled:
        P, T = 1.0 + S, dtau
        eP, eT = g(1) * abs(P) + e_dp * (1 + U), e_dt
    else:
        tb = Bm * pb
        P, T = pb + dpi, tb + dtau
        eP, eT = g(3) * pb + g(1) * abs(P) + e_dp * (1 + U), g(4) * abs(tb) + g(1) * abs(T) + e_dt * (1 + U)
    if not P > floor:
        q = T / floor
        Eq = eT / floor * (1 + U) + U * abs(q)
        mu = Bm + q if scaled else q
        sg = (Bs if scaled else 1.0) / math.sqrt(floor)
        return dict(out=(mu, sg), branch="clamp", clamp=True, rho=0.0,
                    B_mu=Eq + (g(1) * (abs(mu) + Eq) if scaled else 0.0), B_sg=g(2) * sg)
    rp = eP / P
    q = T / P
    Eq = (eT + abs(T) * rp) / (P * (1.0 - rp)) * (1 + U) + U * abs(q) if rp < 1.0 else INF
    mu = Bm + q if scaled else q
    sg = (Bs if scaled else 1.0) / math.sqrt(P)
    return dict(out=(mu, sg), branch="nat", clamp=False, rho=rp,
                B_mu=Eq + (g(1) * (abs(mu) + Eq) if scaled else 0.0),
                B_sg=sg * (amp(rp) / 2 * (1 + g(2)) + g(2)))


def oracle_prefix_delta(t, c, c0, sd, rpi, rtau):
    """Scaled exclusive prefix (r_pi, r_tau) of track t -> raw increments
    (pi_B r_pi, pi_B (r_tau + mu_B r_pi)) and their budgets; zero without a base."""
    if rpi == 0.0 and rtau == 0.0:
        return 0.0, 0.0, 0.0, 0.0
    B = base_of(t, c, c0, sd)
    if B is None:
        return 0.0, 0.0, 0.0, 0.0
    Bm, Bs = B
    pb = 1.0 / Bs ** 2
    with np.errstate(all="ignore"):
        a, b = np.float64(rtau), np.float64(Bm) * np.float64(rpi)
        return (float(pb * np.float64(rpi)), float(pb * (a + b)), g(3) * abs(pb * rpi),
                float(g(5) * pb * (abs(a) + abs(b))))


def oracle_correct(mu, sg, dpi, dtau):
    """nat(rec') = nat(rec) + delta.  -> (mu', sigma', B_mu, B_sg), or None where the
    record is kept: NULL, a zero delta, or a delta that would void its precision."""
    if math.isnan(mu) or (dpi == 0.0 and dtau == 0.0):
        return None
    p0 = 1.0 / sg ** 2
    pi = p0 + dpi
    if not pi > 0.0:
        return None
    a = mu * p0
    num = a + dtau
    rp = (g(3) * p0 + g(1) * abs(pi)) / pi
    e_num = g(4) * abs(a) + g(1) * abs(num)
    q = num / pi
    Eq = (e_num + abs(num) * rp) / (pi * (1.0 - rp)) * (1 + U) + U * abs(q) if rp < 1.0 else INF
    s = 1.0 / math.sqrt(pi)
    return q, s, Eq, s * (amp(rp) / 2 * (1 + g(2)) + g(2))


# ------------------------------------------------------------------ wire formats
def round_wire(x, dtype):
    """fp32 array -> the wire type's bits (uint16), round to nearest even, written from
    the formats' definitions (fp16 by numpy's IEEE conversion)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def wire_value(bits, dtype):
    """uint16 wire bits -> fp32 values."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "fp16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def oracle_block_reduce(recv, N, dtype, want_prefix=True):
    """The owner reduce: recv [N * blk, 8] int32 words (7 words of two wire halves, the
    touch word) -> (total [blk, 8], exclusive prefixes [N * blk, 7] or None): an fp32 sum
    in rank order, rounded once to the wire type; the touch word summed as an integer."""
    recv = np.ascontiguousarray(recv, dtype=np.int32)
    blk = recv.shape[0] // N
    r = recv.reshape(N, blk, 8)
    halves = np.ascontiguousarray(r[..., :7]).view(np.uint16).reshape(N, blk, 14)
    acc = np.zeros((blk, 14), dtype=np.float32)
    pref = np.zeros((N, blk, 7), dtype=np.int32)
    with np.errstate(all="ignore"):
        for q in range(N):
            pref[q] = np.ascontiguousarray(round_wire(acc, dtype)).view(np.int32)
            acc = (acc + wire_value(halves[q], dtype)).astype(np.float32)
    total = np.zeros((blk, 8), dtype=np.int32)
    total[:, :7] = np.ascontiguousarray(round_wire(acc, dtype)).view(np.int32)
    total[:, 7] = r[..., 7].astype(np.int64).sum(0).astype(np.uint32).view(np.int32)
    return total, (pref.reshape(N * blk, 7) if want_prefix else None)


# ------------------------------------------------------------------ tables
def tr(row, t):
    """(mu, sigma) of track t of a [8, 2] row, None = NULL."""
    mu = float(row[t, 0])
    return None if math.isnan(mu) else (mu, float(row[t, 1]))


def make_roster(rows, attrs):
    """Roster.empty with (mu, sigma) [P, 8, 2] and attrs written directly."""
    P = rows.shape[0]
    ro = Roster.empty(P)
    st = ro.state.view(P, 8, 4)
    st[:, :, 0] = torch.from_numpy(rows[:, :, 0])
    st[:, :, 2] = torch.from_numpy(rows[:, :, 1])
    ro.attrs[:, :3] = torch.from_numpy(attrs[:, :3])
    return ro


def base_tensor(rows):
    """(mu, sigma) [P, 8, 2] -> base rows [P, 16]."""
    return torch.from_numpy(np.ascontiguousarray(rows.reshape(rows.shape[0], 16)))


def _null_rows(P):
    return np.full((P, 8, 2), np.nan, dtype=np.float32)


class Table:
    """Rows of a case table: start / prior / after (mu, sigma) [P, 8, 2], attrs [P, 4]."""

    def __init__(self, start, prior, after, attrs, labels):
        self.start, self.prior, self.after, self.attrs, self.labels = start, prior, after, attrs, labels
        self.P = start.shape[0]

    def take(self, idx):
        idx = np.asarray(idx)
        return Table(self.start[idx], self.prior[idx], self.after[idx], self.attrs[idx], [self.labels[i] for i in idx])


@functools.lru_cache(maxsize=None)
def grid_table():
    """The per-track grid: every track position x start {NULL, set} x start shared value
    {NULL, set} x seed {none, rank points, tier} x prior {equals start, moved, NULL} x after
    {unchanged, moved, NULL -> rated} x five start sigmas, mu and the other sigmas cycling
    (never a track set in the prior and NULL after)."""
    rows = []
    k = 0
    for t in range(TRACKS):
        for start_set in (False, True):
            for shared_set in ((False, True) if t > 0 else (start_set,)):
                for sd in SEEDS:
                    for prior_kind in (("equal", "moved") if start_set else ("null", "moved")):
                        for after_kind in (("unchanged", "moved") if prior_kind != "null" else ("unchanged", "rated")):
                            for i in range(len(SIGMAS)):
                                val = lambda dm, ds: (f32(MUS[(k + dm) % 4]), f32(SIGMAS[(i + ds) % 5]))  # noqa: E731
                                c = val(0, 0) if start_set else None
                                c0 = val(1, 2) if shared_set else None
                                a = c if prior_kind in ("equal", "null") else val(2, 1)
                                b = a if after_kind == "unchanged" else val(3, 3)
                                rows.append((t, c, c0 if t > 0 else c, a, b, sd,
                                             dict(t=t, start=start_set, shared=shared_set, seed=sd, prior=prior_kind,
                                                  after=after_kind, sigma=SIGMAS[i])))
                                k += 1
    P = len(rows)
    start, prior, after = _null_rows(P), _null_rows(P), _null_rows(P)
    attrs = np.zeros((P, 4), dtype=np.float32)
    for p, (t, c, c0, a, b, sd, _) in enumerate(rows):
        attrs[p, :3] = SEEDS[sd]
        if t > 0 and c0 is not None:
            start[p, 0] = prior[p, 0] = after[p, 0] = c0
        for arr, v in ((start, c), (prior, a), (after, b)):
            if v is not None:
                arr[p, t] = v
    return Table(start, prior, after, attrs, [r[6] for r in rows])


@functools.lru_cache(maxsize=None)
def tiled_grid():
    """The grid followed by a seeded permutation of it: every case in two lane groups and
    blocks, a few thousand players."""
    gtab = grid_table()
    perm = np.random.default_rng(5).permutation(gtab.P)
    return gtab.take(np.concatenate([np.arange(gtab.P), perm])), perm


@functools.lru_cache(maxsize=None)
def grid_messages(scaled, which="after"):
    """Oracle messages of the grid: msg [P, 7, 2], budgets [P, 7, 2], touch (lo, hi) [P, 2].
    ``which`` = "prior": the message start -> prior (the earlier ranks' exclusive prefix);
    "first": start -> after (a first sweep: the prior is the start)."""
    gtab = grid_table()
    msg, bud = np.zeros((gtab.P, 7, 2)), np.zeros((gtab.P, 7, 2))
    touch = np.zeros((gtab.P, 2), dtype=np.int64)
    for p in range(gtab.P):
        sd = seed_of(gtab.attrs[p])
        c0 = tr(gtab.start[p], 0)
        for t in range(TRACKS):
            c = tr(gtab.start[p], t)
            a = c if which in ("prior", "first") else tr(gtab.prior[p], t)
            b = tr(gtab.prior[p], t) if which == "prior" else tr(gtab.after[p], t)
            dp, dt, touched, bp, bt = oracle_message(t, c, c0, a, b, sd, scaled)
            msg[p, t], bud[p, t] = (dp, dt), (bp, bt)
            if touched:
                touch[p, 0 if t < 4 else 1] += 1 << (4 * (t & 3))
    return msg, bud, touch


class DecodeTable:
    """Summed messages to decode: start [P, 8, 2], attrs [P, 4], scaled and raw messages
    [P, 7, 2] (fp32), contributing ranks m [P, 7], labels."""

    def __init__(self):
        self.rows = []

    def add(self, label, attr=SEEDS["none"], **tracks):
        """tracks: t<k> = (start or None, S, r_tau, m[, raw (d_pi, d_tau)]): the scaled
        message, the raw one derived from it unless given."""
        self.rows.append((label, attr, {int(k[1:]): v for k, v in tracks.items()}))

    def build(self):
        P = len(self.rows)
        self.P = P
        self.start, self.attrs = _null_rows(P), np.zeros((P, 4), dtype=np.float32)
        self.scaled, self.raw = np.zeros((P, 7, 2), dtype=np.float32), np.zeros((P, 7, 2), dtype=np.float32)
        self.m = np.zeros((P, 7), dtype=np.int64)
        self.labels = [r[0] for r in self.rows]
        with np.errstate(all="ignore"):
            for p, (_, attr, tracks) in enumerate(self.rows):
                self.attrs[p, :3] = attr
                for t, v in tracks.items():
                    if v[0] is not None:
                        self.start[p, t] = v[0]
                sd, c0 = seed_of(self.attrs[p]), tr(self.start[p], 0)
                for t, v in tracks.items():
                    S, rtau, self.m[p, t] = np.float32(v[1]), np.float32(v[2]), v[3]
                    self.scaled[p, t] = (S, rtau)
                    B = base_of(t, tr(self.start[p], t), c0, sd)
                    if len(v) > 4:
                        self.raw[p, t] = v[4]
                    elif B is not None:
                        pb = 1.0 / B[1] ** 2
                        self.raw[p, t] = (pb * np.float64(S), pb * (np.float64(rtau) + B[0] * np.float64(S)))
        return self

    def touch(self):
        lo = sum(self.m[:, t] << (4 * t) for t in range(4))
        hi = sum(self.m[:, t] << (4 * (t - 4)) for t in range(4, 7))
        return lo, hi

    def buf(self, scaled):
        """[P, 16] fp32 decode input: messages + the touch fields."""
        lo, hi = self.touch()
        msg = self.scaled if scaled else self.raw
        return torch.from_numpy(np.concatenate([msg.reshape(self.P, 14), lo[:, None].astype(np.float32),
                                                hi[:, None].astype(np.float32)], axis=1))

    def cnt(self):
        lo, hi = self.touch()
        return torch.from_numpy((lo | (hi << 16)).astype(np.int32)[:, None].copy())


def _base_values(i, k, null):
    c = (f32(MUS[k % 4]), f32(SIGMAS[i % 5]))
    return (None, c) if null else (c, (f32(MUS[(k + 1) % 4]), f32(SIGMAS[(i + 2) % 5])))


@functools.lru_cache(maxsize=None)
def decode_table():
    """Summed messages: m in {1, 2, 8, 15} ranks x {equal losses, unequal losses, net
    gain} (m = 1: a loss of one rank) on every track and base sigma, set and NULL starts;
    all seven tracks touched by 15 ranks; both clamp floors a factor >= 2 either side;
    non-finite halves on tracks 0, 2 and 6."""
    T = DecodeTable()
    k = 0
    for t in range(TRACKS):
        for m in (1, 2, 8, 15):
            for kind in ("equal", "unequal", "gain"):
                for i in range(len(SIGMAS)):
                    null = (k % 3 == 2)
                    c, c0 = _base_values(i, k, null)
                    xs = {"equal": [0.8] * m, "unequal": [0.7 if r % 2 else 0.95 for r in range(m)],
                          "gain": [1.3] * m}[kind]
                    S = sum(x - 1.0 for x in xs)
                    rtau = sum(x * (12.5 + 3 * r) for r, x in enumerate(xs))
                    tracks = {"t%d" % t: (c, S, rtau, m)}
                    if t > 0:  # (half of the NULL mode tracks: no shared value either, based on the seed)
                        tracks["t0"] = (None if null and k % 6 == 5 else c0, 0.0, 0.0, 0)
                    T.add(dict(kind=kind, t=t, m=m, sigma=SIGMAS[i % 5], null=null),
                          SEEDS["tier" if k % 2 else "points"], **tracks)
                    k += 1
    # all seven tracks touched by all 15 ranks: lo = 0xFFFF, hi = 0xFFF, m = 15 on the variance branch
    for null in (False, True):
        for i in range(len(SIGMAS)):
            tracks = {}
            for t in range(TRACKS):
                c = None if null else (f32(MUS[(t + i) % 4]), f32(SIGMAS[(t + i) % 5]))
                tracks["t%d" % t] = (c, -15 * (0.02 + 0.01 * t), 15 * (4.0 + t), 15)
            T.add(dict(kind="all15", null=null, i=i), SEEDS["tier"], **tracks)
    # the scaled floor 1e-6, a factor 2 (or more) either side, natural sum and variance space
    for t in (0, 2, 6):
        c = (1500.0, 100.0)
        sh = {"t0": ((1400.0, 200.0), 0.0, 0.0, 0)} if t else {}
        zero = (0.0, 0.0)
        for label, S, m in (("nat above", -1 + 2e-6, 1), ("nat below", -1 + 5e-7, 1), ("nat negative", -1.25, 1),
                            ("var above", 2 * (8e-6 - 1), 2), ("var below", 2 * (1e-6 - 1), 2),
                            ("x <= 0", -2.5, 2), ("15 ranks below", -15.0, 15)):
            T.add(dict(kind="floor scaled", what=label, t=t), **dict(sh, **{"t%d" % t: (c, S, 1e-5, m, zero)}))
        # the raw floor 1e-12: sigma_B = 2000, pi_B = 2.5e-7 (an fp32 rounding of it is 3e-14)
        c = (1500.0, 2000.0)
        pb = 1.0 / 2000.0 ** 2
        for label, pi in (("raw above", 2e-12), ("raw below", 5e-13), ("raw negative", -pb)):
            T.add(dict(kind="floor raw", what=label, t=t),
                  **dict(sh, **{"t%d" % t: (c, 0.0, 0.0, 1, (pi - pb, 1500.0 * (pi - pb)))}))
    # non-finite halves (in fp32 and on the wire): left at the start, counted
    for t in (0, 2, 6):
        for null in (False, True):
            c = None if null else (1500.0, 100.0)
            sh = {"t0": ((1400.0, 200.0), 0.0, 0.0, 0)} if t else {}
            for label, S, rtau in (("+inf r_pi", INF, 3.0), ("-inf r_pi", -INF, 3.0), ("+inf r_tau", 0.25, INF),
                                   ("-inf r_tau", -0.25, -INF), ("nan r_pi", NAN, 3.0), ("nan r_tau", 0.5, NAN)):
                T.add(dict(kind="nonfinite", what=label, t=t, null=null), SEEDS["points"],
                      **dict(sh, **{"t%d" % t: (c, S, rtau, 2, (S, rtau))}))
    return T.build()


def decode_oracle(T, msg, scaled):
    """Oracle of the decode of table T with messages msg [P, 7, 2] (fp32 values, as the
    decode receives them).  -> dict(out [P, 8, 2], B [P, 7, 2], branch [P][7], clamps)."""
    out = np.array(T.start, dtype=np.float64)
    B = np.zeros((T.P, 7, 2))
    branch = [[None] * 7 for _ in range(T.P)]
    clamps = 0
    for p in range(T.P):
        sd, c0 = seed_of(T.attrs[p]), tr(T.start[p], 0)
        for t in range(TRACKS):
            r = oracle_decode(t, tr(T.start[p], t), c0, sd, float(msg[p, t, 0]), float(msg[p, t, 1]),
                              int(T.m[p, t]), scaled)
            branch[p][t] = r["branch"]
            clamps += r["clamp"]
            if r["out"] is not None and r["branch"] in ("nat", "var", "clamp"):
                out[p, t] = r["out"]
                B[p, t] = (r["B_mu"], r["B_sg"])
    return dict(out=out, B=B, branch=branch, clamps=clamps)


# ------------------------------------------------------------------ comparisons
def ratios(got, exp, bud):
    """|got - exp| / budget per element; where the oracle is exact (budget 0), NULL or not
    finite the value itself must match (ratio 0 or inf)."""
    got, exp, bud = (np.asarray(x, dtype=np.float64) for x in (got, exp, bud))
    with np.errstate(all="ignore"):
        err = np.abs(got - exp)
        same = (got == exp) | (np.isnan(got) & np.isnan(exp))
        r = np.where(same, 0.0, np.where(np.isfinite(exp) & (bud > 0), err / bud, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def assert_budget(got, exp, bud, what, labels=None):
    """Every element within its budget (ratio <= 1, no margin); returns the worst ratio."""
    r = ratios(got, exp, bud)
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    worst = float(r[at])
    print("%s worst |error| / budget: %.4f" % (what, worst))
    assert worst <= 1.0, "%s outside the merge budget: ratio %.4g at %s (%s): got %r, oracle %r, budget %r" % (
        what, worst, at, labels[at[0]] if labels else "", np.asarray(got)[at], np.asarray(exp)[at], np.asarray(bud)[at])
    return worst


# ------------------------------------------------------------------ fp32 transcription
F = np.float32
MUTATIONS = ("null_base_seed", "mdiv_ratio", "neighbour_nibble", "r0_for_r1", "prefix_no_mu_term", "record_track")


def t_base(t, c, c0, sd, mut=None):
    if c is not None:
        return c
    if t > 0 and c0 is not None and mut != "null_base_seed":
        return c0
    return sd


def t_message(t, c, c0, a, b, sd, scaled, mut=None):
    had = a is not None
    changed = (b != a) if had else (b is not None)
    B = t_base(t, c, c0, sd, mut)
    if not changed or B is None:
        return F(0), F(0), changed
    bm, bs = F(B[0]), F(B[1])
    bmu, bsg = F(b[0]), F(b[1])
    if scaled:
        r1 = bs / bsg
        r0 = bs / F(a[1]) if had else F(1)
        dp = r1 * r1 - r0 * r0
        lead = r0 if mut == "r0_for_r1" else r1
        dt = lead * lead * (bmu - bm) - (r0 * r0 * (F(a[0]) - bm) if had else F(0))
        return dp, dt, True
    p1 = F(1) / (bsg * bsg)
    pm, ps = (F(a[0]), F(a[1])) if had else (bm, bs)
    p0 = F(1) / (ps * ps)
    return p1 - p0, bmu * p1 - pm * p0, True


def t_decode(t, c, c0, sd, dpi, dtau, m, scaled, mut=None):
    """-> ((mu, sigma) or None, clamped)"""
    dpi, dtau = F(dpi), F(dtau)
    if not (np.isfinite(dpi) and np.isfinite(dtau)):
        return c, True
    live = (dpi != 0 or dtau != 0) if c is not None else m != 0
    B = t_base(t, c, c0, sd, mut)
    if not live or B is None:
        return c, False
    bm, bs = F(B[0]), F(B[1])
    one = F(1)

    def merged(S):
        ratio = one + S
        if S < 0 and m >= 2:
            x = one + S / F(m)
            if x > 0:
                ratio = x / (x + F(m) * (one - x))
                return ratio, (ratio if mut == "mdiv_ratio" else x), True
        return ratio, ratio, False

    with np.errstate(all="ignore"):
        if scaled:
            ratio, mdiv, _ = merged(dpi)
            clamped = not ratio > F(1e-6)
            if clamped:
                ratio = mdiv = F(1e-6)
            return (float(bm + dtau / mdiv), float(bs / np.sqrt(ratio))), clamped
        pb = one / (bs * bs)
        tb = bm * pb
        S = dpi / pb
        ratio, mdiv, var = merged(S)
        if var:
            return (float(bm + (dtau / pb - S * bm) / mdiv), float(bs / np.sqrt(ratio))), False
        pi = pb + dpi
        clamped = not pi > F(1e-12)
        if clamped:
            pi = F(1e-12)
        return (float((tb + dtau) / pi), float(one / np.sqrt(pi))), clamped


def t_touch_count(lo, hi, t, mut=None):
    """m of track t from the touch fields."""
    if mut == "neighbour_nibble":
        t = t + 1 if t < 6 else 5
    return (lo >> (4 * t)) & 15 if t < 4 else (hi >> (4 * (t - 4))) & 15


def t_prefix_delta(t, c, c0, sd, rpi, rtau, mut=None):
    rpi, rtau = F(rpi), F(rtau)
    B = t_base(t, c, c0, sd, mut)
    if (rpi == 0 and rtau == 0) or B is None:
        return F(0), F(0)
    bm, bs = F(B[0]), F(B[1])
    pb = F(1) / (bs * bs)
    with np.errstate(all="ignore"):
        return pb * rpi, pb * (rtau if mut == "prefix_no_mu_term" else rtau + bm * rpi)


def t_correct(mu, sg, dpi, dtau):
    mu, sg, dpi, dtau = F(mu), F(sg), F(dpi), F(dtau)
    if np.isnan(mu) or (dpi == 0 and dtau == 0):
        return mu, sg
    p0 = F(1) / (sg * sg)
    pi = p0 + dpi
    if not pi > 0:
        return mu, sg
    return (mu * p0 + dtau) / pi, F(1) / np.sqrt(pi)


# ------------------------------------------------------------------ record correction
STATUS_CYCLE = (0, 0, 0, 1, 0, 0, 2, 0, 0, 0, 3, 0)   # rated next to AFK, invalid and unsupported rows
REC_PLAYERS = 48


def corr_tile(K):
    """Matches per block of the correction kernel: 256, halved while the LDS tile of
    padded rows exceeds 64 KiB (K = 4, 5: 64-float rows)."""
    W = -(-(5 * 2 * K + 2) // 32) * 32
    T = 256
    while T > 64 and T * (W + 1) * 4 > 64 * 1024:
        T //= 2
    return T, W


@functools.lru_cache(maxsize=None)
def record_case(K):
    """(rec [M, 2K+2] int32, rows [M, W] fp32, delta [P, 16] fp32) with M = 2T + 37: every
    player has its own record sigmas, so its delta row is designed against them --
    player 0: a zero delta; 1: d_pi = -p0 exactly (sigma 64: p0 = 2^-12 in every
    precision); 2: twice that; 3: NULL mode records; the rest gains and losses up to
    0.9 p0, different on every track."""
    T, W = corr_tile(K)
    S, M, P = 2 * K, 2 * T + 37, REC_PLAYERS
    rng = np.random.default_rng(100 + K)
    sg_s = np.array([f32(SIGMAS[p % 5] * (1 + p / 64)) for p in range(P)], dtype=np.float32)
    sg_m = np.array([f32(SIGMAS[(p + 2) % 5] * (1 + p / 96)) for p in range(P)], dtype=np.float32)
    sg_s[1:3] = sg_m[1:3] = 64.0
    delta = np.zeros((P, 16), dtype=np.float32)
    for p in range(1, P):
        for t in range(TRACKS):
            p0 = 1.0 / float(sg_s[p] if t == 0 else sg_m[p]) ** 2
            frac = -1.0 if p == 1 else -2.0 if p == 2 else rng.uniform(-0.9, 3.0) * (1 + t / 10) / 1.6
            delta[p, 2 * t] = p0 * frac
            delta[p, 2 * t + 1] = p0 * rng.uniform(-4000, 4000)
    delta[4, 0:2] = 0.0  # a zero shared delta beside live mode deltas
    rows = rng.uniform(-3.0, 3.0, (M, W)).astype(np.float32)
    rec = np.full((M, S + 2), -1, dtype=np.int32)
    words = rows.view(np.int32)
    for i in range(M):
        st = STATUS_CYCLE[i % len(STATUS_CYCLE)]
        mode = 7 if st == 3 else i % 6
        n0 = K if i % 5 else max(K - 1, 1)
        n1 = K if i % 7 else max(K - 2, 1)
        for j in range(S):
            inr = (j < n0) if j < K else (j - K < n1)
            p = int(rng.integers(0, P))
            if i % 11 == 3 and j == S - 1:
                p = P + int(rng.integers(0, 3))   # an id past the delta table
            rec[i, j] = p if inr else -1
            q = min(p, P - 1)
            if inr:
                rows[i, j], rows[i, S + j] = f32(1500 + 37 * q - 3 * j), sg_s[q]
                rows[i, 3 * S + j], rows[i, 4 * S + j] = f32(900 + 41 * q + 5 * j), sg_m[q]
                if q == 3 or (i + j) % 13 == 0:
                    rows[i, 3 * S + j] = rows[i, 4 * S + j] = np.nan  # no mode rating recorded
            else:
                for f in (0, 1, 2, 3, 4):
                    rows[i, f * S + j] = np.nan
        rec[i, S] = mode | (n0 << 8) | (n1 << 16) | (2 << 24)
        rec[i, S + 1] = 1 | (4 if st == 1 else 0)
        words[i, 5 * S + 1] = st | (0x5A17C3 << 8 if i % 3 == 0 else 0)   # the status byte; the rest is not ours
    return rec, rows, delta


@functools.lru_cache(maxsize=None)
def record_oracle(K):
    """(expected rows fp64 [M, W], budgets [M, W] (0: bit-identical to the input))."""
    rec, rows, delta = record_case(K)
    S, P = 2 * K, delta.shape[0]
    exp, bud = rows.astype(np.float64), np.zeros(rows.shape)
    words = rows.view(np.int32)
    for i in range(rows.shape[0]):
        if words[i, 5 * S + 1] & 0xFF != 0:
            continue
        meta = int(rec[i, S])
        t, n0, n1 = 1 + (meta & 0xFF), (meta >> 8) & 0xFF, (meta >> 16) & 0xFF
        for j in range(S):
            p = int(rec[i, j])
            if not ((j < n0) if j < K else (j - K < n1)) or p < 0 or p >= P:
                continue
            for mu_at, sg_at, tt in ((j, S + j, 0), (3 * S + j, 4 * S + j, t)):
                r = oracle_correct(float(rows[i, mu_at]), float(rows[i, sg_at]), float(delta[p, 2 * tt]),
                                   float(delta[p, 2 * tt + 1]))
                if r is not None:
                    exp[i, mu_at], exp[i, sg_at], bud[i, mu_at], bud[i, sg_at] = r
    return exp, bud


def record_sizes(K):
    T = corr_tile(K)[0]
    return (1, T - 1, T, T + 1, 2 * T + 37)


def check_records(got, K, M, what):
    """``got`` [M, W] fp32 corrected rows of the first M matches: the corrected (mu, sigma)
    within budget, everything else the input's bits.  Returns the worst ratio."""
    rec, rows, _ = record_case(K)
    exp, bud = record_oracle(K)
    got = np.ascontiguousarray(got)
    keep = bud[:M] == 0
    assert np.array_equal(got.view(np.int32)[keep], rows[:M].view(np.int32)[keep]), \
        "%s: a field the correction must not touch changed" % what
    assert int((~keep).sum()) > 0 or M < 3
    return assert_budget(got[~keep], exp[:M][~keep], bud[:M][~keep], what)


# ------------------------------------------------------------------ block reduce
def block_reduce_case(N, blk, dtype):
    """recv [N * blk, 8] int32: halves whose fp32 sums land on round-to-even ties of the
    wire type (both parities), wide-range halves whose fp32 sum depends on the order, and
    touch words with every nibble counted by every rank."""
    rng = np.random.default_rng(N * 1000 + blk)
    ulp = 2.0 ** -10 if dtype == "fp16" else 2.0 ** -7     # spacing in [1, 2)
    h = np.zeros((N, blk, 14), dtype=np.float32)
    for r in range(blk):
        for col in range(14):
            kind = (r + col) % 4
            if kind == 0:      # 1 + k ulp, + half an ulp from the last rank: a tie, k even and odd
                h[0, r, col] = (1 + ((r + col) // 4 % 8) * ulp) * 2.0 ** (col - 6)
                h[N - 1, r, col] += (ulp / 2) * 2.0 ** (col - 6)
            elif kind == 1:    # a negative tie, with a pair of ranks in between that cancels
                h[0, r, col] = -(1 + (r % 4) * ulp) * 8
                h[N - 1, r, col] += -(ulp / 2) * 8
                if N >= 4:
                    h[1, r, col], h[N - 2, r, col] = 0.75, -0.75
            elif kind == 2:    # wide range: the order of the fp32 sum shows
                h[:, r, col] = rng.choice([40000.0, -40000.0, 3.0e-4, 1.0, -0.33], N)
            else:
                h[:, r, col] = rng.normal(0, 40, N)
    bits = np.stack([round_wire(h[q], dtype) for q in range(N)])          # [N, blk, 14] uint16
    recv = np.zeros((N, blk, 8), dtype=np.int32)
    recv[..., :7] = np.ascontiguousarray(bits).view(np.int32).reshape(N, blk, 7)
    recv[..., 7] = 0x01111111 if N == 15 else rng.integers(0, 0x01111111, (N, blk))
    return recv.reshape(N * blk, 8)
