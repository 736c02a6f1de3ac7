"""Shared cases of the single-match numerics tests (test_single_match.py, CPU and
``-m gpu``): hand-built windows of independent matches, a 50-digit mpmath oracle of the
two-team closed form, and the per-element error budget the executor's math
(csrc/rate_dev.h ``rate_pair`` / ``vw_pair``) has to meet.

The oracle is written here from the model's formulas alone (it imports nothing from
``analyzer_amd.models``); test_single_match.py ties it to the factor graph.  The budget
is derived in docs/ARCHITECTURE.md ("Single-match error budget"), not fitted: a test
that misses it points at a wrong term in the kernel or in the derivation."""
import functools
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import pytest
import torch

from analyzer_amd.config import RaterConfig
from analyzer_amd.ops.rate import RATED, Roster

BETA = float(RaterConfig().beta)  # 1000
TAU = float(RaterConfig().tau)    # 10
U = 2.0 ** -24                    # fp32 unit roundoff
Q_FLOOR = 1.1e-19                 # sqrt(FLT_MIN): the kernel's q = sqrt(exp(..)) underflows below it

OUTCOMES = ("win0", "win1", "tie")
SURPLUS = (0, 1, 300, 1500, 3000, 6000, 12000, 30000, 60000)
SIGMA_PATTERNS = ("all1", "all30", "all166.667", "all500", "all2000", "one2000", "mix")
SIGMA_VALUES = (1.0, 30.0, 166.667, 500.0, 2000.0)
MODE_KINDS = ("null", "offset", "minus3000")
FIELDS = ("s_mu", "s_sig", "delta", "m_mu", "m_sig")


def f32(x):
    return float(np.float32(x))


def eps_vw(t, tie):
    """Relative error bound of v and w documented in the rate_dev.h header."""
    if tie:
        return 0.0
    return 8.4e-7 if t < 4 else 2.4e-6 if t < 6 else 9e-6


@dataclass
class Case:
    """One match.  Per-slot lists have 2K entries (team 0 then team 1); ``None`` is NULL.
    ``players``: local player number per slot (equal numbers = one player in several
    slots); ``same_as``: take the players of that earlier case of the window instead of
    fresh ones (their state is not written again); ``fresh`` overrides single slots of such
    a case with players from the end of the roster."""
    K: int
    mu: List[Optional[float]]
    sig: List[Optional[float]]
    mmu: List[Optional[float]]
    msig: List[Optional[float]]
    n1: int
    outcome: str = "win0"
    mode: int = 0
    tie_bits: int = 0
    n0: Optional[int] = None
    attrs: Optional[dict] = None        # slot -> (ranked, blitz, tier), None = NULL
    players: Optional[List[int]] = None
    same_as: Optional[int] = None
    fresh: Optional[dict] = None        # slot -> a player of the window's ``extra_players`` (state written)
    seed: Optional[dict] = None         # slot -> (mu, sigma): the seeded shared prior the oracle takes
    label: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.n0 is None:
            self.n0 = self.K
        if self.players is None:
            self.players = list(range(2 * self.K))

    def slots(self):
        K = self.K
        return [j for j in range(2 * K) if (j < self.n0 if j < K else j - K < self.n1)]

    def winners(self):
        if self.outcome == "tie":
            return self.tie_bits, self.tie_bits
        return (1, 0) if self.outcome == "win0" else (0, 1)


# ------------------------------------------------------------------ window builder
def player_of(case, base, j):
    return int(case.fresh[j]) if case.fresh and j in case.fresh else int(base) + case.players[j]


def build_window(cases, extra_players=0):
    """(roster, rec [M, 2K+2], base [M]): every case gets 2K players of its own
    (``same_as`` cases the players of the case they name)."""
    K = cases[0].K
    S = 2 * K
    M = len(cases)
    roster = Roster.empty(M * S + extra_players)
    st, at = roster.state, roster.attrs
    rec = torch.full((M, S + 2), -1, dtype=torch.int32)
    base = np.zeros(M, dtype=np.int64)
    nan = float("nan")
    for i, c in enumerate(cases):
        assert c.K == K
        base[i] = i * S if c.same_as is None else base[c.same_as]
        for j in c.slots():
            p = player_of(c, base[i], j)
            rec[i, j] = p
            own = c.fresh is not None and j in c.fresh
            if not own and (c.same_as is not None or c.players.index(c.players[j]) != j):
                continue
            if c.mu[j] is not None:
                st[p, 0], st[p, 2] = c.mu[j], c.sig[j]
            if c.mmu[j] is not None:
                st[p, 4 * (1 + c.mode)], st[p, 4 * (1 + c.mode) + 2] = c.mmu[j], c.msig[j]
            if c.attrs and j in c.attrs:
                at[p, 0:3] = torch.tensor([nan if a is None else a for a in c.attrs[j]], dtype=torch.float32)
        w0, w1 = c.winners()
        rec[i, S] = c.mode | (c.n0 << 8) | (c.n1 << 16) | (2 << 24)
        rec[i, S + 1] = w0 | (w1 << 1)
    return roster, rec, base


# ------------------------------------------------------------------ the oracle
def _mp():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    return mp


def priors(case):
    """Per in-roster slot the fp32-rounded priors ((mu, sigma) shared, (mu, sigma) mode,
    had a stored shared rating) after seeding and the mode track's fall-back."""
    out = {}
    for j in case.slots():
        j0 = case.players.index(case.players[j])  # a repeated player rates from its first slot's state
        had = case.mu[j0] is not None
        ms, ss = (case.mu[j0], case.sig[j0]) if had else case.seed[j0]
        mm, sm = (case.mmu[j0], case.msig[j0]) if case.mmu[j0] is not None else (ms, ss)
        out[j] = (f32(ms), f32(ss), f32(mm), f32(sm), had)
    return out


def _track(mp, case, mu, sig, tau):
    """One track of one match at 50 digits: per slot (mu', sigma', B_mu, B_sig relative),
    and (d, delta_d, t)."""
    slots = case.slots()
    n = len(slots)
    K = case.K
    s2 = {j: sig[j] ** 2 + tau ** 2 for j in slots}
    c2 = n * mp.mpf(BETA) ** 2 + sum(s2.values())
    c = mp.sqrt(c2)
    d = sum(mu[j] if j < K else -mu[j] for j in slots)
    dd = 2 * n * U * sum(abs(mu[j]) for j in slots)  # fp32 rounding of the team sums
    tie = case.outcome == "tie"
    if tie:
        sgn, t = 1, d / c
        v, w = -d / c, mp.mpf(1)
    else:
        sgn = 1 if case.outcome == "win0" else -1
        t = sgn * d / c
        v = mp.npdf(t) / mp.ncdf(t)
        w = v * (v + t)
    eps = eps_vw(float(t), tie)
    out = {}
    for j in slots:
        side = sgn if j < K else -sgn
        nm = mu[j] + side * s2[j] * v / c
        y = s2[j] * w / c2
        ns = mp.sqrt(s2[j] * (1 - y))
        b_mu = (s2[j] / c) * (abs(v) * (eps + 8 * U) + w * dd / c) + 4 * U * abs(nm)
        b_sig = y / (1 - y) * (eps + 8 * U) / 2 + 4 * U
        out[j] = (nm, ns, b_mu, b_sig)
    return out, d, dd, t


def shared_track_mp(case):
    """{slot: (mu', sigma')} of the shared track as 50-digit ``mpf`` (for comparisons
    tighter than fp64)."""
    mp = _mp()
    pr = priors(case)
    mu = {j: mp.mpf(pr[j][0]) for j in case.slots()}
    sig = {j: mp.mpf(pr[j][1]) for j in case.slots()}
    return {j: r[:2] for j, r in _track(mp, case, mu, sig, mp.mpf(TAU))[0].items()}


def oracle(cases):
    """Expected outputs and their budgets, float64 [M, 2K] per field of ``FIELDS``
    (NaN on empty slots), ``quality`` [M], ``t`` [M, 2] (shared, mode) and
    ``B_<field>`` / ``B_quality`` of the same shapes.  ``B_s_sig`` / ``B_m_sig`` are
    absolute (the relative bound times sigma')."""
    mp = _mp()
    M, S = len(cases), 2 * cases[0].K
    o = {k: np.full((M, S), np.nan) for k in FIELDS}
    o.update({"B_" + k: np.full((M, S), np.nan) for k in FIELDS})
    o["quality"], o["B_quality"], o["t"] = np.zeros(M), np.zeros(M), np.zeros((M, 2))
    for i, c in enumerate(cases):
        pr = priors(c)
        slots = c.slots()
        smu = {j: mp.mpf(pr[j][0]) for j in slots}
        ssg = {j: mp.mpf(pr[j][1]) for j in slots}
        mmu = {j: mp.mpf(pr[j][2]) for j in slots}
        msg = {j: mp.mpf(pr[j][3]) for j in slots}
        sh, _, _, ts = _track(mp, c, smu, ssg, mp.mpf(TAU))
        md, d, dd, tm = _track(mp, c, mmu, msg, mp.mpf(TAU))
        o["t"][i] = float(ts), float(tm)
        # quality: the mode track, sigma without tau
        nb2 = len(slots) * mp.mpf(BETA) ** 2
        den = nb2 + sum(msg[j] ** 2 for j in slots)
        a = d * d / (2 * den)
        q = mp.sqrt(nb2 / den) * mp.exp(-a)
        o["quality"][i] = float(q)
        o["B_quality"][i] = float(q * (8 * U * (1 + a) + abs(d) * dd / den)) + Q_FLOOR
        for j in slots:
            nm, ns, b_mu, b_sig = sh[j]
            o["s_mu"][i, j], o["s_sig"][i, j] = float(nm), float(ns)
            o["B_s_mu"][i, j], o["B_s_sig"][i, j] = float(b_mu), float(b_sig * ns)
            o["m_mu"][i, j], o["m_sig"][i, j] = float(md[j][0]), float(md[j][1])
            o["B_m_mu"][i, j], o["B_m_sig"][i, j] = float(md[j][2]), float(md[j][3] * md[j][1])
            prev = [k for k in slots if k < j and c.players[k] == c.players[j]]
            if prev:
                # a player's later slot: against the posterior its earlier slot wrote
                pm_, ps_, pb_mu, pb_sig = sh[prev[-1]]
                o["delta"][i, j] = float((nm - ns) - (pm_ - ps_))
                o["B_delta"][i, j] = float(b_mu + b_sig * ns + pb_mu + pb_sig * ps_ + 4 * U * (abs(nm) + abs(pm_)))
            elif pr[j][4]:
                o["delta"][i, j] = float((nm - ns) - (smu[j] - ssg[j]))
                o["B_delta"][i, j] = float(b_mu + b_sig * ns + 4 * U * (abs(nm) + abs(smu[j])))
            else:
                o["delta"][i, j], o["B_delta"][i, j] = 0.0, 0.0
    return o


# ------------------------------------------------------------------ comparisons
def worst_ratios(got, orc, rows=None):
    """{field: (|got - oracle| / budget at its worst element, (row, slot))}; ``got`` maps
    field -> array over the same matches as the oracle (``rows`` selects oracle rows)."""
    out = {}
    for k in FIELDS + ("quality",):
        exp, bud = orc[k], orc["B_" + k]
        if rows is not None:
            exp, bud = exp[rows], bud[rows]
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == exp.shape, (k, g.shape, exp.shape)
        assert np.array_equal(np.isnan(g), np.isnan(exp)), "%s: NaN pattern differs from the oracle's" % k
        err = np.abs(g - exp)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bud)
        ratio = np.where(np.isnan(exp), 0.0, ratio)
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        out[k] = (float(ratio[at]), tuple(int(x) for x in at))
    return out


def result_fields(res):
    d = {k: getattr(res, k).cpu().numpy() for k in FIELDS}
    d["quality"] = res.quality.cpu().numpy()
    return d


def describe(cases, orc, at, rows=None):
    i = at[0] if rows is None else int(np.asarray(rows)[at[0]])
    return dict(cases[i].label, match=i, slot=(at[1] if len(at) > 1 else None),
                t_shared=round(float(orc["t"][i, 0]), 3), t_mode=round(float(orc["t"][i, 1]), 3))


def assert_within_budget(got, orc, cases, rows=None, what=""):
    """Every element within its budget; on failure the worst ratio per field with its
    case.  Returns the worst ratios {field: ratio}."""
    worst = worst_ratios(got, orc, rows)
    print("%s worst |error| / budget: %s" % (what, {k: round(v[0], 4) for k, v in worst.items()}))
    bad = {k: (r, describe(cases, orc, at, rows)) for k, (r, at) in worst.items() if not r <= 1.0}
    assert not bad, "%s outside the single-match budget: %s" % (what, bad)
    return {k: v[0] for k, v in worst.items()}


def roster_fields(roster, cases, base):
    """The stored (mu, sigma) of the shared and the played mode track of every slot's
    player, laid out like the record fields ([M, 2K], NaN on empty slots)."""
    st = roster.state.cpu().numpy()
    M, S = len(cases), 2 * cases[0].K
    out = {k: np.full((M, S), np.nan, dtype=np.float32) for k in ("s_mu", "s_sig", "m_mu", "m_sig")}
    for i, c in enumerate(cases):
        g = 4 * (1 + c.mode)
        for j in c.slots():
            p = player_of(c, base[i], j)
            out["s_mu"][i, j], out["s_sig"][i, j] = st[p, 0], st[p, 2]
            out["m_mu"][i, j], out["m_sig"][i, j] = st[p, g], st[p, g + 2]
    return out


def assert_rated(res):
    st = res.status.cpu().numpy()
    assert (st == RATED).all(), "statuses %s" % dict(zip(*np.unique(st, return_counts=True)))


# ------------------------------------------------------------------ the grid
def _sigmas(pattern, S, rng):
    if pattern == "one2000":
        return [2000.0] + [1.0] * (S - 1)
    if pattern == "mix":
        return [SIGMA_VALUES[k] for k in rng.integers(0, len(SIGMA_VALUES), S)]
    return [float(pattern[3:])] * S


@functools.lru_cache(maxsize=None)
def grid(K):
    """The single-match grid of team size K (docs/ARCHITECTURE.md): outcome x n1 x
    team-0 mu surplus x sigma pattern, the mode track's kind and the game mode cycling
    over the cases.  Shared by every test; never modified."""
    S = 2 * K
    rng = np.random.default_rng(1000 + K)
    cases = []
    for outcome in OUTCOMES:
        for n1 in ((K,) if K == 1 else (K, K - 1)):
            i = 0
            for surplus in SURPLUS:
                for pi, pattern in enumerate(SIGMA_PATTERNS):
                    mu = [f32(1500.0 + rng.uniform(-50, 50) + (surplus / K if j < K else 0.0)) for j in range(S)]
                    sig = [f32(s) for s in _sigmas(pattern, S, rng)]
                    kind = MODE_KINDS[i % 3]
                    off = rng.uniform(-150, 150, S)
                    nxt = _sigmas(SIGMA_PATTERNS[(pi + 1) % len(SIGMA_PATTERNS)], S, rng)
                    if kind == "null":
                        mmu, msig = [None] * S, [None] * S
                    elif kind == "offset":
                        mmu, msig = [f32(m + o) for m, o in zip(mu, off)], [f32(s) for s in nxt]
                    else:
                        mmu, msig = [f32(m - 3000.0) for m in mu], [500.0] * S
                    cases.append(Case(K, mu, sig, mmu, msig, n1, outcome, mode=i % 6, tie_bits=i & 1,
                                      label=dict(K=K, n1=n1, surplus=surplus, sigma=pattern, outcome=outcome,
                                                 mode_track=kind)))
                    i += 1
    return cases


@functools.lru_cache(maxsize=None)
def grid_perm(K):
    n = len(grid(K))
    return np.random.default_rng(77 + K).permutation(n)


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    return oracle(grid(K))


def grid_window(K):
    """(roster, rec, base, cases): the grid followed by the same grid in a seeded
    permutation with fresh players, so every case lands in two lane groups and chunks.
    Rows [n + k] repeat case perm[k]."""
    g = grid(K)
    cases = list(g) + [g[k] for k in grid_perm(K)]
    roster, rec, base = build_window(cases)
    return roster, rec, base, cases


def both_copies(K):
    """Oracle rows of the window's matches: the grid, then the permuted copy."""
    n = len(grid(K))
    return np.concatenate([np.arange(n), grid_perm(K)])
