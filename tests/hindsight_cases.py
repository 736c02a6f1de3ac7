"""Shared cases of the hindsight tests (test_hindsight.py on the CPU, test_hindsight_gpu.py on
the device): the oracle, the error budget, the windows and the checks that run the same way on
either device.

The oracle is written from the definitions in the module docstring of ops/hindsight.py, not
from csrc/: ``elements`` decides in numpy which slots are elements, ``oracle`` walks every
chain backwards with 50-digit mpmath numbers.  The budget of an element is computed from the
length of its chain and its inputs by the formula of the issue,

    |mu_s - E|     <= ulp32(E) / 2 + c n 2^-53 max|mu_t|
    |sigma_s - E|  <= ulp32(E) / 2 + (c n / 2 + 1) 2^-53 E          c = 20

(the derivation of c is in csrc/hindsight_core.h), never from what the code returns.  Both the
host mirror and the kernels are held to it against the oracle; where the oracle would take
too long (540,000 elements) the kernels are held to twice it against the mirror and both to
it on sampled players."""
import dataclasses
import functools
from fractions import Fraction

import mpmath
import numpy as np
import torch

from analyzer_amd.config import MODES, RaterConfig
from analyzer_amd.ops import Hindsight
from analyzer_amd.ops.native import native
from analyzer_amd.ops.rate import BatchRater, RateResult
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream

TILE = 4096  # sorted elements per workgroup of the scan (csrc/kernels.h kHindsightTile; checked below)
C = 20       # csrc/hindsight_core.h kHsBudgetC; checked below
U = 2.0 ** -53
RATED = 0
CFG = RaterConfig()
TAU = float(CFG.tau)
ALL_MODES = {m: 1.0 for m in MODES}
KS = (1, 2, 3, 4, 5)
DIGITS = 50


def check_constants():
    assert int(native().HINDSIGHT_TILE) == TILE and int(native().HINDSIGHT_BUDGET_C) == C


def cfg_tau(tau):
    return dataclasses.replace(CFG, tau=float(tau))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the oracle
def elements(rec, rows, P, track="shared"):
    """(elem [M, S] bool, ids [M, S], mu [M, S] fp32, sigma [M, S] fp32, bad) of a window, from
    the definition: live, rated, the player's last slot in the record, of the track's mode,
    with finite values and sigma >= 0; ``bad`` counts the slots that fail only the last."""
    r = rec.cpu().numpy().astype(np.int64)
    w = rows.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)
    M, cols = r.shape
    S = cols - 2
    K = S // 2
    ids = r[:, :S]
    mode, n0, n1 = r[:, S] & 0xFF, (r[:, S] >> 8) & 0xFF, (r[:, S] >> 16) & 0xFF
    pos = np.concatenate([np.arange(K), np.arange(K)])
    size = np.concatenate([np.repeat(n0[:, None], K, 1), np.repeat(n1[:, None], K, 1)], axis=1)
    live = (pos[None, :] < size) & (ids >= 0) & (ids < P) & (mode < 6)[:, None]
    last = live.copy()
    for j in range(S):
        for i in range(j):
            last[:, i] &= ~(live[:, i] & live[:, j] & (ids[:, i] == ids[:, j]))
    cand = last & ((w[:, 5 * S + 1] & 0xFF) == RATED)[:, None]
    lo = 0
    if track != "shared":
        cand &= (mode == MODES.index(track))[:, None]
        lo = 3 * S
    mu = w[:, lo:lo + S].copy().view(np.float32)
    sigma = w[:, lo + S:lo + 2 * S].copy().view(np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(mu) & np.isfinite(sigma) & ~(sigma < 0)
    return cand & ok, ids, mu, sigma, int((cand & ~ok).sum())


class Exact:
    """The exact smoothed values of the elements ``at`` (flat slot indices, chronological) as
    hi + lo pairs of doubles, with the length and the largest |mu| of each one's chain; and
    per player the exact carry (mu_s, P_s of its oldest element)."""

    def __init__(self, at, mu, sigma, n, top, carry):
        self.at, self.mu, self.sigma, self.n, self.top, self.carry = at, mu, sigma, n, top, carry


def _split(x):
    hi = float(x)
    return hi, float(x - mpmath.mpf(hi))


def oracle(elem, ids, mu, sigma, tau, players=None):
    """``Exact`` of every chain (or of the chains of ``players``): the backward loop in
    50-digit arithmetic on the fp32 inputs and the real tau^2."""
    flat = np.flatnonzero(elem.ravel())
    who = ids.ravel()[flat]
    m32, s32 = mu.ravel()[flat], sigma.ravel()[flat]
    order = np.argsort(who, kind="stable")
    at, emu, esig, ns, tops, carry = [], [], [], [], [], {}
    with mpmath.workdps(DIGITS):
        tau2 = mpmath.mpf(float(tau)) ** 2
        start = 0
        while start < len(order):
            end = start
            while end < len(order) and who[order[end]] == who[order[start]]:
                end += 1
            chain = order[start:end]
            start = end
            p = int(who[chain[0]])
            if players is not None and p not in players:
                continue
            n, top = len(chain), float(np.abs(m32[chain].astype(np.float64)).max())
            mh = ph = None
            for c in chain[::-1]:
                m_t, p_t = mpmath.mpf(float(m32[c])), mpmath.mpf(float(s32[c])) ** 2
                if mh is None:
                    mh, ph = m_t, p_t
                else:
                    d = p_t + tau2
                    g = p_t / d if d != 0 else mpmath.mpf(0)
                    mh = m_t + g * (mh - m_t)
                    ph = p_t + g * g * (ph - p_t - tau2)
                at.append(int(flat[c]))
                emu.append(_split(mh))
                esig.append(_split(mpmath.sqrt(ph)))
                ns.append(n)
                tops.append(top)
            carry[p] = (_split(mh), _split(ph), n, top)
    return Exact(np.array(at, dtype=np.int64), np.array(emu).reshape(-1, 2), np.array(esig).reshape(-1, 2),
                 np.array(ns, dtype=np.float64), np.array(tops), carry)


def ulp32(x):
    """The gap between the fp32 numbers around |x| (an array of doubles)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.frexp(np.maximum(x, 2.0 ** -126))[1]  # x = f 2^e, f in [0.5, 1)
    return np.ldexp(1.0, e - 24)


def budget(n, top, e_mu, e_sigma):
    return 0.5 * ulp32(e_mu) + C * n * U * top, 0.5 * ulp32(e_sigma) + (0.5 * C * n + 1.0) * U * np.abs(e_sigma)


def check_against(got, elem, ex, what, complete=True):
    """``got`` [M, S, 2] fp32 within the budget of the oracle's values at its elements; NaN at
    every slot that is no element (``complete``: the oracle holds every chain)."""
    g = np.asarray(got, dtype=np.float32).reshape(-1, 2)
    nan = np.isnan(g)
    assert (nan[:, 0] == nan[:, 1]).all(), what
    assert nan[~elem.ravel()].all(), (what, "a slot that is no element has a value")
    assert not nan[elem.ravel()].any(), (what, "an element without a value")
    if complete:
        assert len(ex.at) == int(elem.sum()), what
    v = g[ex.at].astype(np.float64)
    err_mu = np.abs((v[:, 0] - ex.mu[:, 0]) - ex.mu[:, 1])
    err_sigma = np.abs((v[:, 1] - ex.sigma[:, 0]) - ex.sigma[:, 1])
    b_mu, b_sigma = budget(ex.n, ex.top, ex.mu[:, 0], ex.sigma[:, 0])
    worst = (float((err_mu / b_mu).max(initial=0.0)), float((err_sigma / b_sigma).max(initial=0.0)))
    print("%s: %d elements, longest chain %d, worst error / budget: mu %.3f sigma %.3f"
          % (what, len(ex.at), int(ex.n.max(initial=0)), *worst))
    assert (err_mu <= b_mu).all() and (err_sigma <= b_sigma).all(), (what, worst)
    return worst


def check_carry(carry, ex, what):
    """The carry rows (mu_s, P_s) fp64 against the oracle: the fp64 part of the budget alone
    (nothing is rounded to fp32), NaN for a player without a chain."""
    carry = np.asarray(carry, dtype=np.float64)
    have = np.zeros(carry.shape[0], dtype=bool)
    for p, ((mh, ml), (ph, pl), n, top) in ex.carry.items():
        have[p] = True
        assert abs((carry[p, 0] - mh) - ml) <= C * n * U * top, (what, p, "mu")
        assert abs((carry[p, 1] - ph) - pl) <= C * n * U * ph, (what, p, "P")
    assert np.isnan(carry[~have]).all(), what


# ------------------------------------------------------------------ running the code under test
def run(device, rec, rows, P, track="shared", tau=TAU, cuts=(), max_slots=None):
    """(smoothed [M, S, 2] fp32, carry [P, 2] fp64, bad) of a history on ``device``: one window,
    or cut at the match indices ``cuts`` and added newest first."""
    hs = Hindsight(P, device, track=track, cfg=cfg_tau(tau))
    rec, rows = rec.to(device), rows.to(device)
    edges = [0, *cuts, rec.shape[0]]
    parts = [hs.add(rec[a:b], rows[a:b], max_slots=max_slots) for a, b in reversed(list(zip(edges[:-1], edges[1:])))]
    assert all(p.device.type == torch.device(device).type and p.dtype == torch.float32 for p in parts)
    out = torch.cat(parts[::-1]).cpu().numpy()
    assert out.shape == (rec.shape[0], rec.shape[1] - 2, 2)
    return out, hs.carry.cpu().numpy(), hs.bad


def check_window(device, rec, rows, P, what, track="shared", tau=TAU, **kw):
    """One history through the code under test against the full oracle; returns what both
    gave."""
    elem, ids, mu, sigma, bad = elements(rec, rows, P, track)
    ex = oracle(elem, ids, mu, sigma, tau)
    out, carry, got_bad = run(device, rec, rows, P, track=track, tau=tau, **kw)
    assert got_bad == bad, (what, got_bad, bad)
    check_against(out, elem, ex, "%s on %s" % (what, device))
    check_carry(carry, ex, what)
    return out, (elem, ids, mu, sigma), ex


# ------------------------------------------------------------------ windows
def window(K, ids, seed, mode=None, status=None, n0=None, n1=None, sigma=(150.0, 600.0)):
    """(rec, rows) of hand-made matches with the players ``ids`` [M, 2K]: random modes 0..5,
    full rosters and rated rows unless given, mu ~ N(1500, 400) and sigma uniform in ``sigma``
    -- a factor of four, within which the mirror's P_s[t+1] - P[t] - tau^2 loses no more than
    the budget allows (csrc/hindsight_core.h) -- independently on the shared and the mode
    fields, every other word of the row garbage."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, dtype=np.int64)
    M, S = ids.shape
    assert S == 2 * K
    W = RateResult.row_floats(K)
    rec = np.zeros((M, S + 2), dtype=np.int64)
    rec[:, :S] = ids
    mode = rng.integers(0, 6, M) if mode is None else np.broadcast_to(mode, (M,))
    n0 = np.full(M, K) if n0 is None else np.broadcast_to(n0, (M,))
    n1 = np.full(M, K) if n1 is None else np.broadcast_to(n1, (M,))
    rec[:, S] = mode | (n0 << 8) | (n1 << 16) | (2 << 24)
    rec[:, S + 1] = rng.integers(1, 3, M)
    rows = rng.uniform(1.0, 2.0, (M, W)).astype(np.float32)
    for lo in (0, 3 * S):
        rows[:, lo:lo + S] = rng.normal(1500.0, 400.0, (M, S))
        rows[:, lo + S:lo + 2 * S] = rng.uniform(sigma[0], sigma[1], (M, S))
    st = np.zeros(M, dtype=np.uint32) if status is None else np.asarray(status, dtype=np.uint32)
    rows.view(np.uint32)[:, 5 * S + 1] = st | 0x5A5A00  # only the low byte is the status
    return torch.from_numpy(rec.astype(np.int32)), torch.from_numpy(rows)


RATED_SPEC = dict(p_afk=0.05, p_unsupported=0.1, p_uneven=0.1, p_bad_rosters=0.04, p_tie=0.08)
RATED_P, RATED_M = 200, 2000


@functools.lru_cache(maxsize=None)
def rated(K, device):
    """(rec, rows) on the CPU: 2,000 matches over 200 players with every record feature on,
    rated by ``BatchRater`` on ``device`` (the host path on the CPU) from a roster with NULL
    tracks.  A real filtered history."""
    roster = make_roster(RosterSpec(num_players=RATED_P, seed=140 + K, p_rated=0.5, p_mode_rated=0.5), device=device)
    rec = make_stream(StreamSpec(team_size=K, seed=150 + K, modes=ALL_MODES, **RATED_SPEC), RATED_M, RATED_P, K=K,
                      device=device)
    res = BatchRater(CFG).rate(roster, rec, K)
    assert {0, 1, 2, 3} <= set(res.status.cpu().tolist())
    return rec.cpu(), res.packed.cpu().clone()


EDGE_COUNTS = (1000, 3096, 50, 4045, 2, 4096, 101)


@functools.lru_cache(maxsize=None)
def tile_edges():
    """1v1 matches in which player p has EDGE_COUNTS[p] elements, so in the sorted order a run
    ends exactly on the first tile edge (4,096), one ends one before the second (8,191, the
    next run of two straddles it) and one ends one after the third (12,289)."""
    ends = np.cumsum(EDGE_COUNTS)
    assert TILE in ends and 2 * TILE - 1 in ends and 3 * TILE + 1 in ends and ends[-1] % 2 == 0
    M = int(ends[-1]) // 2
    assert max(EDGE_COUNTS) <= M  # no player twice in a match
    seq = np.repeat(np.arange(len(EDGE_COUNTS)), EDGE_COUNTS)
    ids = np.stack([seq[:M], seq[M:]], axis=1)[np.random.default_rng(21).permutation(M)]
    return (*window(1, ids, seed=22), len(EDGE_COUNTS))


@functools.lru_cache(maxsize=None)
def every():
    """One player in every one of 5,000 1v1 matches: its run covers the whole first tile."""
    M = 5000
    ids = np.stack([np.zeros(M, dtype=np.int64), 1 + np.arange(M) % 5], axis=1)
    return (*window(1, ids, seed=23), 6)


STITCH_M, STITCH_P = 90_000, 40


@functools.lru_cache(maxsize=None)
def stitch():
    """90,000 3v3 matches over 40 players, no player twice in a match: 540,000 elements, 132
    tiles, 264 edges -- the stitch kernel runs a second iteration."""
    rng = np.random.default_rng(24)
    ids = np.argsort(rng.random((STITCH_M, STITCH_P)), axis=1)[:, :6]
    assert 2 * -(-STITCH_M * 6 // TILE) > 256
    return (*window(3, ids, seed=25), STITCH_P)


@functools.lru_cache(maxsize=None)
def messy(K=2, M=600, P=7):
    """Twins, AFK / invalid / unsupported / failed rows, ids outside [0, P), uneven and empty
    rosters, unsupported modes."""
    rng = np.random.default_rng(26)
    ids = rng.integers(0, P, (M, 2 * K))
    outside = rng.random(ids.shape) < 0.06
    ids[outside] = rng.choice([-1, P, P + 5, 2 ** 31 - 1, -7], int(outside.sum()))
    mode = rng.integers(0, 6, M)
    mode[rng.random(M) < 0.1] = 255
    mode[rng.random(M) < 0.03] = 6
    status = np.where(rng.random(M) < 0.25, rng.choice([1, 2, 3, 7, 255], M), RATED)
    rec, rows = window(K, ids, seed=27, mode=mode, status=status, n0=rng.integers(0, K + 1, M),
                       n1=rng.integers(0, K + 1, M))
    r = rec.numpy()
    assert any(row[0] == row[1] for row in r) and (r[:, :2 * K] >= P).any() and (r[:, :2 * K] < 0).any()
    return rec, rows, P


# ------------------------------------------------------------------ the checks
def check_hand_chain(device):
    """Player 0 plays three 1v1 matches; the expected values come from the formulas in exact
    rational arithmetic (the inputs are integers)."""
    m = [1500, 1520, 1490]
    s = [300, 250, 200]
    tau = 10
    rec, rows = window(1, [[0, 1], [2, 0], [0, 3]], seed=1)
    for t, j in enumerate((0, 1, 0)):  # player 0 sits in slot 0, 1, 0; K = 1: s_mu at [0, 2), s_sig at [2, 4)
        rows[t, j], rows[t, 2 + j] = float(m[t]), float(s[t])
    out, _, bad = run(device, rec, rows, 4, tau=tau)
    assert bad == 0
    mine = [out[0, 0], out[1, 1], out[2, 0]]
    mh, ph = Fraction(m[2]), Fraction(s[2] ** 2)
    assert bits(mine[2]).tolist() == bits(np.array([m[2], s[2]])).tolist()  # the newest is itself
    for t in (1, 0):
        p_t = Fraction(s[t] ** 2)
        g = p_t / (p_t + tau ** 2)
        mh, ph = m[t] + g * (mh - m[t]), p_t + g * g * (ph - p_t - tau ** 2)
        e_mu, e_sigma = float(mh), float(mpmath.sqrt(mpmath.mpf(ph.numerator) / ph.denominator))
        b_mu, b_sigma = budget(3.0, 1520.0, e_mu, e_sigma)
        assert abs(float(mine[t][0]) - e_mu) <= b_mu and abs(float(mine[t][1]) - e_sigma) <= b_sigma, (t, mine[t])
    # the players met once are their own smoothed values
    for (a, j), col in (((0, 1), 1), ((1, 0), 0), ((2, 1), 1)):
        assert bits(out[a, j]).tolist() == bits(rows[a, [col, 2 + col]].numpy()).tolist()


def check_team_size(K, device):
    """A rated history against the oracle, and what holds on a filter's output only: the
    smoothed sigma is at most the filtered one (within 1 fp32 ulp), and the smoothed mu lies
    between the smallest and the largest filtered mu of the element and the later ones."""
    rec, rows = rated(K, device)
    out, (elem, ids, mu, sigma), ex = check_window(device, rec, rows, RATED_P, "rated K=%d" % K)
    assert elem.sum() > RATED_M * K  # most slots are elements
    g = out.reshape(-1, 2)
    f_mu, f_sigma, who = mu.ravel(), sigma.ravel(), ids.ravel()
    flat = np.flatnonzero(elem.ravel())
    assert (g[flat, 1].astype(np.float64) <= f_sigma[flat].astype(np.float64) + ulp32(f_sigma[flat])).all()
    assert (g[flat, 1] < f_sigma[flat]).sum() > len(flat) // 2  # and mostly below it
    lo, hi = {}, {}
    for i in flat[::-1]:  # newest first
        p = who[i]
        lo[p], hi[p] = min(lo.get(p, np.inf), f_mu[i]), max(hi.get(p, -np.inf), f_mu[i])
        assert lo[p] <= g[i, 0] <= hi[p], (K, i, lo[p], g[i, 0], hi[p])
    check_newest_is_filtered(out, elem, ids, mu, sigma)
    return out


def check_newest_is_filtered(out, elem, ids, mu, sigma):
    """Bit for bit: the newest element of every chain is its filtered (mu, sigma)."""
    g = out.reshape(-1, 2)
    seen = set()
    for i in np.flatnonzero(elem.ravel())[::-1]:
        p = ids.ravel()[i]
        if p not in seen:
            seen.add(p)
            assert bits(g[i]).tolist() == bits(np.array([mu.ravel()[i], sigma.ravel()[i]])).tolist(), (i, p)
    assert seen


def check_mode_track(K, device):
    """A mode track of a rated mixed-mode history: only that mode's matches chain."""
    rec, rows = rated(K, device)
    out, (elem, _, _, _), _ = check_window(device, rec, rows, RATED_P, "ranked track K=%d" % K, track="ranked")
    modes = rec.numpy()[:, 2 * K] & 0xFF
    assert elem.any() and not elem[modes != MODES.index("ranked")].any()
    assert np.isnan(out[modes != MODES.index("ranked")]).all()
    shared = elements(rec, rows, RATED_P)[0]
    assert shared.sum() > 3 * elem.sum()  # the shared track chains all modes


def check_tile_edges(device):
    rec, rows, P = tile_edges()
    out, (elem, ids, mu, sigma), _ = check_window(device, rec, rows, P, "tile edges")
    assert elem.all()
    check_newest_is_filtered(out, elem, ids, mu, sigma)


def check_every(device):
    rec, rows, P = every()
    check_window(device, rec, rows, P, "one player in every match")


def check_stitch(device, mirror=None):
    """540,000 elements: sampled players against the oracle; the kernels against the host
    mirror ``mirror`` (its ``run`` result) at twice the budget."""
    rec, rows, P = stitch()
    elem, ids, mu, sigma, bad = elements(rec, rows, P)
    assert bad == 0 and elem.all()
    out, carry, got_bad = run(device, rec, rows, P)
    assert got_bad == 0
    ex = oracle(elem, ids, mu, sigma, TAU, players={0, 39})
    check_against(out, elem, ex, "stitch on %s" % device, complete=False)
    if mirror is not None:
        g, h = out.reshape(-1, 2).astype(np.float64), mirror[0].reshape(-1, 2).astype(np.float64)
        n = np.bincount(ids.ravel(), minlength=P).astype(np.float64)[ids.ravel()]
        top = np.zeros(P)
        np.maximum.at(top, ids.ravel(), np.abs(mu.ravel().astype(np.float64)))
        b_mu, b_sigma = budget(n, top[ids.ravel()], np.maximum(np.abs(g[:, 0]), np.abs(h[:, 0])),
                               np.maximum(g[:, 1], h[:, 1]))
        assert (np.abs(g[:, 0] - h[:, 0]) <= 2 * b_mu).all() and (np.abs(g[:, 1] - h[:, 1]) <= 2 * b_sigma).all()
        per = np.bincount(ids.ravel(), minlength=P).astype(np.float64)
        assert (np.abs(carry[:, 0] - mirror[1][:, 0]) <= 2 * C * per * U * top).all()
        assert (np.abs(carry[:, 1] - mirror[1][:, 1]) <= 2 * C * per * U * mirror[1][:, 1]).all()
    return out, carry


def check_window_cuts(device, K=3):
    """One window, uneven windows (1, 7, 100 matches, then the rest; newest first) and a tiny
    ``max_slots`` that forces chunks: each within the budget of the oracle, carries too."""
    rec, rows = rated(K, device)
    elem, ids, mu, sigma, bad = elements(rec, rows, RATED_P)
    ex = oracle(elem, ids, mu, sigma, TAU)
    M = rec.shape[0]
    for what, kw in (("one window", {}), ("uneven windows", {"cuts": (M - 108, M - 8, M - 1)}),
                     ("chunks", {"max_slots": 50 * 2 * K})):
        out, carry, got_bad = run(device, rec, rows, RATED_P, **kw)
        assert got_bad == bad
        check_against(out, elem, ex, "%s on %s" % (what, device))
        check_carry(carry, ex, what)


def check_rows_and_slots(device):
    rec, rows, P = messy()
    for track in ("shared", "blitz"):
        out, (elem, _, _, _), _ = check_window(device, rec, rows, P, "messy rows, %s" % track, track=track)
        assert 0 < elem.sum() < elem.size // 2
    # the rows next to the carry table are never touched
    hs = Hindsight(P, device)
    big = torch.full((P + 2, 2), 12345.0, dtype=torch.float64, device=device)
    big[1:P + 1] = float("nan")
    hs.carry = big[1:P + 1]
    hs.add(rec.to(device), rows.to(device))
    assert bool((big[0] == 12345.0).all()) and bool((big[P + 1] == 12345.0).all())
    assert not bool(torch.isnan(big[1:P + 1]).all())


def check_bad_values(device):
    """Rows poisoned with NaN, +-inf and a negative sigma: counted, skipped, and the chain goes
    on over them as if the slot were no element."""
    rec, rows, P = every()
    rows = rows.clone()
    M = rows.shape[0]
    rng = np.random.default_rng(28)
    hit = rng.choice(M, 60, replace=False)
    poison = [float("nan"), float("inf"), float("-inf")]
    for n, m in enumerate(hit):
        col = int(rng.integers(0, 4))  # s_mu / s_sig of slot 0 or 1
        rows[m, col] = poison[n % 3] if n % 4 else -abs(float(rows[m, col]))  # a negative mu is fine, a sigma is not
    rows[int(hit[0]), 2] = -0.0  # sigma = -0 is not negative
    elem, _, _, _, bad = elements(rec, rows, P)
    assert 30 < bad <= 60
    out, _, _ = check_window(device, rec, rows, P, "bad values")
    assert np.isnan(out[~elem]).all() and not np.isnan(out[elem]).any()


def check_degenerate(device, also_tau=None):
    """sigma = 0 with tau = 0: G = 0 / 0 is taken as 0, nothing is NaN, and behind such an
    element the older ones see it exactly.  ``also_tau``: the same rows with that tau, for the
    kernels only -- next to sigma = 0 the other sigmas are not within a factor of four, where
    the mirror's loop cancels (``window``)."""
    rec, rows, P = every()
    rows = rows[:400].clone()
    rec = rec[:400]
    rows[::7, 2:4] = 0.0
    out, (elem, _, _, _), _ = check_window(device, rec, rows, P, "sigma = 0, tau = 0", tau=0.0)
    assert elem.all() and not np.isnan(out).any()
    zero = np.flatnonzero(np.arange(400) % 7 == 0)
    assert (out[zero, 0, 1] == 0.0).all()
    if also_tau is not None:
        check_window(device, rec, rows, P, "sigma = 0, tau = %g" % also_tau, tau=also_tau)


def check_tau_zero(device):
    """tau = 0: every element of a chain equals the newest one, bit for bit."""
    rec, rows, P = tile_edges()
    out, _, bad = run(device, rec, rows, P, tau=0.0)
    elem, ids, mu, sigma, _ = elements(rec, rows, P)
    assert bad == 0
    g, who = bits(out).reshape(-1, 2), ids.ravel()
    for p in range(P):
        mine = np.flatnonzero(who == p)
        want = bits(np.array([mu.ravel()[mine[-1]], sigma.ravel()[mine[-1]]]))
        assert (g[mine] == want).all(), p


def check_empty(device):
    rec, rows, P = messy()
    hs = Hindsight(P, device)
    out = hs.add(rec[:0].to(device), rows[:0].to(device))
    assert tuple(out.shape) == (0, 4, 2) and hs.bad == 0 and bool(torch.isnan(hs.carry).all())
    none = Hindsight(0, device).add(rec.to(device), rows.to(device))
    assert bool(torch.isnan(none).all())


def check_arena(device):
    """``RecordArena.hindsight`` over a three-window arena equals ``Hindsight.add`` on the
    concatenation: both within the budget of the oracle, and its columns are the elements of
    the listed players in chronological order with their filtered values."""
    from analyzer_amd.runtime.rerate import RerateSpec, rerate_resident, stream_records

    spec = RerateSpec(total_matches=900, players=120, team_size=3, window=400, seed=2024)
    _, _, arena = rerate_resident(spec, device, free_bytes=1 << 40)
    assert len(list(arena.windows())) == 3
    rec_of = stream_records(spec, device)
    rec, rows = rec_of(0, 900).cpu(), arena.filled_rows().cpu()
    players = [5, 7, 119]
    for track in ("shared", "ranked"):
        out, (elem, ids, mu, sigma), ex = check_window(device, rec, rows, 120, "arena history, %s" % track,
                                                       track=track)
        cols = {k: v.cpu().numpy() for k, v in arena.hindsight(120, rec_of, players, track=track).items()}
        mine = np.flatnonzero(elem.ravel() & np.isin(ids.ravel(), players))
        assert len(mine) > 10
        assert (cols["match"] * 6 + cols["slot"] == mine).all()
        assert (cols["player"] == ids.ravel()[mine]).all()
        assert (bits(cols["mu"]) == bits(mu.ravel()[mine])).all()
        assert (bits(cols["sigma"]) == bits(sigma.ravel()[mine])).all()
        full = np.full((900 * 6, 2), np.nan, dtype=np.float32)
        full[mine, 0], full[mine, 1] = cols["mu_s"], cols["sigma_s"]
        pick = np.isin(ex.at, mine)
        sub = Exact(ex.at[pick], ex.mu[pick], ex.sigma[pick], ex.n[pick], ex.top[pick], {})
        only = np.zeros(elem.size, dtype=bool)
        only[mine] = True
        check_against(full, only, sub, "arena.hindsight, %s" % track)
    return arena
