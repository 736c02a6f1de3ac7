"""Helpers of the matchmaking tests (test_matchmake.py on the CPU, test_matchmake_gpu.py on
the device): rosters, lobbies, the oracle and the checks both suites share.

The oracle is independent of the code under test.  Priors: a numpy fp32 transcription of
the seeding and fall-back rules (and, for stream records, ``single_match_cases.priors``).
Split: K-subsets containing slot 0 from ``itertools.combinations`` sorted by mask value, d
as ``np.float32`` additions in slot order, the first minimal ``abs(d)``.  Quality and
p_win0: mpmath at 50 digits, with budgets that are derived (docs/ARCHITECTURE.md, "K12
error budget"), not fitted:

    dd        = (2K-1) U sum|mu_j|                        rounding of an fp32 sum of 2K terms
    B_quality = q (8U (1 + a) + |d| dd / den) + Q_FLOOR   a = d^2 / (2 den)
    B_p       = phi(t) (4U |t| + dd / sqrt(den)) + 8U p + 1.2e-38
    |d_chosen| <= min|d| + 2 dd                           two sequential fp32 sums compared
"""
import functools
import itertools
import json

import numpy as np
import pytest
import torch

from analyzer_amd.config import MODES, RaterConfig
from analyzer_amd.models.tiers import vst_table
from analyzer_amd.ops import balance_lobbies, make_lobbies, preview_matches
from analyzer_amd.ops import matchmake as MM
from analyzer_amd.ops.rate import BatchRater, Roster

import single_match_cases as SM
from single_match_cases import BETA, Q_FLOOR, U

CFG = RaterConfig()
US = np.float32(CFG.unknown_player_sigma)
KS = (1, 2, 3, 4, 5)
COUNTS = {1: 1, 2: 3, 3: 10, 4: 35, 5: 126}
P = 600            # players of the random-lobby roster: [0, 300) integer mus, [300, 600) fractional
L_RANDOM = 1000    # lobbies of the random set
SEEDS = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1}  # of the random-lobby sets; asserted below to cover every split
RATED, ERR_SEED, ERR_SIGMA, ERR_NUMERIC, ERR_BAD = 0, 4, 5, 7, 8
P_FLOOR = 1.2e-38  # the fp32 normal floor
NAN = float("nan")


def geometry(K):
    """(lanes per lobby, lobbies per wave, lobbies per workgroup): csrc/matchmake_core.h."""
    return MM.geometry(K)


def sizes(K):
    """L = 1, one below / at / one above the lobbies of a lane group (1), a wave and a
    workgroup, and 1000."""
    out = {1, 1000}
    for n in (1,) + tuple(geometry(K)[1:]):
        out |= {n - 1, n, n + 1}
    return sorted(out)


# ------------------------------------------------------------------ rosters
def empty_roster(num):
    return Roster.empty(num)


def set_track(roster, g, mu, sigma, players=None):
    idx = slice(None) if players is None else players
    roster.state[idx, 4 * g] = torch.as_tensor(np.asarray(mu, dtype=np.float32))
    roster.state[idx, 4 * g + 2] = torch.as_tensor(np.asarray(sigma, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def _random_roster():
    """Every track populated with its own values: players [0, 300) have integer mus on a
    narrow grid (sums are exact, ties are real), players [300, 600) fractional mus in
    0..3000 (rounding matters).  Never modified: use ``random_roster()``."""
    rng = np.random.default_rng(12)
    r = empty_roster(P)
    for g in range(7):
        mu = np.empty(P, dtype=np.float32)
        mu[:300] = rng.integers(1490, 1511, 300).astype(np.float32) + 3 * g
        mu[300:] = rng.uniform(0.0, 3000.0, 300).astype(np.float32)
        set_track(r, g, mu, rng.choice(np.array([30.0, 166.667, 500.0, 1000.0], dtype=np.float32), P))
    return r


def random_roster():
    return _random_roster().clone()


@functools.lru_cache(maxsize=None)
def random_lobbies(K):
    """[L_RANDOM, 2K] int32: distinct players, even rows from the integer half of the roster,
    odd rows from the fractional half."""
    rng = np.random.default_rng(100 * K + SEEDS[K])
    lob = np.empty((L_RANDOM, 2 * K), dtype=np.int32)
    for i in range(L_RANDOM):
        lob[i] = rng.choice(300, 2 * K, replace=False) + (300 if i & 1 else 0)
    return lob


# ------------------------------------------------------------------ the oracle
@functools.lru_cache(maxsize=None)
def oracle_masks(K):
    subsets = [c for c in itertools.combinations(range(2 * K), K) if 0 in c]
    return sorted(sum(1 << j for j in c) for c in subsets)


def np_priors(state, attrs, ids, mode):
    """(status, ms, ss, mm, sm) per id: fp32 priors after seeding (rank points, then the tier
    table) and the mode track's fall-back to shared; ``attrs`` None = no attributes."""
    vst = np.asarray(vst_table(), dtype=np.float32)
    two_thirds = np.float32(2.0 / 3.0)
    n = len(ids)
    st = np.zeros(n, dtype=np.uint8)
    out = np.full((4, n), np.nan, dtype=np.float32)
    g = 4 * (1 + mode)
    for k, p in enumerate(ids):
        row = state[p]
        sh_mu, sh_sig, md_mu, md_sig = row[0], row[2], row[g], row[g + 2]
        if np.isnan(sh_mu):
            rr, rb, tier = (np.float32(NAN),) * 3 if attrs is None else attrs[p, :3]
            rp = None
            if not np.isnan(rr) and rr != 0:
                rp = rr
            if not np.isnan(rb) and rb != 0 and (rp is None or rb > rp):
                rp = rb
            if rp is not None:
                sh_sig = np.float32(US * two_thirds)
                sh_mu = np.float32(np.float32(rp) + sh_sig)
            elif np.isnan(tier) or tier != int(tier) or not -1 <= int(tier) <= 29:
                st[k] = ERR_SEED
                continue
            else:
                sh_sig = US
                sh_mu = np.float32(vst[int(tier) + 1] + US)
        elif np.isnan(sh_sig) or sh_sig == 0:
            st[k] = ERR_SIGMA
            continue
        if np.isnan(md_mu):
            md_mu, md_sig = sh_mu, sh_sig
        elif np.isnan(md_sig) or md_sig == 0:
            st[k] = ERR_SIGMA
            continue
        out[:, k] = sh_mu, sh_sig, md_mu, md_sig
    return (st,) + tuple(out)


def split_d32(mu, mask):
    d = np.float32(mu[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(1, len(mu)):
            d = np.float32(d + (mu[j] if (mask >> j) & 1 else -mu[j]))
    return d


def split_d32_all(mu, masks):
    """[L, C] fp32: ``split_d32`` of every row of ``mu`` [L, 2K] for every mask, the same
    sequence of fp32 additions."""
    mu = np.asarray(mu, dtype=np.float32)
    out = np.empty((mu.shape[0], len(masks)), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c, m in enumerate(masks):
            d = mu[:, 0].copy()
            for j in range(1, mu.shape[1]):
                d = d + (mu[:, j] if (m >> j) & 1 else -mu[:, j])
            assert d.dtype == np.float32
            out[:, c] = d
    return out


def _mp():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    return mp


def mp_match(mu, sig, signs, dd_terms):
    """50-digit quality and p_win0 of fp32 priors with team signs (+1 team 0, -1 team 1), and
    their budgets; ``dd_terms``: the roundings of the kernel's d sum."""
    mp = _mp()
    n = len(mu)
    d = sum(s * mp.mpf(float(m)) for m, s in zip(mu, signs))
    nb2 = n * mp.mpf(BETA) ** 2
    den = nb2 + sum(mp.mpf(float(s)) ** 2 for s in sig)
    a = d * d / (2 * den)
    q = mp.sqrt(nb2 / den) * mp.exp(-a)
    t = d / mp.sqrt(den)
    p = mp.ncdf(t)
    dd = dd_terms * U * sum(abs(float(m)) for m in mu)
    b_q = float(q * (8 * U * (1 + a) + abs(d) * dd / den)) + Q_FLOOR
    b_p = float(mp.npdf(t) * (4 * U * abs(t) + dd / mp.sqrt(den)) + 8 * U * p) + P_FLOOR
    # the executor's own budget (single_match_cases.oracle): its team sums round 2n times
    dd_rate = 2 * n * U * sum(abs(float(m)) for m in mu)
    b_q_rate = float(q * (8 * U * (1 + a) + abs(d) * dd_rate / den)) + Q_FLOOR
    return dict(q=float(q), p=float(p), B_q=b_q, B_p=b_p, B_q_rate=b_q_rate, d=float(d), dd=dd, den=float(den))


def oracle_balance(roster, lobbies, mode, attrs=True, budgets=True):
    """Expected outputs of ``balance_lobbies`` for numpy lobbies [L, 2K] on mode index
    ``mode``: exact status / split / team0 / records, and per sound lobby the 50-digit
    quality, p_win0, quality_given with their budgets and the fp64 brute-force min |d|."""
    state = roster.state.numpy()
    at = roster.attrs.numpy() if attrs else None
    L, S = lobbies.shape
    K = S // 2
    masks = oracle_masks(K)
    num = state.shape[0]
    o = dict(status=np.zeros(L, dtype=np.uint8), split=np.full(L, -1, dtype=np.int32),
             team0=np.zeros(L, dtype=np.int32), records=np.zeros((L, S + 2), dtype=np.int32))
    for k in ("q", "p", "qg", "B_q", "B_p", "B_qg", "B_q_rate", "d", "d_min64", "dd"):
        o[k] = np.full(L, np.nan)
    meta0 = mode | (K << 8) | (K << 16) | (2 << 24)
    for i in range(L):
        ids = [int(x) for x in lobbies[i]]
        o["records"][i, :S], o["records"][i, S] = ids, meta0
        if any(p < 0 or p >= num for p in ids) or len(set(ids)) < S:
            o["status"][i] = ERR_BAD
            continue
        st, ms, ss, mm, sm = np_priors(state, at, ids, mode)
        if (st == ERR_SEED).any():
            o["status"][i] = ERR_SEED
            continue
        if (st == ERR_SIGMA).any():
            o["status"][i] = ERR_SIGMA
            continue
        ds = split_d32_all(mm[None], masks)[0]
        assert ds[0].tobytes() == split_d32(mm, masks[0]).tobytes()
        if not (np.isfinite(np.stack([ms, ss, mm, sm])).all() and np.isfinite(ds).all()):
            o["status"][i] = ERR_NUMERIC
            continue
        best = int(np.argmin(np.abs(ds)))  # the first minimal |d|
        mask = masks[best]
        o["split"][i], o["team0"][i] = best, mask
        t0 = [j for j in range(S) if (mask >> j) & 1]
        t1 = [j for j in range(S) if not (mask >> j) & 1]
        o["records"][i, :S] = [ids[j] for j in t0 + t1]
        mu64 = mm.astype(np.float64)
        o["d_min64"][i] = min(abs(sum(mu64[j] if (m >> j) & 1 else -mu64[j] for j in range(S))) for m in masks)
        o["dd"][i] = (S - 1) * U * np.abs(mu64).sum()
        o["d"][i] = abs(sum(mu64[j] if (mask >> j) & 1 else -mu64[j] for j in range(S)))
        if budgets:
            c = mp_match(mm, sm, [1 if (mask >> j) & 1 else -1 for j in range(S)], S - 1)
            g = mp_match(mm, sm, [1 if j < K else -1 for j in range(S)], S - 1)
            o["q"][i], o["p"][i], o["B_q"][i], o["B_p"][i] = c["q"], c["p"], c["B_q"], c["B_p"]
            o["qg"][i], o["B_qg"][i], o["B_q_rate"][i] = g["q"], g["B_q"], c["B_q_rate"]
    return o


@functools.lru_cache(maxsize=None)
def random_oracle(K, mode=1):
    return oracle_balance(_random_roster(), random_lobbies(K), mode)


def _check_inputs():
    """The input conditions of the random-lobby sets, from the oracle's split choice alone."""
    state = _random_roster().state.numpy()
    for K in KS:
        masks = oracle_masks(K)
        assert len(masks) == COUNTS[K] and masks[0] == (1 << K) - 1
        ds = np.abs(split_d32_all(state[random_lobbies(K), 8], masks))  # the ranked track: mode 1
        won = set(np.argmin(ds, axis=1).tolist())
        tied = int(((ds == ds.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        assert won == set(range(COUNTS[K])), "K = %d: splits %s never win" % (K, sorted(set(range(COUNTS[K])) - won))
        assert K == 1 or tied > 0, "K = %d: no lobby has a real tie" % K
    mu = state[:, 8]
    assert (mu[:300] == np.round(mu[:300])).all() and (mu[300:] != np.round(mu[300:])).any()
    assert 0.0 <= mu[300:].min() and mu[300:].max() <= 3000.0


_check_inputs()


# ------------------------------------------------------------------ comparisons
def run_balance(roster, lobbies, device, mode="ranked"):
    """``balance_lobbies`` on ``device`` as numpy arrays."""
    r = roster.to(device)
    lob = torch.as_tensor(np.ascontiguousarray(lobbies), dtype=torch.int32).to(device)
    bal = balance_lobbies(r, lob, mode=mode, cfg=CFG)
    return {k: getattr(bal, k).cpu().numpy() for k in bal._fields}


def ratio(got, exp, bud):
    err = np.abs(np.asarray(got, dtype=np.float64) - exp)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bud)


WORST = {}  # what -> worst |error| / budget seen, for the figures of docs/ARCHITECTURE.md


def note(what, r):
    if r.size:
        WORST[what] = max(WORST.get(what, 0.0), float(np.max(r)))


def assert_balance(got, orc, rows=slice(None), what="", device="cpu"):
    """Exact split outputs; NaN pattern; floats within their budgets; the |d| bound."""
    exp = {k: v[rows] for k, v in orc.items()}
    for k in ("status", "split", "team0", "records"):
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), "%s: %s differs at rows %s" % (
            what, k, np.nonzero((got[k] != exp[k]).reshape(len(exp[k]), -1).any(1))[0][:10])
    ok = exp["status"] == RATED
    for k in ("quality", "p_win0", "quality_given"):
        assert got[k].dtype == np.float32 and np.array_equal(np.isnan(got[k]), ~ok), "%s: NaN pattern of %s" % (what, k)
    if not ok.any() or np.isnan(exp["q"][ok]).all():
        return
    tag = "device" if str(device).startswith("cuda") else "host"
    for k, e, b in (("quality", "q", "B_q"), ("p_win0", "p", "B_p"), ("quality_given", "qg", "B_qg")):
        r = ratio(got[k][ok], exp[e][ok], exp[b][ok])
        note("%s %s" % (tag, k), r)
        print("%s worst |error| / budget of %s: %.4f" % (what, k, r.max()))
        assert (r <= 1.0).all(), "%s: %s outside its budget: ratio %.3f at sound lobby %d" % (
            what, k, r.max(), int(np.argmax(r)))
    assert (exp["d"][ok] <= exp["d_min64"][ok] + 2 * exp["dd"][ok]).all(), "%s: the chosen |d| is not minimal" % what


# ------------------------------------------------------------------ 1. sizes
def check_sizes(K, device):
    orc = random_oracle(K)
    roster = random_roster().to(device)
    for L in sizes(K):
        got = run_balance(roster, random_lobbies(K)[:L], device)
        assert got["records"].shape == (L, 2 * K + 2)
        assert_balance(got, orc, slice(0, L), "K = %d, L = %d" % (K, L), device)


# ------------------------------------------------------------------ 2. ties
def check_ties(device):
    r = empty_roster(40)
    set_track(r, 0, np.full(40, 1500.0), np.full(40, 100.0))
    mu = np.full(40, 1500.0, dtype=np.float32)
    mu[10:14] = 1, 2, 3, 4            # the 2v2 lobby 1, 2, 3, 4
    mu[20:26] = 10, 7, 1, 3, 4, 1     # a 3v3 lobby of small integers: several splits tie
    set_track(r, 2, mu, np.full(40, 100.0))
    for K in KS:  # all mus equal: every split ties at d = 0, index 0 stays
        got = run_balance(r, np.arange(2 * K, dtype=np.int32)[None], device)
        assert got["status"][0] == 0 and got["split"][0] == 0 and got["team0"][0] == (1 << K) - 1
    got = run_balance(r, np.array([[10, 11, 12, 13]], dtype=np.int32), device)
    assert got["split"][0] == 2 and got["team0"][0] == 0b1001, got
    assert list(got["records"][0, :4]) == [10, 13, 11, 12]
    # +x and -x: 10, 1, 10, 3 -> {0,1} d = -2, {0,2} d = +16, {0,3} d = +2: the lower index wins
    mu[30:34] = 10, 1, 10, 3
    set_track(r, 2, mu, np.full(40, 100.0))
    lob = np.array([[30, 31, 32, 33]], dtype=np.int32)
    orc = oracle_balance(r, lob, 1)
    ds = [float(split_d32(mu[30:34], m)) for m in oracle_masks(2)]
    assert ds[0] == -2.0 and ds[2] == 2.0 and abs(ds[1]) > 2.0
    got = run_balance(r, lob, device)
    assert got["split"][0] == 0 == orc["split"][0]
    assert_balance(got, orc, what="+x / -x tie", device=device)
    assert_balance(run_balance(r, np.array([[20, 21, 22, 23, 24, 25]], dtype=np.int32), device),
                   oracle_balance(r, np.array([[20, 21, 22, 23, 24, 25]], dtype=np.int32), 1), what="3v3 ties",
                   device=device)


# ------------------------------------------------------------------ 3. modes
@functools.lru_cache(maxsize=None)
def _mode_roster():
    """64 players: all six modes and shared distinct; players 40.. with a NULL mode track on
    every mode; 48.. with a NULL shared track seeded from ranked points (48..51), blitz
    points (52..55, the larger of both for 54, 55) or the tier (56..63)."""
    rng = np.random.default_rng(3)
    r = empty_roster(64)
    for g in range(7):
        set_track(r, g, rng.uniform(500.0, 2500.0, 64), rng.uniform(50.0, 600.0, 64))
    r.state[40:, 4:28:4] = NAN
    r.state[40:, 6:28:4] = NAN
    r.state[48:, 0] = NAN
    r.state[48:, 2] = NAN
    at = r.attrs
    at[48:52, 0] = torch.tensor([1200.0, 1750.5, 2400.0, 900.25])
    at[52:56, 1] = torch.tensor([1100.0, 1999.0, 2100.0, 1300.0])
    at[54:56, 0] = torch.tensor([2050.0, 1350.0])
    at[56:64, 2] = torch.tensor([-1.0, 0.0, 1.0, 7.0, 12.0, 20.0, 27.0, 29.0])
    return r


def check_modes(device):
    r = _mode_roster().clone()
    rng = np.random.default_rng(4)
    lob = np.stack([rng.choice(64, 6, replace=False) for _ in range(40)]).astype(np.int32)
    lob[0] = 48, 52, 54, 56, 60, 63   # every kind of seed in one lobby
    lob[1] = 40, 41, 42, 43, 44, 45   # fall-back to shared only
    answers = set()
    for m, name in enumerate(MODES):
        orc = oracle_balance(r, lob, m)
        assert (orc["status"] == 0).all()
        got = run_balance(r, lob, device, mode=name)
        assert_balance(got, orc, what="mode %s" % name, device=device)
        pre = run_balance(r, lob, device, mode="trueskill_" + name)
        assert all(np.array_equal(got[k], pre[k], equal_nan=True) for k in got)
        answers.add(got["quality"][2:].tobytes())
    assert len(answers) == len(MODES), "two modes gave the same qualities: a wrong granule was read"
    # a bare state tensor: no attributes, so a NULL shared track cannot be seeded
    got = run_balance(r.state, lob, device)
    orc = oracle_balance(r, lob, 1, attrs=False)
    assert orc["status"][0] == ERR_SEED and (orc["status"] == 0).any()
    assert_balance(got, orc, what="state tensor only", device=device)


# ------------------------------------------------------------------ 4. errors
def _error_roster():
    r = random_roster()
    r.state[590, 0], r.state[590, 2] = NAN, NAN   # NULL shared and tier 30: kErrSeed
    r.attrs[590, 2] = 30.0
    r.state[591, 10] = 0.0                        # sigma 0 on the ranked track: kErrSigma
    r.state[592, 8] = float("inf")                # mu = inf on the ranked track: kErrNumeric
    r.state[593, 2] = 0.0                         # sigma 0 on the shared track
    return r


def error_lobbies(K, kind):
    """A wave and a half of sound lobbies (players < 580) with one bad lobby in the middle
    of the first wave."""
    S = 2 * K
    n = geometry(K)[1] * 3 // 2 + 1
    lob = random_lobbies(K)[1:1 + n].copy()
    lob[lob >= 580] -= 100
    at = geometry(K)[1] // 2
    row = lob[at]
    if kind == "id -1":
        row[S - 1] = -1
    elif kind == "id P":
        row[0] = P
    elif kind == "repeated":
        row[S - 1] = row[0]
    elif kind == "seed":
        row[1] = 590
    elif kind == "sigma":
        row[0] = 591
    elif kind == "numeric":
        row[S - 1] = 592
    elif kind == "bad+seed":      # precedence: bad record first
        row[0], row[1] = 590, -1
    elif kind == "sigma+seed":    # seed before sigma, whatever the slots
        row[0], row[1] = 591, 590
    elif kind == "numeric+sigma":
        row[0], row[1] = 592, 593
    return lob, at


ERROR_KINDS = {"id -1": ERR_BAD, "id P": ERR_BAD, "repeated": ERR_BAD, "seed": ERR_SEED, "sigma": ERR_SIGMA,
               "numeric": ERR_NUMERIC, "bad+seed": ERR_BAD, "sigma+seed": ERR_SEED, "numeric+sigma": ERR_SIGMA}


def check_errors(K, device):
    r = _error_roster()
    for kind, status in ERROR_KINDS.items():
        lob, at = error_lobbies(K, kind)
        if K == 1 and kind == "repeated":
            lob[at, 1] = lob[at, 0]
        orc = oracle_balance(r, lob, 1, budgets=False)
        assert orc["status"][at] == status and (np.delete(orc["status"], at) == 0).all(), (kind, orc["status"])
        got = run_balance(r, lob, device)
        assert_balance(got, orc, what="K = %d, %s" % (K, kind), device=device)
        assert got["split"][at] == -1 and got["team0"][at] == 0 and np.array_equal(got["records"][at, :2 * K], lob[at])
        rest = np.delete(np.arange(len(lob)), at)  # the neighbours: as in a run without the bad lobby
        alone = run_balance(r, lob[rest], device)
        for k in got:
            assert np.array_equal(got[k][rest], alone[k], equal_nan=True), "%s: %s of a neighbour moved" % (kind, k)


# ------------------------------------------------------------------ 5. read-only
def check_read_only(roster, device):
    """``roster`` on ``device`` (its tags as they are): every call leaves every bit alone, and
    the results equal those on a copy with all tags zeroed."""
    before = roster.state.clone()
    attrs = roster.attrs.clone()
    clean = roster.clone()
    clean.state[:, 1::2] = 0.0
    num = roster.num_players
    rng = np.random.default_rng(8)
    lob = torch.as_tensor(np.stack([rng.choice(num, 6, replace=False) for _ in range(100)]).astype(np.int32)).to(device)
    rec = torch.cat([lob, torch.tensor([[1 | (3 << 8) | (3 << 16) | (2 << 24), 1]], dtype=torch.int32,
                                       device=device).expand(100, 2)], 1).contiguous()
    queue = torch.as_tensor(rng.permutation(num).astype(np.int32)[:200]).to(device)
    outs = []
    for r in (roster, clean):
        bal = balance_lobbies(r, lob, "ranked", cfg=CFG)
        pv = preview_matches(r, rec, cfg=CFG)
        made, left = make_lobbies(r, queue, "ranked", K=3, cfg=CFG)
        outs.append([x.cpu() for x in tuple(bal) + tuple(pv) + tuple(made) + (left,)])
    assert torch.equal(roster.state.view(torch.int32), before.view(torch.int32)), "the roster state changed"
    assert torch.equal(roster.attrs.view(torch.int32), attrs.view(torch.int32))
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy(), equal_nan=True), "tags changed a result"
    assert (outs[0][0] == 0).any()


def live_roster():
    """The random roster with arbitrary bits, NaN patterns included, in every tag word."""
    r = random_roster()
    rng = np.random.default_rng(5)
    tags = rng.integers(0, 1 << 32, (P, 16), dtype=np.uint64).astype(np.uint32)
    tags[rng.random((P, 16)) < 0.25] |= 0x7f800001
    r.state.view(torch.int32)[:, 1::2] = torch.as_tensor(tags.view(np.int32))
    return r


# ------------------------------------------------------------------ 6. preview against rate
def preview_cases(K):
    """(cases, patches, expected status): matches with disjoint players.  ``patches`` edit the
    built records (row -> function) for what a ``Case`` cannot say."""
    S = 2 * K
    g = SM.grid(K)
    pick = [g[i] for i in range(0, len(g), max(1, len(g) // 12))][:12]   # outcomes, surpluses, sigma patterns
    cases = list(pick)
    status = [RATED] * len(cases)
    patches = {}

    def plain(**kw):
        mu = [1400.0 + 37.0 * j for j in range(S)]
        base = dict(K=K, mu=mu, sig=[200.0] * S, mmu=[m + 11.0 for m in mu], msig=[150.0 + j for j in range(S)],
                    n1=K, mode=2)
        base.update(kw)
        return SM.Case(**base)

    def add(case, st, patch=None):
        cases.append(case)
        status.append(st)
        if patch is not None:
            patches[len(cases) - 1] = patch

    if K >= 2:
        add(plain(n1=K - 1), RATED)                                   # uneven teams
        add(plain(n0=K - 1, n1=K), RATED)
        add(plain(players=list(range(S - 1)) + [0]), RATED)           # one player on both teams
        add(plain(players=[0, 0] + list(range(2, S))), RATED)         # ... twice in one team
    # seeded shared track: ranked points; the oracle takes the fp32 seed
    sig_rp = float(np.float32(US * np.float32(2.0 / 3.0)))
    mu0 = [None] + [1500.0] * (S - 1)
    add(plain(mu=mu0, sig=[None] + [200.0] * (S - 1), mmu=[None] * S, msig=[None] * S,
              attrs={0: (1800.0, None, None)}, seed={0: (float(np.float32(np.float32(1800.0) + np.float32(sig_rp))), sig_rp)}),
        RATED)
    add(plain(), 1, lambda rec, i: rec.__setitem__((i, S + 1), int(rec[i, S + 1]) | 4 | (1 << 8)))          # AFK
    add(plain(), 2, lambda rec, i: rec.__setitem__((i, S), (int(rec[i, S]) & 0xffffff) | (3 << 24)))       # 3 rosters
    add(plain(), 2, lambda rec, i: rec.__setitem__((i, S), (int(rec[i, S]) & 0xffffff) | (1 << 24)))
    add(plain(), 3, lambda rec, i: rec.__setitem__((i, S), (int(rec[i, S]) & ~0xff) | 9))                  # mode 9
    add(plain(mu=mu0, sig=[None] + [200.0] * (S - 1), attrs={0: (None, None, 30.0)}), ERR_SEED)
    add(plain(sig=[200.0] * (S - 1) + [0.0]), ERR_SIGMA)
    add(plain(msig=[0.0] + [150.0] * (S - 1)), ERR_SIGMA)
    add(plain(n0=0), 6)                                                                                     # empty roster
    add(plain(), ERR_BAD, lambda rec, i: rec.__setitem__((i, 0), rec.shape[0] * S))                         # id = P
    add(plain(), ERR_BAD, lambda rec, i: rec.__setitem__((i, S), (int(rec[i, S]) & ~0xff00) | ((K + 1) << 8)))  # n0 > K
    add(plain(), RATED)
    return cases, patches, np.array(status, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def preview_window(K):
    cases, patches, status = preview_cases(K)
    roster, rec, _ = SM.build_window(cases)
    for i, f in patches.items():
        f(rec, i)
    rated = np.nonzero(status == RATED)[0]
    orc = SM.oracle([cases[i] for i in rated])
    mp = _mp()
    p = np.full(len(cases), np.nan)
    b_p = np.full(len(cases), np.nan)
    for i in rated:
        c = cases[i]
        pr = SM.priors(c)
        slots = c.slots()
        m = mp_match([pr[j][2] for j in slots], [pr[j][3] for j in slots], [1 if j < K else -1 for j in slots], 2 * K - 1)
        p[i], b_p[i] = m["p"], m["B_p"]
    del mp
    return roster, rec, status, rated, orc, p, b_p


def swap_teams(rec, K):
    S = 2 * K
    out = rec.clone()
    out[:, :K], out[:, K:S] = rec[:, K:S], rec[:, :K]
    m0 = rec[:, S]
    out[:, S] = (m0 & ~0xffff00) | (((m0 >> 16) & 0xff) << 8) | (((m0 >> 8) & 0xff) << 16)
    return out


def check_preview(K, device):
    roster, rec, status, rated, orc, p, b_p = preview_window(K)
    roster, rec = roster.clone().to(device), rec.to(device)
    before = roster.state.clone()
    pv = preview_matches(roster.clone(), rec, cfg=CFG)
    assert torch.equal(roster.state.view(torch.int32), before.view(torch.int32))
    res = BatchRater(CFG).rate(roster, rec)
    st, q, pw = pv.status.cpu().numpy(), pv.quality.cpu().numpy(), pv.p_win0.cpu().numpy()
    assert np.array_equal(st, status), (st, status)
    assert np.array_equal(res.status.cpu().numpy(), st), "preview and rate disagree on a status"
    rq = res.quality.cpu().numpy()
    assert np.array_equal(np.isnan(q), np.isnan(rq)) and np.array_equal(q[st != 0], rq[st != 0], equal_nan=True)
    assert (q[(st == 1) | (st == 2)] == 0).all() and np.isnan(q[st >= 3]).all()
    assert np.array_equal(np.isnan(pw), st != 0)
    tag = "device" if str(device).startswith("cuda") else "host"
    for what, v in (("preview quality", q), ("rate quality", rq)):
        r = ratio(v[rated], orc["quality"], orc["B_quality"])
        note("%s %s" % (tag, what), r)
        assert (r <= 1.0).all(), "K = %d: %s outside B_quality: %.3f (case %d)" % (K, what, r.max(), rated[np.argmax(r)])
    if tag == "host":
        assert np.array_equal(q.view(np.uint32), rq.view(np.uint32)), "fp64 mirror: preview and rate qualities differ"
    r = ratio(pw[rated], p[rated], b_p[rated])
    note("%s preview p_win0" % tag, r)
    assert (r <= 1.0).all(), "K = %d: p_win0 outside B_p: %.3f (case %d)" % (K, r.max(), rated[np.argmax(r)])
    sw = preview_matches(_fresh(K, device), swap_teams(rec, K), cfg=CFG)
    sp = sw.p_win0.cpu().numpy()
    assert np.array_equal(sw.status.cpu().numpy()[rated], st[rated])
    assert (np.abs(sp[rated].astype(np.float64) - (1.0 - pw[rated].astype(np.float64))) <= 2 * b_p[rated]).all()
    # the winner bits make no difference, bit for bit
    fresh = _fresh(K, device)
    for bits in (0, 1, 2, 3):
        other = rec.clone()
        other[:, -1] = (other[:, -1] & ~3) | bits
        o = preview_matches(fresh, other, cfg=CFG)
        a = preview_matches(fresh, rec, cfg=CFG)
        for x, y in zip(o, a):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)


def _fresh(K, device):
    return preview_window(K)[0].to(device).clone()


# ------------------------------------------------------------------ 7. round trip
def check_round_trip(K, device):
    S = 2 * K
    roster = random_roster()
    lob = np.random.default_rng(40 + K).permutation(P)[:(P // S) * S].reshape(-1, S).astype(np.int32)
    lob[3, S - 1] = lob[3, 0]                      # one status-8 lobby
    orc = oracle_balance(roster, lob, 1)
    dev_roster = roster.to(device)
    bal = balance_lobbies(dev_roster, torch.as_tensor(lob).to(device), "ranked", cfg=CFG)
    got = {k: getattr(bal, k).cpu().numpy() for k in bal._fields}
    assert_balance(got, orc, what="round trip K = %d" % K, device=device)
    ok = got["status"] == 0
    assert ok.sum() == len(lob) - 1
    assert all(sorted(a[:S]) == sorted(b) for a, b in zip(got["records"][ok], lob[ok])), "not a permutation"
    for winner in (0, 1, 2):
        res = BatchRater(CFG).rate(dev_roster.clone(), MM.fill_winners(bal.records[bal.status == 0], winner))
        assert (res.status.cpu().numpy() == 0).all()
    # the executor sums d itself: single_match_cases' dd = 2 n U sum|mu|
    r = ratio(res.quality.cpu().numpy(), orc["q"][ok], orc["B_q_rate"][ok])
    assert (r <= 1.0).all(), "rate's quality of a balanced record: %.3f" % r.max()
    # balancing never loses quality beyond the |d| bound: q is decreasing in |d|
    mp = _mp()
    for i in np.nonzero(ok)[0]:
        mm = roster.state.numpy()[lob[i], 8].astype(np.float64)
        dg = abs(mm[:K].sum() - mm[K:].sum()) + 2 * orc["dd"][i]
        den = S * BETA ** 2 + float((roster.state.numpy()[lob[i], 10].astype(np.float64) ** 2).sum())
        floor = float(mp.sqrt(S * BETA ** 2 / den) * mp.exp(-mp.mpf(dg) ** 2 / (2 * den)))
        assert got["quality"][i] >= floor - orc["B_q"][i], (i, got["quality"][i], floor)


# ------------------------------------------------------------------ 8. make_lobbies
QUEUE_P = 1200


@functools.lru_cache(maxsize=None)
def _queue_roster():
    """1200 players on a grid of 40 integer mus (many ties); a NULL shared track with tier 30
    (1190..1194) and a zero sigma (1195..1199) fail."""
    rng = np.random.default_rng(21)
    r = empty_roster(QUEUE_P)
    for g in range(7):
        set_track(r, g, rng.integers(1480, 1520, QUEUE_P).astype(np.float32) + g, rng.uniform(50.0, 500.0, QUEUE_P))
    r.state[1190:1195, 0] = NAN
    r.state[1190:1195, 2] = NAN
    r.attrs[1190:1195, 2] = 30.0
    r.state[1195:1200, 10] = 0.0
    r.state[7, 8] = -0.0   # canonicalised to +0: ties with 0
    r.state[8, 8] = 0.0
    return r


def queue_size(K, name):
    return {"0": 0, "1": 1, "2K-1": 2 * K - 1, "2K": 2 * K, "2K+1": 2 * K + 1, "1000": 1000}[name]


def oracle_queue(roster, queue, mode):
    """(sorted valid positions, failed positions): descending fp32 mu + 0, ties and failures in
    queue order."""
    state, at = roster.state.numpy(), roster.attrs.numpy()
    num = state.shape[0]
    valid, failed = [], []
    for i, p in enumerate(queue):
        if p < 0 or p >= num:
            failed.append(i)
            continue
        st, _, _, mm, _ = np_priors(state, at, [int(p)], mode)
        if st[0] != 0 or np.isnan(mm[0]):
            failed.append(i)
        else:
            valid.append((-float(mm[0] + np.float32(0.0)), i))
    return [i for _, i in sorted(valid)], failed


def check_make_lobbies(K, Q, device, repeat=False):
    S = 2 * K
    roster = _queue_roster().clone()
    rng = np.random.default_rng(7 * K + Q)
    queue = rng.permutation(QUEUE_P)[:Q].astype(np.int32)
    if Q >= 1000:  # failed players are in; two ids outside the roster
        queue[5], queue[6] = -1, QUEUE_P
        assert np.isin(np.arange(1190, 1200), queue).sum() >= 5
    if repeat:     # the best player queues twice: both entries land in the first lobby
        mu = roster.state.numpy()[:, 8]
        best = int(np.argmax(np.where(np.isin(np.arange(QUEUE_P), queue) & (np.arange(QUEUE_P) < 1190), mu, -1e9)))
        roster.state[best, 8] = 5000.0
        queue[-1] = best
    order, failed = oracle_queue(roster, queue, 1)
    n = len(order) // S
    lob = queue[order[:n * S]].reshape(n, S)
    left = np.concatenate([queue[order[n * S:]], queue[failed]]).astype(np.int32)
    orc = oracle_balance(roster, lob, 1, budgets=False)
    bal, unmatched = make_lobbies(roster.to(device), torch.as_tensor(queue).to(device), mode="ranked", K=K, cfg=CFG)
    got = {k: getattr(bal, k).cpu().numpy() for k in bal._fields}
    assert got["status"].shape == (n,) and got["records"].shape == (n, S + 2)
    assert unmatched.dtype == torch.int32 and np.array_equal(unmatched.cpu().numpy(), left), (unmatched, left)
    assert_balance(got, orc, what="make_lobbies K = %d, Q = %d" % (K, Q), device=device)
    if Q >= 1000:
        mu = roster.state.numpy()[lob.reshape(-1), 8]
        assert (np.diff(mu) <= 0).all() and (np.diff(mu) == 0).any(), "lobbies are not in descending-mu order with ties"
    if repeat:
        assert got["status"][0] == ERR_BAD and (got["status"][1:] == 0).all()
    elif n:
        assert (got["status"] == 0).all()


# ------------------------------------------------------------------ 9. plumbing
def check_repeatable(device):
    roster = random_roster().to(device)
    lob = torch.as_tensor(random_lobbies(5)[:333]).to(device)
    a, b = balance_lobbies(roster, lob, "ranked", cfg=CFG), balance_lobbies(roster, lob, "ranked", cfg=CFG)
    rec = torch.cat([a.records, a.records], 0)
    c, d = preview_matches(roster, rec, cfg=CFG), preview_matches(roster, rec, cfg=CFG)
    for x, y in zip(tuple(a) + tuple(c), tuple(b) + tuple(d)):
        assert x.dtype == y.dtype and np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)


def check_empty(device):
    roster = random_roster().to(device)
    i32 = dict(dtype=torch.int32, device=device)
    pv = preview_matches(roster, torch.empty((0, 8), **i32), cfg=CFG)
    assert pv.status.shape == pv.quality.shape == pv.p_win0.shape == (0,) and pv.status.dtype == torch.uint8
    bal = balance_lobbies(roster, torch.empty((0, 6), **i32), cfg=CFG)
    assert bal.records.shape == (0, 8) and bal.split.shape == (0,) and bal.quality.dtype == torch.float32
    made, left = make_lobbies(roster, torch.empty(0, **i32), K=2, cfg=CFG)
    assert made.records.shape == (0, 6) and left.shape == (0,) and left.dtype == torch.int32


def check_value_errors(device):
    roster = random_roster().to(device)
    lob = torch.as_tensor(random_lobbies(3)[:8]).to(device)
    rec = torch.zeros((4, 8), dtype=torch.int32, device=device)
    queue = torch.arange(20, dtype=torch.int32, device=device)
    other = "cpu" if str(device).startswith("cuda") else None
    bad = [
        lambda: balance_lobbies(roster, lob.to(torch.int64)),                 # dtype
        lambda: balance_lobbies(roster, lob[:, :5].contiguous()),             # odd width
        lambda: balance_lobbies(roster, torch.zeros((4, 12), dtype=torch.int32, device=device)),  # K = 6
        lambda: balance_lobbies(roster, lob.reshape(-1)),                     # shape
        lambda: balance_lobbies(roster, lob.t().contiguous().t()),            # non-contiguous
        lambda: balance_lobbies(roster, lob, mode="rankd"),                   # unknown mode
        lambda: balance_lobbies(roster, lob, mode="shared"),                  # shared is not a mode
        lambda: balance_lobbies(roster, lob, mode=2),
        lambda: balance_lobbies(roster.state.double(), lob),                  # roster dtype
        lambda: balance_lobbies(roster.state[:, :16].contiguous(), lob),      # roster shape
        lambda: balance_lobbies(torch.zeros((P, 64), device=device)[:, :32], lob),  # roster non-contiguous
        lambda: preview_matches(roster, rec.to(torch.int64)),
        lambda: preview_matches(roster, rec, K=2),                            # K against the width
        lambda: preview_matches(roster, rec, K=6),
        lambda: preview_matches(roster, rec[:, :7].contiguous()),
        lambda: preview_matches(roster, rec.t().contiguous().t()),
        lambda: make_lobbies(roster, queue, K=0),
        lambda: make_lobbies(roster, queue, K=6),
        lambda: make_lobbies(roster, queue.reshape(4, 5)),
        lambda: make_lobbies(roster, queue.to(torch.int64)),
        lambda: make_lobbies(roster, queue[::2]),
        lambda: make_lobbies(roster, queue, mode="trueskill"),
    ]
    if other is not None:  # device mismatches
        bad += [lambda: balance_lobbies(roster, lob.to(other)), lambda: preview_matches(roster.to(other), rec),
                lambda: make_lobbies(Roster(roster.state, roster.attrs.to(other)), queue)]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("call %d raised nothing" % k)


def check_cli(device, capsys):
    """The re-rate command line's matchmaking line against make_lobbies on the same run's roster."""
    from analyzer_amd.runtime import rerate

    args = ["--matches", "3000", "--players", "300", "--window", "1000", "--device", str(device),
            "--matchmake", "ranked:3:100"]
    assert rerate.main(args) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and "matchmake" not in lines[0]
    line = lines[1]
    spec = rerate.RerateSpec(total_matches=3000, players=300, window=1000)
    _, roster = rerate.run(spec, device)
    queue = torch.randperm(300, generator=torch.Generator().manual_seed(spec.seed))[:100].to(torch.int32)
    bal, left = make_lobbies(roster, queue.to(roster.device), mode="ranked", K=3)
    ok = (bal.status == 0).cpu().numpy()
    q, qg = bal.quality.cpu().numpy()[ok].astype(np.float64), bal.quality_given.cpu().numpy()[ok].astype(np.float64)
    assert line["matchmake"] == "ranked" and line["team_size"] == 3 and line["queue"] == 100
    assert line["lobbies"] == len(ok) == 16 and line["balanced"] == int(ok.sum()) and line["unmatched"] == left.numel() == 4
    assert line["quality_mean"] == pytest.approx(q.mean(), rel=1e-12) and line["quality_min"] == q.min()
    assert line["quality_given_mean"] == pytest.approx(qg.mean(), rel=1e-12) and line["quality_given_min"] == qg.min()
    off = np.abs(bal.p_win0.cpu().numpy()[ok].astype(np.float64) - 0.5).mean()
    assert line["p_off_mean"] == pytest.approx(off, rel=1e-12)
    assert line["p_off_mean"] <= line["p_off_given_mean"] and line["quality_mean"] >= line["quality_given_mean"]
    # without --matchmake the output is the one result line, as before
    assert rerate.main(args[:8]) == 0
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]) == 1
