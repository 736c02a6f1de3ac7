"""Shared cases of the scorecard tests (test_scorecard.py on the CPU, test_scorecard_gpu.py
on the device): plain Python oracles written from the definitions in the module docstring of
ops/scorecard.py (not from csrc/score_core.h), the windows they are checked on, and the checks
that run the same way on either device.

Oracles: ``priors_ref`` -- a sequential loop over (chain, rec, rows) for the priors and the
final chain; ``table_ref`` -- plain ``int`` arithmetic for the bins and the sums, fed from the
pred rows of the code under test; ``analyzer_amd.ops.scorecard.nlog2_q20`` is itself the
plain-``int`` form of the integer log and is checked against mpmath here."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from analyzer_amd.config import MODES, RaterConfig
from analyzer_amd.models.match_rater import make_env
from analyzer_amd.ops import Scorecard, match_priors, preview_matches
from analyzer_amd.ops import scorecard as SC
from analyzer_amd.ops.native import native
from analyzer_amd.ops.rate import BatchRater, RateResult, Roster
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream, play_out

import matchmake_cases as MC
import records_cases as RC

TILE = 4096  # sorted elements per workgroup of the scan (csrc/kernels.h kPriorTile; checked below)
NANBITS = 0x7FC00000
RATED = 0
CFG = RaterConfig()
ALL_MODES = {m: 1.0 for m in MODES}
KS = (1, 2, 3, 4, 5)


def check_constants():
    assert int(native().PRIOR_TILE) == TILE and int(native().SCORE_BINS) == 32


def u32(t):
    """The words of a tensor as a numpy uint32 array."""
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


# ------------------------------------------------------------------ the priors oracle
def priors_ref(chain, rec, rows):
    """(priors [M, 4, 2K], chain after) as uint32 words, from chain [P, 16], rec [M, 2K+2]
    and packed rows [M, W]: the definition, one match after the other."""
    ch = u32(chain).copy()
    r = rec.cpu().numpy().astype(np.int64)
    w = u32(rows)
    P, (M, cols) = ch.shape[0], r.shape
    S = cols - 2
    K = S // 2
    pri = np.full((M, 4, S), NANBITS, dtype=np.uint32)
    for m in range(M):
        mode, n0, n1 = r[m, S] & 0xFF, (r[m, S] >> 8) & 0xFF, (r[m, S] >> 16) & 0xFF
        if mode >= 6:
            continue
        live = [j for j in range(S) if (j if j < K else j - K) < (n0 if j < K else n1) and 0 <= r[m, j] < P]
        for j in live:
            p = r[m, j]
            pri[m, :, j] = ch[p, 0], ch[p, 1], ch[p, 2 + 2 * mode], ch[p, 3 + 2 * mode]
        if (w[m, 5 * S + 1] & 0xFF) != RATED:
            continue
        for j in live:
            p = r[m, j]
            if any(r[m, i] == p for i in live if i > j):
                continue  # later writes win: the earlier twin's write is never seen
            ch[p, 0], ch[p, 1] = w[m, j], w[m, S + j]
            ch[p, 2 + 2 * mode], ch[p, 3 + 2 * mode] = w[m, 3 * S + j], w[m, 4 * S + j]
    return pri, ch


# ------------------------------------------------------------------ windows
def synthetic(K, M, P, seed, live=None, other=0.15, ids=None, chain_p=None):
    """(chain, rec, rows): M matches of random players of [0, P) on all six modes, random row
    words (distinct, so a wrong source shows; NaNs among them), ``other``: the share of rows
    that are not rated.  ``live``: slots of the last matches are emptied until exactly that
    many are occupied.  ``ids`` [M, 2K] overrides the players.  The chain starts from random
    words with NULL tracks among them."""
    rng = np.random.default_rng(seed)
    S, W = 2 * K, RateResult.row_floats(K)
    rec = np.zeros((M, S + 2), dtype=np.int64)
    rec[:, :S] = rng.integers(0, P, (M, S)) if ids is None else ids
    free = 0 if live is None else M * S - live
    n = np.full((M, 2), K)
    for m in reversed(range(M)):
        drop = min(free, S - 1)
        free -= drop
        n[m, 1] -= min(drop, K)
        n[m, 0] -= drop - min(drop, K)
    rec[:, S] = rng.integers(0, 6, M) | (n[:, 0] << 8) | (n[:, 1] << 16) | (2 << 24)
    rec[:, S + 1] = rng.integers(0, 4, M)
    rows = rng.integers(0x3F000000, 0x45000000, (M, W)).astype(np.uint32)  # floats in 0.5 .. 2048
    rows[rng.random((M, W)) < 0.03] = NANBITS
    st = np.where(rng.random(M) < other, rng.choice([1, 2, 3, 7, 255], M), RATED).astype(np.uint32)
    rows[:, 5 * S + 1] = st | 0x5A5A00  # only the low byte is the status
    cp = P if chain_p is None else chain_p
    chain = rng.integers(0x3F000000, 0x45000000, (cp, 16)).astype(np.uint32)
    chain[rng.random((cp, 16)) < 0.2] = NANBITS
    as_f = lambda a: torch.from_numpy(a.view(np.int32).copy()).view(torch.float32)  # noqa: E731
    return as_f(chain), torch.from_numpy(rec.astype(np.int32)), as_f(rows)


FEW_P, FEW_M = 12, 200
FEW_SPEC = dict(p_afk=0.05, p_unsupported=0.5, p_uneven=0.1, p_bad_rosters=0.04, p_tie=0.08)


@functools.lru_cache(maxsize=None)
def few(K):
    """(roster before, rec, rows, roster after): P = 12, M = 200, every record feature on --
    AFK, invalid rosters, unsupported mode, uneven rosters, ties, a player twice in a match,
    all six modes -- over a roster with NULL shared and NULL mode tracks, rated by the host
    mirror once."""
    roster = make_roster(RosterSpec(num_players=FEW_P, seed=40 + K, p_rated=0.5, p_mode_rated=0.5))
    rec = make_stream(StreamSpec(team_size=K, seed=50 + K, modes=ALL_MODES, **FEW_SPEC), FEW_M, FEW_P, K=K)
    r = rec.numpy()
    assert len(set(r[:, 2 * K] & 0xFF)) == 7, "six modes and the unsupported one"
    assert K == 1 or any(len(set(row[:2 * K])) < 2 * K for row in r), "a player twice in a match"
    before = roster.clone()
    assert bool(torch.isnan(before.state[:, 0]).any()) and bool(torch.isnan(before.state[:, 4::4]).any())
    res = BatchRater(CFG).rate(roster, rec, K)
    st = set(res.status.tolist())
    assert {0, 1, 2, 3} <= st, st
    return before, rec, res.packed, roster


@functools.lru_cache(maxsize=None)
def case(name):
    """(chain, rec, rows) of a named case, built once and never modified."""
    kind, _, arg = name.partition(":")
    if kind == "few":
        before, rec, rows, _ = few(int(arg))
        return SC.chain_of(before.state), rec, rows
    if kind == "tile":  # tile:K:slots -- live slots just below / at / above one tile and above two
        K, live = (int(x) for x in arg.split(":"))
        M = -(-live // (2 * K))
        chain, rec, rows = synthetic(K, M, 37, seed=K * 10007 + live, live=live)
        keys = np.sort(live_keys(rec, 37))
        assert len(keys) == live
        for edge in range(TILE, live, TILE):  # a player's run straddles every tile edge
            assert keys[edge - 1] == keys[edge], (name, edge)
        return chain, rec, rows
    if kind == "stitch":  # 129 tiles, 258 edges: the stitch kernel runs a second iteration
        chain, rec, rows = synthetic(5, 52_429, 37, seed=99)
        keys = np.sort(live_keys(rec, 37))
        assert len(keys) == 524_290 and 2 * -(-len(keys) // TILE) == 258
        # edge 255 ends tile 127, edge 256 begins tile 128: one player's run crosses the iterations
        assert keys[128 * TILE - 1] == keys[128 * TILE]
        return chain, rec, rows
    if kind == "every":  # one player in every match across three tiles: a whole tile is one key
        M = 3 * TILE + 5
        ids = np.stack([np.zeros(M, dtype=np.int64), 1 + np.arange(M) % 5], axis=1)
        return synthetic(1, M, 6, seed=3, ids=ids)
    if kind == "alternate":  # two players, both in every match, swapping sides
        M = TILE + TILE // 2
        ids = np.stack([np.arange(M) % 2, (np.arange(M) + 1) % 2], axis=1)
        return synthetic(1, M, 2, seed=4, ids=ids, other=0.3)
    if kind == "twins":  # one player in both slots of every match: only the later twin writes
        M = TILE + 9
        return synthetic(1, M, 1, seed=5, ids=np.zeros((M, 2), dtype=np.int64))
    if kind == "sparse":  # P = 2^20, about 50 active players, ids out of range in occupied slots
        P, M, K = 1 << 20, 400, 3
        rng = np.random.default_rng(6)
        active = rng.choice(P, 50, replace=False)
        ids = active[rng.integers(0, 50, (M, 2 * K))]
        outside = rng.random((M, 2 * K)) < 0.05
        ids[outside] = rng.choice([-1, P, P + 5, 2 ** 31 - 1, -7], int(outside.sum()))
        return synthetic(K, M, P, seed=7, ids=ids)
    if kind == "split":
        return synthetic(2, 60, 7, seed=8, other=0.2)
    raise KeyError(name)


def live_keys(rec, P):
    """The players of the live slots of ``rec``, in slot order."""
    r = rec.numpy().astype(np.int64)
    S = r.shape[1] - 2
    K = S // 2
    out = []
    for row in r:
        mode, n0, n1 = row[S] & 0xFF, (row[S] >> 8) & 0xFF, (row[S] >> 16) & 0xFF
        if mode < 6:
            out += [row[j] for j in range(S) if (j if j < K else j - K) < (n0 if j < K else n1) and 0 <= row[j] < P]
    return np.array(out, dtype=np.int64)


FEW_CASES = ["few:%d" % K for K in KS]
TILE_CASES = ["tile:%d:%d" % (K, n) for K in KS for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]
LONG_CASES = ["every", "alternate", "twins"]
DEVICE_LONG_CASES = LONG_CASES + ["stitch"]  # 524,290 slots: the oracle alone takes seconds, so on the device only
OTHER_CASES = ["sparse", "split"]


@functools.lru_cache(maxsize=None)
def expected(name):
    return priors_ref(*case(name))


def run_priors(name, device, cuts=(), max_slots=None):
    """(priors words [M, 4, 2K], chain words) of a case on ``device``, the window in one piece
    or cut at ``cuts``."""
    chain, rec, rows = case(name)
    chain = chain.clone().to(device)
    edges = [0, *cuts, rec.shape[0]]
    parts = [match_priors(chain, rec[a:b].to(device), rows[a:b].to(device), max_slots=max_slots)
             for a, b in zip(edges[:-1], edges[1:])]
    assert all(p.device.type == torch.device(device).type for p in parts)
    return u32(torch.cat(parts)), u32(chain)


def check_priors(name, device):
    """Priors and final chain against the oracle, bit for bit (a NaN by its bit pattern)."""
    pri, ch = run_priors(name, device)
    want_pri, want_ch = expected(name)
    bad = np.argwhere(pri != want_pri)[:5]
    assert np.array_equal(pri, want_pri), (name, bad.tolist(), [hex(pri[tuple(b)]) for b in bad],
                                           [hex(want_pri[tuple(b)]) for b in bad])
    assert np.array_equal(ch, want_ch), (name, np.argwhere(ch != want_ch)[:5].tolist())
    return pri, ch


def check_sparse(device):
    """Out-of-range ids touch no chain row and get NaN priors; most of the 2^20 rows stay."""
    chain, rec, rows = case("sparse")
    pri, ch = check_priors("sparse", device)
    P, S = chain.shape[0], rec.shape[1] - 2
    ids = rec.numpy()[:, :S]
    out = (ids < 0) | (ids >= P)
    assert out.sum() > 50 and (pri.transpose(0, 2, 1)[out] == NANBITS).all()
    assert (ch != u32(chain)).any(axis=1).sum() <= 50
    # the rows next to the table are never touched
    big = torch.full((P + 2, 16), 12345.0, device=device)
    big[1:P + 1] = chain.to(device)
    match_priors(big[1:P + 1], rec.to(device), rows.to(device))
    assert np.array_equal(u32(big[1:P + 1]), ch)
    assert bool((big[0] == 12345.0).all()) and bool((big[P + 1] == 12345.0).all())


def check_empty(device):
    chain, rec, rows = case("split")
    c = chain.clone().to(device)
    out = match_priors(c, rec[:0].to(device), rows[:0].to(device))
    assert tuple(out.shape) == (0, 4, 4) and np.array_equal(u32(c), u32(chain))
    card = Scorecard(Roster.empty(4).to(device), cfg=CFG)
    pred = card.add(rec[:0].to(device), rows[:0].to(device), keep=True)
    assert pred.status.numel() == 0 and int(card.table.abs().sum()) == 0


# ------------------------------------------------------------------ 2. the chain is the roster
def check_chain_is_roster(K, device):
    """Three windows of 2,000 matches over 150 players, rated by ``BatchRater`` on ``device``:
    after every ``add`` the chain equals the roster's (mu, sigma) on all seven tracks."""
    P, M = 150, 2000
    roster = make_roster(RosterSpec(num_players=P, seed=60 + K), device=device)
    card = Scorecard(roster, cfg=CFG)
    rater = BatchRater(CFG)
    spec = StreamSpec(team_size=K, seed=70 + K, modes=ALL_MODES, **FEW_SPEC)
    statuses = set()
    for g in range(3):
        rec = make_stream(spec, M, P, K=K, base=g * M, device=device)
        res = rater.rate(roster, rec, K)
        card.add(rec, res.packed)
        want = u32(SC.chain_of(roster.state))[:, :14]
        got = u32(card.chain)[:, :14]
        assert np.array_equal(got, want), (K, g, np.argwhere(got != want)[:5].tolist())
        statuses |= set(res.status.cpu().tolist())
    assert {0, 1, 2, 3} <= statuses  # statuses other than rated ran, and wrote nothing
    summ = card.summary()
    assert summ["inconsistent"] == 0 and summ["n"] > 3000 and summ["ties"] > 100, summ
    return card


# ------------------------------------------------------------------ 3. first appearances equal the preview
@functools.lru_cache(maxsize=None)
def first_window(K):
    """(roster, rec, rows): M = 300 matches in which no player occurs twice (P = 2K M), NULL
    tracks, seeds that fail, sigma errors and every early status included; rows as the host
    mirror rates them."""
    M = 300
    P = 2 * K * M
    roster = make_roster(RosterSpec(num_players=P, seed=80 + K, p_tier_bad=0.02, p_tier_null=0.02, p_rp_ranked=0.2,
                                    p_rp_blitz=0.1))
    rng = np.random.default_rng(81 + K)
    zero = rng.choice(P, 12, replace=False)
    roster.state[zero[:6], 2] = 0.0    # sigma errors on the shared and on a mode track
    roster.state[zero[6:], 4 * 2 + 2] = 0.0
    rec = make_stream(StreamSpec(team_size=K, seed=82 + K, modes=ALL_MODES, **FEW_SPEC), M, P, K=K)
    rec[:, :2 * K] = torch.from_numpy(rng.permutation(P).reshape(M, 2 * K).astype(np.int32))
    rec[5, 0], rec[9, 2 * K - 1] = P, -1       # malformed records
    rec[11, 2 * K] = (rec[11, 2 * K] & ~0xFF00)  # an empty roster
    before = roster.clone()
    res = BatchRater(CFG).rate(roster, rec, K)
    assert len(set(res.status.tolist())) >= 7, set(res.status.tolist())
    return before, rec, res.packed


def check_first_appearances(K, device):
    roster, rec, rows = first_window(K)
    roster, rec, rows = roster.clone().to(device), rec.to(device), rows.to(device)
    pv = preview_matches(roster, rec, cfg=CFG)
    pred = Scorecard(roster, cfg=CFG).add(rec, rows, keep=True)
    assert torch.equal(pred.status, pv.status)
    assert np.array_equal(u32(pred.p_win0), u32(pv.p_win0))
    assert int((pv.status == 0).sum()) > 150 and int((pv.status >= 4).sum()) > 5
    # the rows were rated from this roster: whatever was rated is consistent
    rated = u32(rows)[:, 10 * K + 1] & 0xFF == RATED
    assert (pred.status.cpu().numpy()[rated] == RATED).all()


# ------------------------------------------------------------------ resolved priors, 4. and 5.
def resolved(K, pri, rec, attrs, m):
    """(status, ms, ss, mm, sm) per slot of match m: the prior words through the seeding and
    fall-back rules (``matchmake_cases.np_priors``, fp32)."""
    S = 2 * K
    r = rec.numpy()
    mode = int(r[m, S]) & 0xFF
    fake = np.full((attrs.shape[0], 32), np.nan, dtype=np.float32)
    f = pri[m].view(np.float32)
    slots = [j for j in range(S) if (j if j < K else j - K) < ((r[m, S] >> 8) & 0xFF if j < K else (r[m, S] >> 16) & 0xFF)]
    for j in slots:
        p = r[m, j]
        fake[p, 0], fake[p, 2], fake[p, 4 * (1 + mode)], fake[p, 4 * (1 + mode) + 2] = f[:, j]
    return slots, MC.np_priors(fake, attrs.numpy(), [int(r[m, j]) for j in slots], mode)


def check_closing_the_loop(K, device, rtol=2e-6, atol=2e-3):
    """On ``few``: each rated match's resolved priors through the fp64 closed form of
    ``models/`` reproduce the row's post-state, within the tolerance of the single-match
    parity test of the host mirror (tests/test_engine_host.py: rtol 2e-6, atol 2e-3), whose
    rows these are."""
    before, rec, rows, _ = few(K)
    pri, _ = run_priors("few:%d" % K, device)
    env = make_env(CFG)
    S = 2 * K
    w = rows.numpy()
    r = rec.numpy()
    done = 0
    for m in range(rec.shape[0]):
        if u32(rows)[m, 5 * S + 1] & 0xFF != RATED:
            continue
        slots, (st, ms, ss, mm, sm) = resolved(K, pri, rec, before.attrs, m)
        assert (st == 0).all()
        a = [i for i, j in enumerate(slots) if j < K]
        b = [i for i, j in enumerate(slots) if j >= K]
        ranks = (0 if r[m, S + 1] & 1 else 1, 0 if r[m, S + 1] & 2 else 1)
        for mu, sg, f_mu, f_sg in ((ms, ss, 0, 1), (mm, sm, 3, 4)):
            na, nb = env.rate_two_teams([(float(mu[i]), float(sg[i])) for i in a],
                                        [(float(mu[i]), float(sg[i])) for i in b], *ranks)
            for i, (nmu, nsg) in zip(a + b, na + nb):
                j = slots[i]
                np.testing.assert_allclose(w[m, f_mu * S + j], nmu, rtol=rtol, atol=atol, err_msg=str((m, j)))
                np.testing.assert_allclose(w[m, f_sg * S + j], nsg, rtol=rtol, atol=atol, err_msg=str((m, j)))
        done += 1
    assert done > 100


@functools.lru_cache(maxsize=None)
def tail_window():
    """(roster, rec, rows): K = 1 and 3, fully rated rosters so the prior words are the priors;
    upsets up to |t| > 8, so p_outcome goes below 2^-40."""
    out = {}
    for K in (1, 3):
        S = 2 * K
        M = 64
        roster = Roster.empty(S * M)
        rng = np.random.default_rng(90 + K)
        gap = np.repeat(np.linspace(0.0, 14000.0 / K, M), S).reshape(M, S)
        gap[:, K:] = 0.0
        mu = (1500.0 + gap + rng.uniform(-50, 50, (M, S))).astype(np.float32).reshape(-1)
        for g in range(7):
            MC.set_track(roster, g, mu + 3 * g, rng.uniform(40.0, 300.0, S * M).astype(np.float32))
        rec = np.zeros((M, S + 2), dtype=np.int32)
        rec[:, :S] = np.arange(S * M).reshape(M, S)
        rec[:, S] = (np.arange(M) % 6) | (K << 8) | (K << 16) | (2 << 24)
        rec[:, S + 1] = 1 + (np.arange(M) % 2)  # the favourite wins, then the underdog
        rows = torch.zeros((M, RateResult.row_floats(K)))  # status byte 0: rated
        out[K] = (roster, torch.from_numpy(rec), rows)
    return out


def check_p_against_mpmath(device):
    """p_win0 and p_outcome against Phi at 50 digits from the same fp32 priors, within the
    budget B_p that matchmake_cases.mp_match derives for p_win0 (for p_outcome of a win of
    roster 1 the same derivation with the signs swapped)."""
    lowest = 1.0
    for K, (roster, rec, rows) in tail_window().items():
        S = 2 * K
        card = Scorecard(roster.clone().to(device), cfg=CFG)
        pred = card.add(rec.to(device), rows.to(device), keep=True)
        assert bool(pred.scored.all())
        state = roster.state.numpy()
        pw, po = pred.p_win0.cpu().numpy().astype(np.float64), pred.p_outcome.cpu().numpy().astype(np.float64)
        for m in range(rec.shape[0]):
            ids = rec[m, :S].tolist()
            g = 4 * (1 + (int(rec[m, S]) & 0xFF))
            mu, sg = state[ids, g], state[ids, g + 2]
            signs = [1 if j < K else -1 for j in range(S)]
            a = MC.mp_match(mu, sg, signs, S - 1)
            assert abs(pw[m] - a["p"]) <= a["B_p"], (K, m, pw[m], a["p"], a["B_p"])
            if int(rec[m, S + 1]) & 3 == 2:
                a = MC.mp_match(mu, sg, [-s for s in signs], S - 1)
            assert abs(po[m] - a["p"]) <= a["B_p"], (K, m, po[m], a["p"], a["B_p"])
            lowest = min(lowest, po[m])
    assert 0 < lowest < 2.0 ** -40, lowest


# ------------------------------------------------------------------ 6. the integer log
def log_patterns():
    """fp32 bit patterns: p = 1, 0.5 and its neighbours, the smallest normal, a denormal, 0,
    and 4,096 random patterns in (0, 1]."""
    rng = np.random.default_rng(11)
    half = np.float32(0.5)
    named = np.array([1.0, 0.5, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)),
                      np.float32(2.0 ** -126)], dtype=np.float32).view(np.uint32)
    named = np.concatenate([named, np.array([0x00000123, 0], dtype=np.uint32)])
    rand = rng.integers(0x00800000, 0x3F800001, 4096).astype(np.uint32)
    return np.concatenate([named, rand])


def check_integer_log(device):
    bits = log_patterns()
    got = native().nlog2_q20(torch.from_numpy(bits.view(np.int32).copy()).to(device)).cpu().tolist()
    want = [SC.nlog2_q20(int(b)) for b in bits]
    assert got == want
    assert want[0] == 0 and want[1] == 1 << 20 and want[4] == 126 << 20
    assert want[5] == want[6] == SC.NLOG2_CAP == int(native().NLOG2_CAP)
    assert want[2] > want[1] >= want[3]  # the result rounds up: the upper neighbour of 0.5 is within one unit


def integer_log_error():
    """(min, max) of nlog2_q20(p) - (-log2 p) 2^20 over the random patterns, in units of 2^-20."""
    mp = MC._mp()
    errs = []
    for b in log_patterns()[7:]:
        p = mp.mpf(float(np.array([b], dtype=np.uint32).view(np.float32)[0]))
        errs.append(SC.nlog2_q20(int(b)) - (-mp.log(p, 2) * (1 << 20)))
    return float(min(errs)), float(max(errs))


# ------------------------------------------------------------------ 7. the table oracle
def table_ref(pred, rec, rows, modes=None):
    """The int64 table [6, 33, 4] as Python ints from the pred rows of the code under test."""
    allowed = set(range(6)) if modes is None else {MODES.index(m) for m in modes}
    flags = pred.flags.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    pw_bits, po_bits = u32(pred.p_win0), u32(pred.p_outcome)
    pw = pw_bits.view(np.float32)
    po = po_bits.view(np.float32)
    r = rec.cpu().numpy().astype(np.int64)
    S = r.shape[1] - 2
    st = u32(rows)[:, 5 * S + 1] & 0xFF
    t = [[[0] * 4 for _ in range(33)] for _ in range(6)]
    for m in range(r.shape[0]):
        mode, w0, w1 = int(r[m, S] & 0xFF), bool(r[m, S + 1] & 1), bool(r[m, S + 1] & 2)
        scored = False
        if st[m] == RATED and mode in allowed:
            if (flags[m] & 0xFF) != RATED or not np.isfinite(pw[m]):
                t[mode][SC.SPARE_INCONSISTENT][3] += 1
                assert flags[m] & SC.FLAG_INCONSISTENT
            elif not w0 and not w1:
                t[mode][32][3] += 1
                assert flags[m] & SC.FLAG_TIE
            elif w0 != w1:
                scored = True
                p = Fraction(float(pw[m]))
                b = min(31, int(p * 32))
                assert (flags[m] >> 16) & 0xFF == b
                t[mode][b][0] += 1
                t[mode][b][1] += int(w0)
                t[mode][b][2] += int(round(p * (1 << 24)))  # exact product, ties to even
                e = float(pw[m]) - (1.0 if w0 else 0.0)     # IEEE fp64, operation by operation
                t[mode][32][0] += int(round(e * e * 16777216.0))
                t[mode][32][1] += SC.nlog2_q20(int(po_bits[m]))
                t[mode][32][2] += int(po[m] > 0.5)
                t[mode][SC.SPARE_COIN][3] += int(po[m] == 0.5)
        assert bool(flags[m] & SC.FLAG_SCORED) == scored == bool(pred.scored[m])
    return t


def check_table(K, device, modes=None, track="mode"):
    """On ``few``: every word of the table from the device's own pred rows; ties counted."""
    before, rec, rows, _ = few(K)
    card = Scorecard(before.clone().to(device), track=track, modes=modes, cfg=CFG)
    pred = card.add(rec.to(device), rows.to(device), keep=True)
    assert card.table.dtype == torch.int64 and card.table.device.type == torch.device(device).type
    want = table_ref(pred, rec, rows, modes)
    assert card.table.cpu().tolist() == want
    summ = card.summary()
    assert summ["inconsistent"] == 0 and summ["ties"] > 0 and summ["n"] > 50
    assert summ["n"] == int(pred.scored.sum()) and 0.0 <= summ["ece"] <= 1.0
    return card, pred


def check_coin(device):
    """Equal priors on both sides: p_win0 = p_outcome = 0.5 exactly, counted as coins, one bit
    each, the favourite never 'won'."""
    M, K = 40, 1
    roster = Roster.empty(2 * M)
    for g in range(7):
        MC.set_track(roster, g, np.full(2 * M, 1500.0), np.full(2 * M, 200.0))
    rec = torch.zeros((M, 4), dtype=torch.int32)
    rec[:, :2] = torch.arange(2 * M).reshape(M, 2)
    rec[:, 2] = 1 | (1 << 8) | (1 << 16) | (2 << 24)
    rec[:, 3] = 1 + (torch.arange(M) % 2)
    rows = torch.zeros((M, RateResult.row_floats(K)))
    card = Scorecard(roster.to(device), cfg=CFG)
    pred = card.add(rec.to(device), rows.to(device), keep=True)
    assert card.table.cpu().tolist() == table_ref(pred, rec, rows)
    s = card.summary()
    assert (s["n"], s["coin"], s["accuracy"], s["bits"], s["brier"]) == (M, M, 0.0, 1.0, 0.25)
    assert s["bins"] == [{"bin": 16, "n": M, "mean_p": 0.5, "win_rate": 0.5}] and s["ece"] == 0.0


def check_wrong_roster(K, device):
    """An empty starting roster where the history had rated players: inconsistent > 0, no
    exception (the empty roster has no attributes to seed from)."""
    before, rec, rows, _ = few(K)
    card = Scorecard(Roster.empty(FEW_P).state.to(device), cfg=CFG)
    pred = card.add(rec.to(device), rows.to(device), keep=True)
    assert card.table.cpu().tolist() == table_ref(pred, rec, rows)
    assert card.summary()["inconsistent"] > 0


# ------------------------------------------------------------------ 8. invariance
def check_invariance(device):
    """One window whole or cut at arbitrary points: the same priors, chain and table bits;
    twice the same; chunks above a lowered slot limit."""
    chain, rec, rows = case("split")
    M = rec.shape[0]
    one = run_priors("split", device)
    assert np.array_equal(one[0], expected("split")[0])
    for cuts in ((1,), (17,), (M - 1,), (1, 2), (9, 40), (1, 30, M - 1)):
        got = run_priors("split", device, cuts)
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]), cuts
    got = run_priors("split", device, max_slots=4 * 7 + 1)  # chunks of 7 matches
    assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])
    for K in (2, 5):
        before, rec, rows, _ = few(K)
        tables = []
        for cuts in ((), (), (1, 50), (199,), "chunks"):
            card = Scorecard(before.clone().to(device), cfg=CFG)
            if cuts == "chunks":
                card.max_slots = 2 * K * 30 + 3  # ``add`` splits the window into chunks of 30 matches
                cuts = ()
            edges = [0, *cuts, rec.shape[0]]
            preds = [card.add(rec[a:b].to(device), rows[a:b].to(device), keep=True) for a, b in zip(edges[:-1], edges[1:])]
            tables.append((card.table.cpu(), u32(card.chain), np.concatenate([u32(p.p_win0) for p in preds]),
                           np.concatenate([u32(p.p_outcome) for p in preds])))
        for t in tables[1:]:
            assert torch.equal(t[0], tables[0][0]) and all(np.array_equal(x, y) for x, y in zip(t[1:], tables[0][1:]))


# ------------------------------------------------------------------ 9. it means something
def latent_history(players=300, matches=20000, seed=5):
    """(roster before, rec): a 3v3 history whose winners are played out from latent skills."""
    K = 3
    roster = make_roster(RosterSpec(num_players=players, seed=seed))
    g = torch.Generator().manual_seed(seed)
    skill = 1500.0 + 1000.0 * torch.randn(players, generator=g, dtype=torch.float64)
    rec = make_stream(StreamSpec(team_size=K, seed=seed + 1), matches, players, K=K)
    return roster, play_out(rec, skill, float(CFG.beta), seed + 2)


# ------------------------------------------------------------------ 10. arena
def check_arena(spec, device):
    """``RecordArena.scorecard`` equals window-by-window ``add``."""
    from analyzer_amd.runtime.rerate import rerate_resident, start_roster, stream_records

    roster0 = start_roster(spec, None, torch.device(device))
    _, roster, arena = rerate_resident(spec, device, free_bytes=RC.FREE)
    rec_of = stream_records(spec, device)
    card = arena.scorecard(roster0, rec_of, cfg=CFG)
    want = Scorecard(roster0, cfg=CFG)
    for lo, hi in arena.windows():
        want.add(rec_of(lo, hi), arena.result(lo, hi).packed)
    assert torch.equal(card.table, want.table) and int(card.table[:, :32, 0].sum()) > spec.total_matches // 2
    assert np.array_equal(u32(card.chain)[:, :14], u32(SC.chain_of(roster.state))[:, :14])
    assert card.summary()["inconsistent"] == 0
    return arena, card
