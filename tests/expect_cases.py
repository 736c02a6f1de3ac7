"""Shared cases of the expectation tests (test_expectations.py on the CPU,
test_expectations_gpu.py on the device): an oracle of the K19 player table in numpy int64 and
plain Python ints, written from the definitions in the module docstring of
ops/expectations.py (nothing of csrc/expect_core.h; ``ops.scorecard.nlog2_q20`` is the plain
``int`` form of the integer log), the windows it is checked on, and the checks that run the
same way on either device.

Every check is ``torch.equal`` on the whole player table and ``==`` on the bad counter."""
import functools
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import torch

from analyzer_amd.config import MODES, RaterConfig
from analyzer_amd.ops import Expectations, Scorecard
from analyzer_amd.ops import expectations as EX
from analyzer_amd.ops.native import native
from analyzer_amd.ops.rate import AFK, RATED, BatchRater
from analyzer_amd.ops.scorecard import FLAG_INCONSISTENT, FLAG_SCORED, FLAG_TEAM0_WON, FLAG_TIE, nlog2_q20
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096  # sorted elements per workgroup of the fold (csrc/kernels.h kExpectTile; checked below)
NAN, INF = float("nan"), float("inf")
ONE, HALF = 1 << 24, 1 << 23
TWO20 = float(2 ** 20)
ABOVE_TWO20 = float(np.nextafter(np.float32(2 ** 20), np.float32(INF)))
CFG = RaterConfig()
WORDS = 24


def check_tile():
    assert int(native().EXPECT_TILE) == TILE and int(native().EXPECT_WORDS) == WORDS == EX.WORDS


def bits_of(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


# ------------------------------------------------------------------ the oracle
@functools.lru_cache(maxsize=None)
def _nlog2(bits):
    return nlog2_q20(bits)


def expect_terms(rec, priors, pred, P, track="mode"):
    """Per slot, int64 / bool arrays [M, 2K] of one window: game, ids, won, q24, var, surprise,
    known, t, mates, mate_slots, opp, opp_slots and the bad count."""
    r = rec.cpu().numpy().astype(np.int64)
    M, S = r.shape[0], r.shape[1] - 2
    K = S // 2
    ids = r[:, :S]
    m0, m1 = r[:, S] & 0xFFFFFFFF, r[:, S + 1] & 0xFFFFFFFF
    mode, n0, n1 = m0 & 0xFF, (m0 >> 8) & 0xFF, (m0 >> 16) & 0xFF
    j = np.arange(S)
    team1 = j >= K
    occupied = np.where(team1, j - K, j)[None, :] < np.where(team1[None, :], n1[:, None], n0[:, None])
    live = occupied & (ids >= 0) & (ids < P) & (mode < len(MODES))[:, None]
    pw = pred.cpu().numpy().view(np.uint32).reshape(M, 4)
    pri = priors.cpu().contiguous().numpy().reshape(M, 4, S)
    with np.errstate(invalid="ignore", over="ignore"):
        p = pw[:, 1].copy().view(np.float32)
        scored = ((pw[:, 0] & FLAG_SCORED) != 0) & (p >= 0) & (p <= 1)
        game = live & scored[:, None]
        p24 = np.rint(np.where(scored, p, 0).astype(np.float64) * ONE).astype(np.int64)  # exact product
        q = np.where(team1[None, :], ONE - p24[:, None], p24[:, None])
        var = (q * (ONE - q)) >> 16
        surprise = np.array([_nlog2(int(b)) for b in pw[:, 2]], dtype=np.int64).reshape(M, 1) + 0 * q
        w0, w2 = pri[:, 0, :], pri[:, 2, :]
        raw = w0 if track == "shared" else np.where(np.isnan(w2), w0, w2)
        off = np.isinf(raw) | (np.abs(raw) > np.float32(TWO20))
        known = game & ~np.isnan(raw) & ~off
        t = np.where(known, np.rint(np.where(known, raw, 0).astype(np.float64) * 256), 0).astype(np.int64)
    bad = int((game & off).sum())
    k64 = known.astype(np.int64)
    team_sum = np.stack([t[:, :K].sum(axis=1), t[:, K:].sum(axis=1)], axis=1)  # [M, 2]
    team_cnt = np.stack([k64[:, :K].sum(axis=1), k64[:, K:].sum(axis=1)], axis=1)
    me = team1.astype(np.int64)
    won = np.where(team1[None, :], (m1[:, None] >> 1) & 1, m1[:, None] & 1).astype(bool)
    return dict(game=game, ids=ids, won=won, q=q, var=var, surprise=surprise, known=known, t=t,
                mates=team_sum[:, me] - t, mate_slots=team_cnt[:, me] - k64, opp=team_sum[:, 1 - me],
                opp_slots=team_cnt[:, 1 - me], bad=bad)


def expect_ref(rec, priors, pred, P, track="mode"):
    """(player table [P, 24] int32, bad) of one window."""
    x = expect_terms(rec, priors, pred, P, track)
    g, won = x["game"], x["won"]
    who = x["ids"][g]
    fav, dog = x["q"] > HALF, x["q"] < HALF
    cols = [np.ones_like(x["q"]), won, fav, fav & won, dog, dog & won, x["known"], 0 * x["q"],
            x["q"], x["var"], x["surprise"], x["t"], x["mates"], x["mate_slots"], x["opp"], x["opp_slots"]]
    acc = np.zeros((P, 16), np.int64)
    np.add.at(acc, who, np.stack([np.asarray(c).astype(np.int64)[g] for c in cols], axis=1))
    return table_of(acc[:, :8], acc[:, 8:]), x["bad"]


def table_of(counters, sums):
    """The int32 table [P, 24] of int64 counters [P, 8] and sums [P, 8]."""
    P = counters.shape[0]
    table = np.zeros((P, WORDS), np.int64)
    table[:, :8] = counters
    table[:, 8::2], table[:, 9::2] = sums & 0xFFFFFFFF, (sums >> 32) & 0xFFFFFFFF
    return torch.from_numpy(table.astype(np.uint32).view(np.int32).copy())


# ------------------------------------------------------------------ windows
P_BITS = [bits_of(v) for v in (0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(0)),
                               np.nextafter(np.float32(0.5), np.float32(1)), 2.0 ** -126, 0.25, 0.75, 0.3, 0.999)]
PO_BITS = [0, 1, bits_of(1.0), bits_of(0.5), bits_of(0.3), bits_of(2.0 ** -126), bits_of(0.999)]
MU_VALUES = [NAN, INF, -INF, TWO20, -TWO20, ABOVE_TWO20, -ABOVE_TWO20, -0.0, 0.0, 0.5 / 256, 1.5 / 256, 2.5 / 256,
             -0.5 / 256, -1.5 / 256, 1000000.5 / 256, 1000001.5 / 256, 1500.0, 1499.99, -3.25, 2.0 ** -140, 3.0e38]
POISON = (INF, -INF, 3.0e38, -1.0e30)  # priors of slots that are no game: each would count as bad


def _mu_term(x):
    x32 = float(np.float32(x))
    if x32 != x32:
        return None
    if x32 in (INF, -INF) or abs(x32) > TWO20:
        return "bad"
    return int(round(Fraction(x32) * 256))  # exact product, ties to even


assert [_mu_term(v) for v in MU_VALUES[3:16]] == [2 ** 28, -2 ** 28, "bad", "bad", 0, 0, 0, 2, 2, 0, -2, 1000000,
                                                  1000002]


def live_mask(rec, P):
    r = rec.numpy().astype(np.int64)
    S = r.shape[1] - 2
    K = S // 2
    m0 = r[:, S] & 0xFFFFFFFF
    j = np.arange(S)
    occupied = np.where(j < K, j, j - K)[None, :] < np.where(j < K, (m0 >> 8 & 0xFF)[:, None], (m0 >> 16 & 0xFF)[:, None])
    return occupied & (r[:, :S] >= 0) & (r[:, :S] < P) & ((m0 & 0xFF) < 6)[:, None]


def poison(rec, priors, pred, P):
    """The priors of the slots that are no game overwritten with values that would be bad."""
    scored = torch.from_numpy(((pred[:, 0].numpy().view(np.uint32) & FLAG_SCORED) != 0))
    game = torch.from_numpy(live_mask(rec, P)) & scored[:, None]
    M, S = game.shape
    junk = torch.tensor(POISON, dtype=torch.float32)[torch.arange(M * 4 * S) % 4].reshape(M, 4, S)
    return torch.where(game[:, None, :], priors, junk)


def random_scored(K, M, P, seed, games=None, unscored=0.1, holes=0.1, ids=None):
    """(rec, priors [M, 4, 2K], pred [M, 4]): M matches of random players of [0, P) on random
    modes with one winner each, p_win0 / p_outcome from the edge patterns and random floats,
    mu words from ``MU_VALUES`` and a grid of sixteenths; ``unscored``: the share of rows
    without the scored flag (ties, inconsistent, nothing); ``holes``: the share of NaN mu words.
    ``games``: slots of the last matches are emptied until exactly that many are games (then
    every row is scored).  Whatever lies behind a slot that is no game is poisoned."""
    g = torch.Generator().manual_seed(seed)
    S = 2 * K
    ri = lambda hi, *shape: torch.randint(hi, shape, generator=g)  # noqa: E731
    n0, n1 = torch.full((M,), K), torch.full((M,), K)
    free = 0 if games is None else M * S - games
    for m in reversed(range(M)):
        if free <= 0:
            break
        drop = min(free, S - 1)
        free -= drop
        n1[m] = K - min(drop, K)
        n0[m] = K - (drop - (K - int(n1[m])))
    rec = torch.zeros((M, S + 2), dtype=torch.int64)
    rec[:, :S] = ri(P, M, S) if ids is None else ids
    mode = ri(6, M)
    rec[:, S] = mode | (n0 << 8) | (n1 << 16) | (2 << 24)
    rec[:, S + 1] = 1 + ri(2, M)
    pb = torch.tensor(P_BITS)[ri(len(P_BITS), M)]
    rnd = torch.rand(M, generator=g).to(torch.float32).view(torch.int32).to(torch.int64)
    pb = torch.where(ri(2, M) == 0, pb, rnd)
    po = torch.where(ri(2, M) == 0, torch.tensor(PO_BITS)[ri(len(PO_BITS), M)],
                     torch.rand(M, generator=g).to(torch.float32).view(torch.int32).to(torch.int64))
    flags = FLAG_SCORED | (mode << 8) | torch.where(rec[:, S + 1] == 1, FLAG_TEAM0_WON, 0)
    if games is None:
        other = torch.tensor([FLAG_TIE, FLAG_INCONSISTENT, 0, FLAG_TEAM0_WON])[ri(4, M)] | (mode << 8)
        flags = torch.where(torch.rand(M, generator=g) < unscored, other, flags)
    pred = torch.stack([flags, pb, po, torch.zeros(M, dtype=torch.int64)], dim=1)
    pred = ((pred + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
    grid = (ri(1 << 16, M, 4, S).to(torch.float32) - 32768.0) / 4096.0  # sixteenths of 1 / 256: ties among them
    special = torch.tensor(MU_VALUES, dtype=torch.float32)[ri(len(MU_VALUES), M, 4, S)]
    priors = torch.where(torch.rand((M, 4, S), generator=g) < 0.15, special, grid)
    priors = torch.where(torch.rand((M, 4, S), generator=g) < holes, torch.tensor(NAN), priors)
    rec = rec.to(torch.int32)
    return rec, poison(rec, priors, pred, P), pred


def scored(K, matches):
    """(rec, priors, pred) from a list of dicts: ``ids`` [2K] and optionally ``mode`` (1), ``n0`` /
    ``n1`` (K), ``meta1`` (1: roster 0 won), ``flags`` (scored), ``p`` / ``po`` (floats) or
    ``pbits`` / ``pobits``, ``mu0`` / ``mu2`` (per slot or one number; 1500.0 / NaN)."""
    S, M = 2 * K, len(matches)
    rec = torch.zeros((M, S + 2), dtype=torch.int64)
    pred = torch.zeros((M, 4), dtype=torch.int64)
    priors = torch.full((M, 4, S), 777.0, dtype=torch.float32)
    for m, c in enumerate(matches):
        rec[m, :S] = torch.tensor(c["ids"])
        rec[m, S] = c.get("mode", 1) | (c.get("n0", K) << 8) | (c.get("n1", K) << 16) | (2 << 24)
        rec[m, S + 1] = c.get("meta1", 1)
        pred[m, 0] = c.get("flags", FLAG_SCORED) | (c.get("mode", 1) << 8)
        pred[m, 1] = c["pbits"] if "pbits" in c else bits_of(c.get("p", 0.5))
        pred[m, 2] = c["pobits"] if "pobits" in c else bits_of(c.get("po", 0.5))
        for f, name, default in ((0, "mu0", 1500.0), (2, "mu2", NAN)):
            v = c.get(name, default)
            priors[m, f] = torch.tensor(v if isinstance(v, (list, tuple)) else [v] * S, dtype=torch.float32)
    pred = ((pred + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
    return rec.to(torch.int32), priors, pred


def value_matches():
    """K = 1, P = 3: player 0 in slot 0 meets player 1 once per value of each list."""
    ms = [{"ids": [0, 1], "pbits": b, "meta1": 1 + i % 2} for i, b in enumerate(P_BITS)]
    ms += [{"ids": [0, 1], "pobits": b} for b in PO_BITS]
    ms += [{"ids": [0, 1], "mu0": [v, 10.0]} for v in MU_VALUES]
    # the mode track: word 2 NaN and word 0 set, both NaN, word 2 set (and an infinite word 0 behind it)
    ms += [{"ids": [2, 1], "mu0": [8.0, NAN], "mu2": [NAN, NAN]}, {"ids": [2, 1], "mu0": [INF, 1.0], "mu2": [4.0, 2.0]}]
    return ms


SLOTS_P = 9


def slot_matches():
    """K = 3, P = 9: uneven rosters (1 v 3, 3 v 1, 2 v 3), twins within a roster and across the
    rosters, ids outside [0, P) in occupied slots, each with distinct strengths."""
    X = 8
    mu = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    return [{"ids": [0, X, X, 1, 2, 3], "n0": 1, "p": 0.25, "po": 0.25, "mu0": mu},
            {"ids": [0, 1, 2, 3, X, X], "n1": 1, "p": 0.75, "po": 0.25, "meta1": 2, "mu0": mu},
            {"ids": [4, 5, X, 6, 7, 0], "n0": 2, "p": 0.5, "mu0": mu},
            {"ids": [1, 1, 2, 3, 4, 5], "p": 0.6, "po": 0.6, "mu0": mu},           # twins within roster 0
            {"ids": [1, 2, 3, 1, 4, 3], "p": 0.4, "po": 0.6, "meta1": 2, "mu0": mu},  # twins across the rosters
            {"ids": [-1, 2, 9, 3, 2 ** 31 - 1, 4], "p": 0.7, "po": 0.7, "mu0": mu},  # three ids outside [0, P)
            {"ids": [5, 6, 7, 0, 1, 2], "p": 0.9, "po": 0.9, "mu0": [NAN, 2.0, INF, NAN, NAN, NAN]}]


def carry_window():
    """K = 1, P = 6: player 5 wins 300 games at q24 = 2^24 in slot 0 against players below it;
    1823 matches among players 0..4 put its run across the first tile edge of the sorted games."""
    ms = [{"ids": [i % 5, (i + 1) % 5], "p": 0.5} for i in range(1823)]
    ms[1000:1000] = [{"ids": [5, i % 5], "pbits": bits_of(1.0), "pobits": bits_of(1.0)} for i in range(300)]
    return ms


STITCH = (5, 52_429, 37)  # K, M, P of the window whose fold leaves 129 tiles


@functools.lru_cache(maxsize=None)
def case(name):
    """(rec, priors, pred, P, track) of a named case, built once and never modified."""
    kind, _, arg = name.partition(":")
    if kind == "tile":  # tile:K:games -- games just below / at / above one tile and above two
        K, games = (int(x) for x in arg.split(":"))
        M = -(-games // (2 * K))
        rec, priors, pred = random_scored(K, M, 37, seed=K * 10007 + games, games=games)
        assert int(expect_terms(rec, priors, pred, 37)["game"].sum()) == games
        return rec, priors, pred, 37, "mode"
    if kind == "three":  # one player in both slots of every match: a run over three tiles
        M = TILE + 100
        return random_scored(1, M, 1, seed=3, unscored=0.0) + (1, "mode")
    if kind == "exact":  # player 0's run ends on the last element of tile 0
        ids = torch.tensor([[0, 0]] * (TILE // 2) + [[1, 1]] * 50)
        return random_scored(1, ids.shape[0], 2, seed=4, unscored=0.0, ids=ids) + (2, "shared")
    if kind == "nogames":  # every row without the scored flag: the head key of tile 0 is P
        rec, priors, pred = random_scored(2, 300, 11, seed=5, unscored=1.1)
        assert not bool(expect_terms(rec, priors, pred, 11)["game"].any())
        return rec, priors, pred, 11, "mode"
    if kind == "m":  # m:M
        return random_scored(3, int(arg), 5, seed=6, unscored=0.0) + (5, "mode")
    if kind == "few":  # few:P -- every run crosses tile edges
        return random_scored(2, 2500, int(arg), seed=int(arg)) + (int(arg), "mode")
    if kind == "stitch":  # more than 256 edges: the stitch workgroup takes a second pass
        K, M, P = STITCH
        rec, priors, pred = random_scored(K, M, P, seed=77, unscored=0.0)
        keys = np.sort(rec[:, :2 * K].numpy().reshape(-1))
        assert len(keys) == 524_290 and 2 * -(-len(keys) // TILE) == 258
        assert keys[128 * TILE - 1] == keys[128 * TILE] and np.bincount(keys).min() > 2 * TILE
        return rec, priors, pred, P, "mode"
    if kind == "mixed":  # mixed:K:track
        K, track = arg.split(":")
        return random_scored(int(K), 700, 50, seed=20 + int(K), unscored=0.3) + (50, track)
    if kind == "values":  # values:track
        return scored(1, value_matches()) + (3, arg)
    if kind == "slots":
        rec, priors, pred = scored(3, slot_matches())
        return rec, poison(rec, priors, pred, SLOTS_P), pred, SLOTS_P, "shared"
    if kind == "carry":
        return scored(1, carry_window()) + (6, "shared")
    if kind == "split":
        return random_scored(2, 240, 11, seed=33, unscored=0.2) + (11, "mode")
    raise KeyError(name)


TILE_CASES = ["tile:%d:%d" % (K, n) for K in (1, 2, 3, 4, 5) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]
LONG_CASES = ["three", "exact", "few:2", "few:3", "stitch"]
OTHER_CASES = ["nogames", "m:0", "m:1", "values:mode", "values:shared", "slots", "carry", "split"] + \
    ["mixed:%d:%s" % (K, t) for K in (1, 2, 3, 4, 5) for t in ("mode", "shared")]


@functools.lru_cache(maxsize=None)
def expected(name):
    rec, priors, pred, P, track = case(name)
    return expect_ref(rec, priors, pred, P, track)


class Table:
    """An ``Expectations`` without a card: the table, the counter and ``add_scored``."""

    def __init__(self, P, device, track):
        self.exp = Expectations.__new__(Expectations)
        e = self.exp
        e.device, e.num_players, e.track, e.modes = torch.device(device), P, track, 63
        e.max_slots = int(native().MAX_SLOTS)
        e.table = torch.zeros((P, WORDS), dtype=torch.int32, device=device)
        e._bad = torch.zeros(1, dtype=torch.int64, device=device)


def fold(name, device, pieces=None, max_slots=None):
    """The ``Expectations`` of a case on ``device``: its window folded with ``add_scored`` in
    one piece, or the ``pieces`` (a, b) of it in the order given."""
    rec, priors, pred, P, track = case(name)
    exp = Table(P, device, track).exp
    if max_slots is not None:
        exp.max_slots = max_slots
    for a, b in pieces if pieces is not None else [(0, rec.shape[0])]:
        exp.add_scored(rec[a:b].to(device), priors[a:b].to(device), pred[a:b].to(device))
    return exp


@functools.lru_cache(maxsize=None)
def host_table(name):
    e = fold(name, "cpu")
    return e.table, e.bad


def assert_table(exp, want, what):
    got = exp.table.cpu()
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(want[0].shape)
    rows = (got != want[0]).any(dim=1).nonzero().reshape(-1)[:5].tolist()
    assert torch.equal(got, want[0]), (what, rows, got[rows].tolist(), want[0][rows].tolist())
    assert exp.bad == want[1], (what, "bad", exp.bad, want[1])


def check_case(name, device):
    exp = fold(name, device)
    assert exp.table.device.type == torch.device(device).type
    assert_table(exp, expected(name), name)
    if torch.device(device).type != "cpu":
        assert_table(exp, host_table(name), name + " (host mirror)")
    return exp


# ------------------------------------------------------------------ checks
def check_values(device):
    """The hand-made value patterns, figure by figure for player 0 (always slot 0)."""
    exp = check_case("values:shared", device)
    c = {k: v.cpu() for k, v in exp.columns().items()}
    n_p, n_po, n_mu = len(P_BITS), len(PO_BITS), len(MU_VALUES)
    assert int(c["games"][0]) == n_p + n_po + n_mu and int(c["games"][2]) == 2
    p24 = [int(round(Fraction(float(np.array([b], np.uint32).view(np.float32)[0])) * ONE)) for b in P_BITS]
    assert p24[:6] == [0, ONE, HALF, HALF, HALF + 1, 0]  # the float below 0.5 rounds to even
    assert int(c["exp"][0]) == sum(p24) + (n_po + n_mu) * HALF
    assert int(c["var"][0]) == sum((q * (ONE - q)) >> 16 for q in p24) + (n_po + n_mu) * ((HALF * HALF) >> 16)
    assert int(c["fav"][0]) == sum(q > HALF for q in p24) and int(c["dog"][0]) == sum(q < HALF for q in p24)
    cap, one_bit = 150 << 20, 1 << 20
    assert [nlog2_q20(b) for b in PO_BITS[:4]] == [cap, cap, 0, one_bit]
    assert int(c["surprise"][0]) == sum(nlog2_q20(b) for b in PO_BITS) + (n_p + n_mu) * one_bit
    terms = [_mu_term(v) for v in MU_VALUES]
    good = [t for t in terms if isinstance(t, int)]
    # +-inf, the floats beyond +-2^20, 3e38; and on the shared track player 2's infinite word 0
    assert terms.count("bad") == 5 and exp.bad == 6
    assert int(c["own"][0]) == sum(good) + (n_p + n_po) * 1500 * 256
    assert int(c["own_known"][0]) == len(good) + n_p + n_po
    # player 1 sees player 0's strengths as its opponents'; a bad value of another slot is not its own
    assert int(c["opp"][1]) == sum(good) + (n_p + n_po) * 1500 * 256 + 8 * 256 and int(c["opp_slots"][1]) == len(
        good) + n_p + n_po + 1
    assert int(c["mate_slots"].sum()) == 0 and int(c["mates"].abs().sum()) == 0
    # shared track: player 2's word 0 is 8.0, then inf (bad)
    assert int(c["own"][2]) == 8 * 256 and int(c["own_known"][2]) == 1
    mode = check_case("values:mode", device)
    m = {k: v.cpu() for k, v in mode.columns().items()}
    # mode track: word 2 is NaN everywhere but the last match -- 8.0 from word 0, then word 2 = 4.0
    assert int(m["own"][2]) == (8 + 4) * 256 and int(m["own_known"][2]) == 2 and mode.bad == exp.bad - 1
    assert int(m["opp"][2]) == 2 * 256 and int(m["opp_slots"][2]) == 1  # (NaN, NaN) has no strength


def check_slots(device):
    """``slot_matches``, slot by slot."""
    exp = check_case("slots", device)
    c = {k: v.cpu().tolist() for k, v in exp.columns().items()}
    u = 256
    # twins are two games: player 1 plays matches 0, 1, 3 (slots 0, 1), 4 (slots 0, 3) and 6
    assert c["games"] == [4, 7, 6, 6, 4, 3, 2, 2, 0] and exp.bad == 1
    # match 0, 1 v 3: player 0 alone (mates 0 of 0 slots) against 8 + 16 + 32, and wins
    # match 1, 3 v 1: player 0 with 2 + 4 against 8 alone; match 2: player 0 in roster 1 with 8 + 16 against 1 + 2
    # match 6: player 0 (slot 3, NaN) with NaN mates against 2.0 (the inf counts as bad for player 7, not as strength)
    assert c["mates"][0] == (0 + 6 + 24 + 0) * u and c["mate_slots"][0] == 0 + 2 + 2 + 0
    assert c["opp"][0] == (56 + 8 + 3 + 2) * u and c["opp_slots"][0] == 3 + 1 + 2 + 1
    assert c["own"][0] == (1 + 1 + 32) * u and c["own_known"][0] == 3
    assert c["exp"][0] == ONE // 4 + 3 * ONE // 4 + HALF + (ONE - int(round(Fraction(float(np.float32(0.9))) * ONE)))
    assert c["wins"][0] == 1 and c["wins"][3] == 0 + 1 + 0 + 1 + 0  # player 3 wins one of its two slots of match 4
    # player 1's mates: match 0 (slot 3) 16 + 32, match 1 (slot 1) 1 + 4, match 3 within roster 0 -- slot 0 has its
    # twin 2 and 4, slot 1 has 1 and 4 --, match 4 across the rosters -- slot 0 has 2 + 4, slot 3 has 16 + 32 --,
    # match 6 NaNs
    assert c["mates"][1] == (48 + 5 + 6 + 5 + 6 + 48 + 0) * u and c["mate_slots"][1] == 2 * 6
    assert c["games"][8] == 0 and c["exp"][8] == 0  # the bystander of the empty slots
    # match 5: the slots with ids -1, 9 and 2^31 - 1 are no games and no one's mates or opponents:
    # player 2 (slot 1, roster 0) has no mate there and meets 8 and 32
    assert c["mate_slots"][2] == 2 + 2 + 2 + 2 + 0 + 0 and c["opp_slots"][4] == 3 + 3 + 3 + 1


def check_guards(device):
    """Ids outside [0, P), emptied slots and unscored rows with poisoned priors next to a table
    with guard rows: nothing but the table moves."""
    rec, priors, pred, P, track = case("slots")
    exp = Table(P, device, track).exp
    big = torch.full((P + 2, WORDS), 0x55AA55, dtype=torch.int32, device=device)
    big[1:P + 1] = 0
    exp.table = big[1:P + 1]
    exp.add_scored(rec.to(device), priors.to(device), pred.to(device))
    assert_table(exp, expected("slots"), "slots")
    assert bool((big[0] == 0x55AA55).all()) and bool((big[P + 1] == 0x55AA55).all())
    dead = priors[:, 0][~torch.from_numpy(live_mask(rec, P))]
    assert dead.numel() == 8 and bool((dead.abs() > TWO20).all())  # each would count as bad


def check_carries(device):
    """exp of player 5 passes 2^32 inside one run, across a tile edge and across two calls."""
    exp = check_case("carry", device)
    c = exp.columns()
    assert int(c["exp"][5]) == 300 * ONE > 1 << 32 and int(c["wins"][5]) == 300 == int(c["fav_wins"][5])
    keys = np.sort(case("carry")[0][:, :2].numpy().reshape(-1))
    assert keys[TILE - 1] == 5 == keys[TILE] and keys[TILE - 150] == 5 and keys[TILE - 151] < 5
    M = case("carry")[0].shape[0]
    assert_table(fold("carry", device, [(0, 1150), (1150, M)]), expected("carry"), "two calls")  # 150 + 150 games
    assert exp.table[5, 9].item() == 1  # the high word


def check_invariance(device):
    M = case("split")[0].shape[0]
    whole = fold("split", device)
    assert_table(whole, expected("split"), "split")
    want = (whole.table.cpu(), whole.bad)
    assert whole.bad > 0
    sevens = [(a, min(M, a + 7)) for a in range(0, M, 7)]
    assert_table(fold("split", device, sevens), want, "chunks of 7 matches")
    assert_table(fold("split", device, sevens[::-1]), want, "reversed")
    assert_table(fold("split", device), want, "second run")
    assert_table(fold("split", device, [(0, M), (5, 5)]), want, "M = 0")
    assert_table(fold("split", device, max_slots=4 * 50 + 3), want, "max_slots: chunks of 50 matches")
    a, b = fold("split", device, [(0, 100)]), fold("split", device, [(100, M)])
    a.card = b.card = type("Card", (), {"table": torch.zeros(1, dtype=torch.int64, device=device)})()
    assert_table(a.merge(b), want, "merge")


# ------------------------------------------------------------------ every branch of "game"
@functools.lru_cache(maxsize=None)
def rated(K, M, P, seed=60, idle=0):
    """(roster before, rec, rows) on the CPU: a stream with every record feature, rated by the
    host mirror once; the last ``idle`` players of the roster never play."""
    roster = make_roster(RosterSpec(num_players=P, seed=seed + K))
    P -= idle
    rec = make_stream(StreamSpec(team_size=K, seed=seed + 10 + K, p_afk=0.05, p_unsupported=0.05, p_uneven=0.15,
                                 p_tie=0.05, skew=2), M, P, K=K)
    before = roster.clone()
    res = BatchRater(CFG).rate(roster, rec, K)
    return before, rec, res.packed


def scored_tensors(roster0, rec, rows, device, cuts=None, **kw):
    """(priors, pred, card) of a plain ``Scorecard`` over the windows ``cuts`` of (rec, rows)."""
    card = Scorecard(roster0.to(device) if hasattr(roster0, "to") else roster0, cfg=CFG, **kw)
    pri, prd = [], []
    for a, b in cuts or [(0, rec.shape[0])]:
        for _, _, priors, pred in card.scored_chunks(rec[a:b].to(device), rows[a:b].to(device)):
            pri.append(priors)
            prd.append(pred)
    return torch.cat(pri), torch.cat(prd), card


def check_branches(device):
    """One more match behind a rated window, made no game in every way there is: the table
    stays what it was without the match, and the pred row says why."""
    K, P = 2, 60
    roster0, rec, rows = rated(K, 120, P, idle=10)
    S = 2 * K
    good = torch.tensor([[3, 4, 5, 6, 1 | (K << 8) | (K << 16) | (2 << 24), 1]], dtype=torch.int32)
    last = rows[(rows.view(torch.int32)[:, 5 * S + 1] & 0xFF) == RATED][-1:].clone()

    def run(extra_rec=None, extra_row=None, modes=None, spoil=None):
        r = rec if extra_rec is None else torch.cat([rec, extra_rec])
        w = rows if extra_rec is None else torch.cat([rows, last if extra_row is None else extra_row])
        exp = Expectations(roster0.to(device), modes=modes, cfg=CFG)
        if spoil is not None:
            exp.card.chain[spoil, 0::2] = 1500.0  # a mu with a sigma of 0 on every track: the priors of this
            exp.card.chain[spoil, 1::2] = 0.0     # player do not resolve
        pred = exp.add(r.to(device), w.to(device), keep=True)
        return exp, pred

    base, base_pred = run()
    want = (base.table.cpu(), base.bad)
    assert int(base.columns()["games"].sum()) > 200
    added, pred = run(good)
    assert bool(pred.scored[-1]) and int(added.columns()["games"].sum()) == int(base.columns()["games"].sum()) + S

    def variant(col, value):
        r = good.clone()
        r[0, col] = value
        return r

    sizes = (K << 8) | (K << 16) | (2 << 24)
    not_rated = last.clone()
    not_rated.view(torch.int32)[0, 5 * S + 1] = AFK
    cases = {"not rated": dict(extra_rec=good, extra_row=not_rated),
             "unsupported mode": dict(extra_rec=variant(S, 255 | sizes)),
             "tie": dict(extra_rec=variant(S + 1, 0)),
             "both winner bits": dict(extra_rec=variant(S + 1, 3))}
    for what, kw in cases.items():
        exp, pred = run(**kw)
        assert not bool(pred.scored[-1]), what
        assert_table(exp, want, what)
    ranked_only, _ = run(modes=("ranked",))
    exp, pred = run(variant(S, 2 | sizes), modes=("ranked",))  # mode 2, blitz, is outside the mask
    assert not bool(pred.scored[-1])
    assert_table(exp, (ranked_only.table.cpu(), ranked_only.bad), "mode outside the mask")
    never = P - 1
    assert int(rec[:, :S].max()) < P - 10
    fresh = variant(0, never)  # a player no earlier match writes: its prior is the chain row as it starts
    _, ok_pred = run(fresh)
    assert bool(ok_pred.scored[-1])
    exp, pred = run(fresh, spoil=never)
    assert not bool(pred.scored[-1]) and bool(pred.flags[-1] & FLAG_INCONSISTENT)
    assert_table(exp, want, "inconsistent")


# ------------------------------------------------------------------ end to end
def check_end_to_end(K, device):
    """A synthetic window rated, then ``Expectations.add`` in two windows: the oracle on the
    device's own priors and pred, the conservation sums and the card."""
    M, P = (3000, 4000) if K == 3 else (1200, 4000)
    roster0, rec, rows = rated(K, M, P, seed=40)
    rec_d, rows_d = rec.to(device), rows.to(device)
    h = M // 2 + 7
    exp = Expectations(roster0.to(device), cfg=CFG)
    preds = [exp.add(rec_d[a:b], rows_d[a:b], keep=True) for a, b in ((0, h), (h, M))]
    priors, pred, card = scored_tensors(roster0, rec, rows, device, cuts=[(0, h), (h, M)])
    assert torch.equal(torch.cat([p.flags for p in preds]), pred[:, 0])
    want = expect_ref(rec, priors.cpu(), pred.cpu(), P, "mode")
    assert_table(exp, want, "end to end %dv%d" % (K, K))
    assert torch.equal(exp.card.table, card.table) and torch.equal(exp.card.chain.view(torch.int32),
                                                                   card.chain.view(torch.int32))
    c = {k: v.cpu() for k, v in exp.columns().items()}
    scored_m = torch.cat([p.scored for p in preds]).cpu().numpy()
    assert int(c["games"].sum()) > 3 * K * scored_m.sum() // 2 and scored_m.sum() > M // 2
    # sum_p surprise = sum over scored matches of live slots * nlog2_q20(p_outcome)
    live = live_mask(rec, P).sum(axis=1)
    po = torch.cat([p.p_outcome for p in preds]).cpu().view(torch.int32).numpy().view(np.uint32)
    assert int(c["surprise"].sum()) == sum(int(live[m]) * nlog2_q20(int(po[m])) for m in np.nonzero(scored_m)[0])
    # over the matches with even rosters, the expected wins of all players are the wins there are
    m0 = rec[:, 2 * K].numpy().astype(np.int64)
    even = torch.from_numpy(((m0 >> 8) & 0xFF) == ((m0 >> 16) & 0xFF))
    assert 0 < int(even.sum()) < M
    sub = Table(P, device, "mode").exp.add_scored(rec_d[even.to(device)], priors[even.to(device)],
                                                  pred[even.to(device)])
    s = sub.columns()
    assert int(s["exp"].sum()) == ONE * int(s["wins"].sum()) > 0
    assert int(c["exp"].sum()) != ONE * int(c["wins"].sum())  # the uneven matches do not balance
    return exp


# ------------------------------------------------------------------ the API on a hand-made table
def hand_table(device):
    """P = 8: z scores 4, 4, 3, -3.5, -4, NaN (sd 0), a player below min_games and an empty row."""
    P = 8
    e = Table(P, device, "mode").exp
    cnt, sums = np.zeros((P, 8), np.int64), np.zeros((P, 8), np.int64)
    # var = 25 * 2^32 -> sd 5; exp = 50 wins
    for p, (games, wins, var, exp) in enumerate([(100, 70, 25, 50), (100, 70, 25, 50), (100, 65, 25, 50),
                                                 (100, 33, 16, 47), (100, 30, 25, 50), (30, 30, 0, 30),
                                                 (10, 10, 1, 2), (0, 0, 0, 0)]):
        cnt[p, 0], cnt[p, 1], sums[p, 0], sums[p, 1] = games, wins, exp * ONE, var << 32
        sums[p, 2] = games << 20  # one bit per game
        cnt[p, 6], sums[p, 3] = games, games * 1500 * 256
        sums[p, 4], sums[p, 5] = 2 * games * (1400 + p) * 256, 2 * games
        sums[p, 6], sums[p, 7] = 3 * games * 1450 * 256, 3 * games
    e.table.copy_(table_of(cnt, sums))
    return e


def check_api(device):
    e = hand_table(device)
    look = {k: v.cpu() for k, v in e.lookup([0, 3, 5, 7]).items()}
    assert look["games"].tolist() == [100, 100, 30, 0] and look["exp"].dtype == torch.int64
    assert look["expected"].tolist() == [50.0, 47.0, 30.0, 0.0] and look["surplus"].tolist() == [20.0, -14.0, 0.0, 0.0]
    assert look["sd"].tolist() == [5.0, 4.0, 0.0, 0.0] and look["z"][:2].tolist() == [4.0, -3.5]
    assert bool(torch.isnan(look["z"][2:]).all()) and look["bits"][:3].tolist() == [1.0, 1.0, 1.0]
    assert look["own_mean"][:3].tolist() == [1500.0] * 3 and look["mates_mean"][:2].tolist() == [1400.0, 1403.0]
    assert look["opp_mean"][0].item() == 1450.0 and look["edge"][:2].tolist() == [-50.0, -47.0]
    assert all(bool(torch.isnan(look[k][3])) for k in ("bits", "own_mean", "mates_mean", "opp_mean", "edge", "z"))
    out = e.outliers(min_games=20, z=3.0)
    assert out["ids"].tolist() == [0, 1, 2] and out["z"].tolist() == [4.0, 4.0, 3.0]  # ties by id
    assert out["games"].tolist() == [100] * 3 and out["surplus"].tolist() == [20.0, 20.0, 15.0]
    assert e.outliers(min_games=20, z=3.0, top=2)["ids"].tolist() == [0, 1]
    assert e.outliers(min_games=5, z=3.0)["ids"].tolist() == [6, 0, 1, 2]  # z = 8 with 10 games
    assert e.outliers(min_games=20, z=-3.0)["ids"].tolist() == [4, 3]  # the other tail, worst first
    assert e.outliers(min_games=20, z=4.5)["ids"].tolist() == [] and e.outliers(z=3.0, top=0)["ids"].tolist() == []
    fair = e.fairness(min_games=20)
    assert fair["players"] == 6 and fair["edge"]["n"] == 6 and fair["mean_q"]["n"] == 6
    edges = sorted(-50.0 + p for p in range(6))
    assert fair["edge"]["quantiles"]["q50"] == float(np.quantile(edges, 0.5)) and fair["edge"]["mean"] == -47.5
    assert fair["mean_q"]["quantiles"]["q95"] == float(np.quantile([0.5, 0.5, 0.5, 0.47, 0.5, 1.0], 0.95))
    assert -1.0 <= fair["edge"]["games_corr"] <= 1.0 and fair["mean_q"]["games_corr"] < 0  # the 30-game player has q 1
    none = e.fairness(min_games=1000)
    assert none["players"] == 0 and none["edge"]["mean"] is None and none["edge"]["games_corr"] is None
    lines = EX.expectation_lines(e, [3, 7])
    assert lines[0]["expect"] == 3 and lines[0]["z"] == -3.5 and lines[1]["z"] is None and lines[1]["games"] == 0
    assert json.loads(json.dumps(lines)) == lines
    line = EX.outliers_line(e, 2)
    assert [o["player"] for o in line["outliers"]] == [0, 1] and line["bad"] == 0
    try:
        e.lookup([8])
    except ValueError:
        pass
    else:
        raise AssertionError("an id outside [0, P) must raise")


def check_merge(device):
    K, P = 3, 60
    roster0, rec, rows = rated(K, 300, P)
    whole = Expectations(roster0.to(device), cfg=CFG)
    whole.add(rec.to(device), rows.to(device))
    priors, pred, _ = scored_tensors(roster0, rec, rows, device)
    a = Expectations(roster0.to(device), cfg=CFG).add_scored(rec[:100].to(device), priors[:100], pred[:100])
    b = Expectations(roster0.to(device), cfg=CFG).add_scored(rec[100:].to(device), priors[100:], pred[100:])
    assert_table(a.merge(b), (whole.table.cpu(), whole.bad), "merge")
    other = Expectations(roster0.to(device), track="shared", cfg=CFG)
    try:
        a.merge(other)
    except ValueError:
        pass
    else:
        raise AssertionError("tables of different options must not merge")


def check_arena(spec, device):
    """``RecordArena.expectations`` equals window-by-window ``add``."""
    from analyzer_amd.runtime.rerate import rerate_resident, start_roster, stream_records

    import records_cases as RC

    roster0 = start_roster(spec, None, torch.device(device))
    _, roster, arena = rerate_resident(spec, device, free_bytes=RC.FREE)
    rec_of = stream_records(spec, device)
    exp = arena.expectations(roster0, rec_of, cfg=CFG)
    want = Expectations(roster0, cfg=CFG)
    for lo, hi in arena.windows():
        want.add(rec_of(lo, hi), arena.result(lo, hi).packed)
    assert_table(exp, (want.table.cpu(), want.bad), "arena")
    assert torch.equal(exp.card.table, want.card.table) and int(exp.columns()["games"].sum()) > spec.total_matches
    return arena


CLI = ["--matches", "900", "--players", "120", "--window", "400"]


def run_cli(device, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", device, *CLI, *args],
                          capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)


def check_cli(device):
    ok = run_cli(device, "--records", "resident", "--arena-free-bytes", str(1 << 30), "--expect", "5,7,119",
                 "--expect-outliers", "3", "--expect-track", "shared")
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"expect"')]
    assert [ln["expect"] for ln in lines] == [5, 7, 119] and all(ln["track"] == "shared" for ln in lines)
    assert lines[0]["games"] > 0 and abs(lines[0]["surplus"] - (lines[0]["wins"] - lines[0]["expected"])) < 1e-9
    out = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"outliers"')]
    assert len(out) == 1 and len(out[0]["outliers"]) <= 3 and out[0]["z"] == 3.0
