"""Shared cases of the career tests (test_careers.py on the CPU, test_careers_gpu.py on the
device): a plain Python oracle of the career table, written from the definition of a game
and of the career row (not from csrc/career_core.h), the windows it is checked on, and the
checks that run the same way on either device.

The oracle eats *hits* -- the [n, 12] int32 rows of ``records_select`` (K10) for every
player -- either from ``records_cases.select_ref`` (a plain loop) or from
``RecordArena.history(range(P))``: a hit of a player is a game of that player if its mode
is selected."""
import functools
from fractions import Fraction

import numpy as np
import torch

from analyzer_amd.config import MODES
from analyzer_amd.ops.careers import CareerTable
from analyzer_amd.ops.native import native
from analyzer_amd.ops.rate import AFK, INVALID_ROSTERS, RATED, RateResult

import records_cases as RC

TILE = 4096  # sorted elements per workgroup of the fold (csrc/kernels.h kCareerTile; checked below)
NONE = 0x7FC00000
NAN = float("nan")


def check_tile():
    assert int(native().CAREER_TILE) == TILE and int(native().CAREER_WORDS) == 16


# ------------------------------------------------------------------ the oracle
def _words64(v):
    return [v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF]


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _quality_term(q):
    if q != q or q < 0 or q > 1:
        return 0
    return int(round(Fraction(float(q)) * (1 << 24)))  # exact product, ties to even


def _career_row(games):
    """games: (match, status, score, win, quality) in (match, slot) order."""
    rated = [g for g in games if g[1] == RATED]
    row = [len(rated), sum(1 for g in rated if g[3]), sum(1 for g in games if g[1] == AFK),
           sum(1 for g in games if g[1] == INVALID_ROSTERS)]
    row += _words64(rated[0][0] if rated else -1) + _words64(rated[-1][0] if rated else -1)
    scored = [(float(g[2]), g[0]) for g in rated if g[2] == g[2]]
    if scored:
        top, low = max(s for s, _ in scored), min(s for s, _ in scored)
        row += [_bits(top)] + _words64(next(m for s, m in scored if s == top)) + [_bits(low)]
    else:
        row += [NONE] + _words64(-1) + [NONE]
    streak = 0
    for g in reversed(rated):
        if bool(g[3]) != bool(rated[-1][3]):
            break
        streak += 1 if g[3] else -1
    best = run = 0
    for g in rated:
        run = run + 1 if g[3] else 0
        best = max(best, run)
    row += [streak & 0xFFFFFFFF, best] + _words64(sum(_quality_term(g[4]) for g in rated) & (2 ** 64 - 1))
    return row


def career_ref(hits, P, K, track="shared", score="conservative", modes=None):
    """The career table [P, 16] int32 of the games among ``hits`` [n, 12] (ascending
    (match, slot))."""
    h = hits.numpy().astype(np.int64)
    f = hits.numpy().view(np.float32)
    allowed = set(range(len(MODES))) if modes is None else {MODES.index(m) for m in modes}
    games = [[] for _ in range(P)]
    zero = np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(h.shape[0]):
            if (h[i, 10] & 0xFF) not in allowed:
                continue
            match = int((h[i, 0] & 0xFFFFFFFF) | (h[i, 1] << 32))
            slot, status = int(h[i, 3] & 0xFF), int((h[i, 3] >> 8) & 0xFF)
            mu, sigma = (f[i, 4], f[i, 5]) if track == "shared" else (f[i, 7], f[i, 8])
            s = (mu if score == "mu" else mu - sigma) + zero  # fp32; -0 becomes +0
            win = bool(h[i, 11] & (1 if slot < K else 2))
            games[int(h[i, 2])].append((match, status, s, win, f[i, 9]))
    table = np.array([_career_row(g) for g in games], dtype=np.int64).reshape(P, 16)
    return torch.from_numpy(table.astype(np.uint32).view(np.int32).copy())


def hits_from_history(hist):
    """The [n, 12] hits behind the columns of ``RecordArena.history``."""
    m = hist["match"].cpu()
    cols = [(m & 0xFFFFFFFF), (m >> 32), hist["player"].cpu().to(torch.int64),
            (hist["slot"].cpu() | (hist["status"].cpu() << 8)).to(torch.int64)]
    cols += [hist[n].cpu().view(torch.int32).to(torch.int64)
             for n in ("s_mu", "s_sig", "delta", "m_mu", "m_sig", "quality")]
    meta = hist["meta"].cpu().to(torch.int64)
    a = torch.stack(cols + [meta[:, 0], meta[:, 1]], dim=1).numpy()
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy())


# ------------------------------------------------------------------ windows
def window(K, matches):
    """(rec, rows) from a list of dicts: ``ids`` [2K], and optionally ``mode`` (1), ``n0`` / ``n1``
    (K), ``nr`` (2), ``meta1`` (1: roster 0 won), ``status`` (RATED), ``s_mu`` / ``s_sig`` /
    ``m_mu`` / ``m_sig`` (per slot or one number) and ``q``.  Unset words hold a marker."""
    S, W = 2 * K, RateResult.row_floats(K)
    rec = torch.zeros((len(matches), S + 2), dtype=torch.int64)
    rows = torch.full((len(matches), W), 12345.0, dtype=torch.float32)
    words = rows.view(torch.int32)
    for m, c in enumerate(matches):
        rec[m, :S] = torch.tensor(c["ids"])
        rec[m, S] = c.get("mode", 1) | (c.get("n0", K) << 8) | (c.get("n1", K) << 16) | (c.get("nr", 2) << 24)
        rec[m, S + 1] = c.get("meta1", 1)
        for f, name in enumerate(("s_mu", "s_sig", "delta", "m_mu", "m_sig")):
            v = c.get(name, (1500.0, 300.0, 0.0, 1400.0, 250.0)[f])
            rows[m, f * S:(f + 1) * S] = torch.tensor(v if isinstance(v, (list, tuple)) else [v] * S,
                                                      dtype=torch.float32)
        rows[m, 5 * S] = c.get("q", 0.5)
        words[m, 5 * S + 1] = c.get("status", RATED) | 0x5A5A00  # only the low byte is the status
    return rec.to(torch.int32), rows


def random_window(K, M, P, seed, games=None, other=0.0, grid=7):
    """M matches of random players of [0, P) with scores on a small integer grid (many equal
    peaks, zeros of both signs), random winners, modes and qualities; ``other``: the share
    of matches that are AFK, invalid, unsupported or failed.  ``games``: empty slots of the
    last matches until exactly that many slots are occupied."""
    g = torch.Generator().manual_seed(seed)
    S = 2 * K
    ri = lambda hi, *shape: torch.randint(hi, shape, generator=g)  # noqa: E731
    free = 0 if games is None else M * S - games
    drops = [0] * M
    for m in reversed(range(M)):
        drops[m] = min(free, S - 1)
        free -= drops[m]
    matches = []
    for m in range(M):
        drop = drops[m]
        n1 = K - min(drop, K)
        n0 = K - (drop - (K - n1))
        st = RATED
        if float(torch.rand((), generator=g)) < other:
            st = [AFK, INVALID_ROSTERS, 3, 7, 255][int(ri(5))]
        matches.append({
            "ids": ri(P, S).tolist(), "mode": int(ri(6)), "n0": n0, "n1": n1, "meta1": int(ri(2)) + 1,
            "status": st, "q": float(ri(1 << 12)) / (1 << 12),
            "s_mu": (ri(grid, S) - grid // 2).to(torch.float32).mul(-1.0).tolist(),  # -0.0 among them
            "s_sig": ri(3, S).to(torch.float32).tolist(),
            "m_mu": (ri(grid, S) * 100.0).tolist(), "m_sig": (ri(grid, S) * 10.0 + 1.0).tolist()})
    return window(K, matches)


def hand_built():
    """K = 2, P = 9: (rec, rows).  Player 0: every status.  Player 1: NaN score, zeros of
    both signs, negative scores.  Player 2: equal peaks.  Player 3: both teams of one
    match.  Player 4: AFK and invalid games inside a win streak.  Player 5: the qualities.
    Ids outside [0, 9) sit in occupied slots of rated rows."""
    X = 8  # a bystander
    ms = [{"ids": [0, X, X, X], "status": st} for st in (RATED, AFK, INVALID_ROSTERS, 3, 4, 5, 6, 7, 8, 255, RATED)]
    ms += [{"ids": [-1, 9, 2 ** 31 - 1, -5]}, {"ids": [X, -1, 100, X]}, {"ids": [1, X, X, X], "n0": 1, "n1": 0}]
    for mu, sg in ((NAN, 1.0), (-0.0, 0.0), (0.0, 0.0), (-3.0, 2.0), (-7.5, 0.0), (5.0, NAN)):
        ms.append({"ids": [X, 1, X, X], "s_mu": mu, "s_sig": sg, "meta1": 2})
    for mu in (10.0, 40.0, 20.0, 40.0, 40.0, 5.0, 5.0):
        ms.append({"ids": [X, X, 2, X], "s_mu": mu, "s_sig": 15.0, "meta1": 2})
    ms += [{"ids": [3, X, 3, X], "meta1": 1, "s_mu": [9.0, 0.0, 9.0, 0.0], "s_sig": 1.0}]
    for st, w in ((RATED, 2), (RATED, 1), (AFK, 2), (RATED, 1), (INVALID_ROSTERS, 2), (7, 2), (RATED, 1)):
        ms.append({"ids": [4, X, X, X], "status": st, "meta1": w})
    for q in (0.0, 1.0, 2.0 ** -25, 1.5 * 2.0 ** -24, NAN, 1.5, -0.25, 0.75):
        ms.append({"ids": [X, X, X, 5], "q": q, "meta1": 2})
    ms += [{"ids": [6, 6, 6, 6], "mode": 255, "status": 3}, {"ids": [6, X, X, X], "mode": 2, "n0": 0, "n1": 2}]
    return window(2, ms)


HAND_P = 9
SPLIT = (2, 40, 5)  # K, M, P of the split-invariance window
STITCH = (5, 52_429, 37)  # K, M, P of the window whose fold leaves 129 tiles


@functools.lru_cache(maxsize=None)
def case(name):
    """(rec, rows, base, P, options of CareerTable) of a named case, built once."""
    kind, _, arg = name.partition(":")
    if kind == "tile":  # tile:K:games -- games just below / at / above one tile and above two
        K, games = (int(x) for x in arg.split(":"))
        M = -(-games // (2 * K))
        return random_window(K, M, 37, seed=K * 10007 + games, games=games) + (3, 37, {})
    if kind == "alias":  # one player in both slots of every match: a win and a loss per match
        M = TILE + TILE // 2
        return window(1, [{"ids": [0, 0], "meta1": 1 + (m % 5 == 0), "s_mu": float(m % 11), "s_sig": 1.0}
                          for m in range(M)]) + (0, 1, {})
    if kind == "few":  # few:P -- every run crosses tile edges
        return random_window(2, 2500, int(arg), seed=int(arg)) + (11, int(arg), {})
    if kind == "stitch":  # more than 256 edges: the stitch kernel runs a second iteration
        K, M, P = STITCH
        rec, rows = random_window(K, M, P, seed=77)
        keys = np.sort(rec[:, :2 * K].numpy().reshape(-1))  # every slot is a game
        edges = 2 * -(-len(keys) // TILE)
        assert len(keys) == 524_290 and edges == 258
        # edge 255 ends tile 127, edge 256 begins tile 128: one player's run crosses the iterations
        assert keys[128 * TILE - 1] == keys[128 * TILE]
        return rec, rows, 9, P, {}
    if kind == "mixed":  # every kind of match, random
        return random_window(3, 900, 50, seed=5, other=0.3) + (0, 50, {})
    if kind == "nogame":  # the games end inside tile 0: tiles 1 and 2 return early and leave kNoKey edges
        K, M, P, occupied = 3, 1370, 50, 3000
        rec, rows = random_window(K, M, P, seed=41, games=occupied, other=0.3)
        meta0 = rec[:, 2 * K]
        assert int((((meta0 >> 8) & 0xFF) + ((meta0 >> 16) & 0xFF)).sum()) == occupied  # every game is one of these
        assert occupied < TILE and 2 * TILE < M * 2 * K
        return rec, rows, 4, P, {}
    if kind == "real":  # rated by the host mirror; most of the 6000 players never play
        return RC.rated_window(3, 700, 6000) + (1000, 6000, {})
    if kind == "hand":
        return hand_built() + (100, HAND_P, {})
    if kind == "base64":
        return random_window(3, 60, 20, seed=9) + (5_000_000_000, 20, {})
    if kind == "opt":  # opt:track:score:modes
        track, score, modes = arg.split(":")
        return random_window(3, 300, 40, seed=21, other=0.2) + (
            7, 40, {"track": track, "score": score, "modes": tuple(modes.split("+")) if modes else None})
    if kind == "split":
        K, M, P = SPLIT
        return random_window(K, M, P, seed=33, other=0.2, grid=3) + (500, P, {})
    raise KeyError(name)


TILE_CASES = ["tile:%d:%d" % (K, n) for K in (1, 2, 3, 4, 5) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]
LONG_CASES = ["alias", "few:2", "few:3"]
DEVICE_LONG_CASES = LONG_CASES + ["stitch"]  # its expected table is the host mirror's: nothing to check on the CPU
OTHER_CASES = ["mixed", "nogame", "real", "hand", "base64", "opt:shared:conservative:ranked", "opt:mode:conservative:",
               "opt:shared:mu:", "opt:mode:mu:casual+blitz", "split"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's table of a case, from the plain-loop hits of every player."""
    if name == "stitch":  # the plain loops take 9 s over 524,290 games: the host mirror, which
        return host_table(name)  # every smaller case pins to the oracle
    rec, rows, base, P, opt = case(name)
    K = (rec.shape[1] - 2) // 2
    return career_ref(RC.select_ref(rec, rows, base, P, range(P)), P, K, **opt)


def run(name, device, cuts=()):
    """The table of a case on ``device``, its window added in one piece or cut at ``cuts``."""
    rec, rows, base, P, opt = case(name)
    table = CareerTable(P, device, **opt)
    edges = [0, *cuts, rec.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        table.add(rec[a:b].to(device), rows[a:b].to(device), base + a)
    return table


@functools.lru_cache(maxsize=None)
def host_table(name):
    return run(name, "cpu").table


def check_case(name, device):
    table = run(name, device)
    assert table.table.dtype == torch.int32 and tuple(table.table.shape) == (case(name)[3], 16)
    assert table.table.device.type == torch.device(device).type
    got = table.table.cpu()
    bad = (got != expected(name)).any(dim=1).nonzero().reshape(-1)[:5].tolist()
    assert torch.equal(got, expected(name)), (name, bad, got[bad].tolist(), expected(name)[bad].tolist())
    if torch.device(device).type != "cpu":
        assert torch.equal(got, host_table(name)), name
    return table


def streak_cut(name):
    """A cut inside a win streak of the case: the index of a match after which some player's
    next rated game continues a run of wins."""
    rec, rows, base, P, _ = case(name)
    K = (rec.shape[1] - 2) // 2
    hits = RC.select_ref(rec, rows, base, P, range(P)).numpy()
    last = {}
    for h in hits:
        if (h[3] >> 8) & 0xFF != RATED:
            continue
        win = bool(h[11] & (1 if (h[3] & 0xFF) < K else 2))
        m = int(h[0]) - base
        if win and last.get(int(h[2]), (False, m))[0] and last[int(h[2])][1] < m and 1 < m < rec.shape[0] - 1:
            return m
        last[int(h[2])] = (win, m)
    raise AssertionError("the case has no win streak over two matches")


def check_split_invariance(device):
    one = run("split", device).table.cpu()
    assert torch.equal(one, expected("split"))
    M = SPLIT[1]
    s = streak_cut("split")
    assert 1 < s < M - 1
    for cuts in ((1,), (s,), (M - 1,), (1, s), (s, M - 1), (1, M - 1)):
        assert torch.equal(run("split", device, cuts).table.cpu(), one), cuts


def check_hand_built(device):
    cols = {k: v.cpu().tolist() for k, v in check_case("hand", device).columns().items()}
    base = 100
    # player 0: of eleven statuses one AFK, one invalid and the two rated ones count
    assert (cols["games"][0], cols["afk"][0], cols["invalid"][0]) == (2, 1, 1)
    assert (cols["first"][0], cols["last"][0]) == (base, base + 10)
    # player 1: seven rated games (slot 0 of match 13 exists, the bystander's slots past n0 / n1 do
    # not); the NaN scores are games but never peak or trough, -0 reads as +0
    assert cols["games"][1] == 7 and cols["peak"][1] == 1500.0 - 300.0 and cols["trough"][1] == -7.5
    # player 2: 25, the peak, is reached three times; the earliest match holds it
    first2 = base + 11 + 3 + 6
    assert cols["peak"][2] == 25.0 and cols["peak_match"][2] == first2 + 1 and cols["trough"][2] == -10.0
    # player 3: slot 0 wins, then slot 2 loses, in one match
    assert (cols["games"][3], cols["wins"][3], cols["streak"][3], cols["best_win"][3]) == (2, 1, -1, 1)
    assert cols["first"][3] == cols["last"][3] == cols["peak_match"][3]
    # player 4: loss, win, (AFK), win, (invalid), (error), win
    assert (cols["games"][4], cols["wins"][4], cols["streak"][4], cols["best_win"][4]) == (4, 3, 3, 3)
    # player 5: 0 + 2^24 + 0 (tie to even) + 2 (tie to even) + 0 + 0 + 0 + 0.75 * 2^24
    assert cols["quality_sum"][5] == (1 << 24) + 2 + 3 * (1 << 22) and cols["streak"][5] == 8
    # player 6 appears only in an unsupported match and past n0; 7 never; nobody out of range
    assert cols["games"][6] == cols["games"][7] == 0 and cols["first"][7] == -1 and cols["peak"][7] != cols["peak"][7]
    assert sum(cols["games"]) + sum(cols["afk"]) + sum(cols["invalid"]) == int(
        RC.select_ref(*case("hand")[:4], range(HAND_P)).shape[0])


def check_guarded_table(device):
    """Ids -1, P and beyond in occupied slots of rated rows: the rows next to the table are
    never touched."""
    rec, rows, base, P, _ = case("hand")
    table = CareerTable(P, device)
    big = torch.full((P + 2, 16), 0x55AA55, dtype=torch.int32, device=device)
    big[1:P + 1] = table.table
    table.table = big[1:P + 1]
    table.add(rec.to(device), rows.to(device), base)
    assert torch.equal(table.table.cpu(), expected("hand"))
    assert bool((big[0] == 0x55AA55).all()) and bool((big[P + 1] == 0x55AA55).all())


def check_64_bit(device):
    cols = check_case("base64", device).columns()
    played = cols["games"] > 0
    assert int(played.sum()) > 10
    for name in ("first", "last", "peak_match"):
        assert cols[name].dtype == torch.int64
        assert bool((cols[name][played] >= 5_000_000_000).all()) and bool((cols[name][played] < 5_000_000_060).all())
    assert bool((cols["first"][~played] == -1).all())


def check_empty_window_and_chunks(device):
    rec, rows, base, P, _ = case("mixed")
    table = CareerTable(P, device)
    before = table.table.clone()
    table.add(rec[:0].to(device), rows[:0].to(device), 5)
    assert torch.equal(table.table, before) and bool((table.columns()["peak_match"] == -1).all())
    table.max_slots = 6 * 100 + 5  # ``add`` splits the window into chunks of 100 matches itself
    table.add(rec.to(device), rows.to(device), base)
    assert torch.equal(table.table.cpu(), expected("mixed"))


def check_lookup(device):
    table = check_case("mixed", device)
    ids = [3, 0, 49, 3]
    look = table.lookup(ids)
    cols = table.columns()
    for name, col in cols.items():
        assert torch.equal(look[name].cpu().view(torch.int32 if col.dtype == torch.float32 else col.dtype),
                           col.cpu()[ids].view(torch.int32 if col.dtype == torch.float32 else col.dtype)), name
    games, wins = cols["games"].cpu()[ids].double(), cols["wins"].cpu()[ids].double()
    assert torch.equal(look["win_rate"].cpu(), wins / games)
    assert torch.equal(look["mean_quality"].cpu(), cols["quality_sum"].cpu()[ids].double() / (1 << 24) / games)
    empty = CareerTable(4, device).lookup([1])
    assert bool(torch.isnan(empty["win_rate"]).all()) and bool(torch.isnan(empty["mean_quality"]).all())
    assert bool(torch.isnan(empty["peak"]).all()) and int(empty["first"][0]) == -1


def check_arena_careers(spec, device):
    """``RecordArena.careers`` over a small resident re-rate against the oracle fed from
    ``history(range(P))``; returns (arena, table)."""
    from analyzer_amd.runtime.rerate import rerate_resident, stream_records

    _, _, arena = rerate_resident(spec, device, free_bytes=RC.FREE)
    rec_of = stream_records(spec, device)
    hist = arena.history(range(spec.players), spec.players, rec_of)
    want = career_ref(hits_from_history(hist), spec.players, spec.team_size)
    table = arena.careers(spec.players, rec_of)
    assert torch.equal(table.table.cpu(), want)
    assert int(table.columns()["games"].sum()) > spec.total_matches  # most matches are rated
    ranked = arena.careers(spec.players, rec_of, track="mode", modes=("ranked",))
    assert torch.equal(ranked.table.cpu(), career_ref(hits_from_history(hist), spec.players, spec.team_size,
                                                      track="mode", modes=("ranked",)))
    return arena, table
