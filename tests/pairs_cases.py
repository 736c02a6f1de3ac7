"""Shared cases of the pair-table tests (test_pairs.py on the CPU, test_pairs_gpu.py on the
device): a plain Python oracle of the pair table -- a dict keyed by (a, b), filled by loops
over the records and the status bytes straight from the definition of an entry (not from
csrc/pair_core.h) -- the windows it is checked on, and the checks that run the same way on
either device.  Every comparison is ``torch.equal`` on keys and counts."""
import functools
import json
import os
import subprocess
import sys

import torch

from analyzer_amd.config import MODES
from analyzer_amd.ops.native import native
from analyzer_amd.ops.pairs import PairTable
from analyzer_amd.ops.rate import AFK, INVALID_ROSTERS, RATED
from analyzer_amd.ops.synth import make_stream

import career_cases as CC
import records_cases as RC

TILE = 2048  # sorted entries per workgroup of count and emit (csrc/kernels.h kPairTile; checked below)
ENTRIES = {1: 2, 2: 12, 3: 30, 4: 56, 5: 90}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_constants():
    assert int(native().PAIR_TILE) == TILE and int(native().PAIR_WORDS) == 4
    assert {K: int(native().PAIR_ENTRIES(K)) for K in ENTRIES} == ENTRIES


# ------------------------------------------------------------------ the oracle
def pairs_dict(rec, rows, P, modes=None, players=None):
    """{(a, b): [with_games, with_wins, vs_games, vs_wins]} of a window."""
    r_ = rec.numpy()
    w_ = rows.view(torch.int32).numpy()
    S = r_.shape[1] - 2
    K = S // 2
    allowed = set(range(len(MODES))) if modes is None else {MODES.index(m) for m in modes}
    keep = None if players is None else {int(p) for p in players}
    out = {}
    for m in range(r_.shape[0]):
        m0, m1 = int(r_[m, S]) & 0xFFFFFFFF, int(r_[m, S + 1]) & 0xFFFFFFFF
        if (m0 & 0xFF) not in allowed or (int(w_[m, 5 * S + 1]) & 0xFF) != RATED:
            continue
        n = ((m0 >> 8) & 0xFF, (m0 >> 16) & 0xFF)
        live = [j for j in range(S) if j % K < n[j // K] and 0 <= int(r_[m, j]) < P]
        for ja in live:
            a = int(r_[m, ja])
            if keep is not None and a not in keep:
                continue
            for jb in live:
                b = int(r_[m, jb])
                if ja == jb or a == b:
                    continue
                row = out.setdefault((a, b), [0, 0, 0, 0])
                o = 0 if ja // K == jb // K else 2
                row[o] += 1
                row[o + 1] += 1 if m1 & (1 << (ja // K)) else 0
    return out


def table_of(d):
    """(keys int64 [U] ascending, counts int32 [U, 4]) of an oracle dict."""
    pairs = sorted(d)
    keys = torch.tensor([(a << 32) | b for a, b in pairs], dtype=torch.int64).reshape(-1)
    counts = torch.tensor([d[p] for p in pairs], dtype=torch.int32).reshape(-1, 4)
    return keys, counts


# ------------------------------------------------------------------ windows
def random_window(K, M, P, seed, winners=(1, 2), other=0.0, ids=None):
    """M matches of random players (of ``ids``, default [0, P)) on random modes with ``meta1``
    drawn from ``winners``; ``other``: the share of matches that are not rated; some matches
    are short-handed."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda hi, *shape: torch.randint(hi, shape, generator=g)  # noqa: E731
    pool = torch.arange(P) if ids is None else torch.tensor(ids)
    matches = []
    for m in range(M):
        st = RATED
        if float(torch.rand((), generator=g)) < other:
            st = [AFK, INVALID_ROSTERS, 3, 7, 255][int(ri(5))]
        short = int(ri(8)) == 0
        matches.append({"ids": pool[ri(len(pool), 2 * K)].tolist(), "mode": int(ri(6)),
                        "n0": K - 1 if short else K, "n1": K, "meta1": winners[int(ri(len(winners)))], "status": st})
    return CC.window(K, matches)


HAND_P = 11


def hand_built(K):
    """P = 11: a full match, a short-handed one, ids -1, P and far above P in occupied slots,
    an unsupported mode and a mode outside the mask, every status other than rated, both
    winner bits and neither, and a player aliased into two and into all slots."""
    S = 2 * K
    full = list(range(S))
    ms = [{"ids": full, "meta1": 1}, {"ids": full, "meta1": 2, "mode": 0},
          {"ids": full, "n0": K - 1, "n1": K, "meta1": 1},
          {"ids": [-1] + full[1:]}, {"ids": full[:-1] + [HAND_P]}, {"ids": [2 ** 31 - 1] + full[1:]},
          {"ids": [-5, 100] * K, "meta1": 3},
          {"ids": full, "mode": 255, "status": 3}, {"ids": full, "mode": 255}, {"ids": full, "mode": 6},
          {"ids": full, "mode": 4, "meta1": 2}]  # 5v5_casual: outside the mask of the case
    ms += [{"ids": full, "status": st} for st in (AFK, INVALID_ROSTERS, 3, 4, 5, 6, 7, 8, 255)]
    ms += [{"ids": full, "meta1": 3}, {"ids": full, "meta1": 0}, {"ids": full[::-1], "meta1": 3}]
    ms += [{"ids": [3] * S, "meta1": 1}, {"ids": [3] + full[1:-1] + [3], "meta1": 2},
           {"ids": ([3, 3] + full[2:]) if K > 1 else [3, 8], "meta1": 1}]
    return CC.window(K, ms)


HAND_MODES = ("casual", "ranked", "blitz", "br")
PLANT = {"trader": (7, 8), "duo": (20, 21)}


def planted_window():
    """3v3, 100 players: random matches of the players from 30 up, 60 matches in which 7 beats 8
    (win trading) and 80 in which 20 and 21 share a roster (a duo)."""
    g = torch.Generator().manual_seed(77)
    ri = lambda lo, hi, n: (torch.randint(hi - lo, (n,), generator=g) + lo).tolist()  # noqa: E731
    ms = [{"ids": ri(30, 100, 6), "meta1": 1 + m % 2} for m in range(700)]
    for m in range(60):
        o = ri(30, 100, 4)
        ms.insert(11 * m, {"ids": [7, o[0], o[1], 8, o[2], o[3]], "meta1": 1})
    for m in range(80):
        o = ri(30, 100, 4)
        ms.insert(9 * m + 3, {"ids": [o[0], o[1], o[2], 21, o[3], 20], "meta1": 1 + m % 3 // 2})
    return CC.window(3, ms)


WIDE = {"p1": 1, "pow2": 256, "pow2-1": 255, "b16": (1 << 16) + 300, "b24": (1 << 24) + 300, "max": (1 << 31) - 1}
SYM = {3: (3, 2000, 150), 5: (5, 2000, 150)}  # K, M, P of the random windows of the symmetries
CUT = (3, 660, 60)


@functools.lru_cache(maxsize=None)
def case(name):
    """(rec, rows, P, options of PairTable) of a named case, built once."""
    kind, _, arg = name.partition(":")
    one = lambda a, b, n, w=None: [{"ids": [a, b], "meta1": (m % 4 if w is None else w)}  # noqa: E731
                                   for m in range(n)]
    if kind == "hand":
        return hand_built(int(arg)) + (HAND_P, {"modes": HAND_MODES})
    if kind == "run":  # run:n -- one pair in every match: the runs (0, 1) and (1, 0) of n entries
        return CC.window(1, one(0, 1, int(arg))) + (3, {})
    if kind == "edge_a":  # the run (0, 1) ends on a tile edge; next comes (0, 2): same a, another b
        return CC.window(1, one(0, 1, TILE) + one(0, 2, 5)) + (3, {})
    if kind == "edge_b":  # the run (0, 5) ends on a tile edge; next comes (1, 5): another a, the same b
        return CC.window(1, one(0, 5, TILE) + one(1, 5, 5)) + (6, {})
    if kind == "long":  # a run that starts inside a tile and covers more than two whole ones
        return CC.window(1, one(0, 1, 5) + one(0, 2, 3 * TILE + 7) + one(3, 4, 9)) + (5, {})
    if kind == "wide":  # wide:name -- ids up to P - 1: the sorts take 1 to 4 passes per key
        P = WIDE[arg]
        ids = sorted({p for p in (0, 1, 2, 70, 255, 256, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1,
                                  P - 3, P - 2, P - 1, P, P + 1) if 0 <= p < 2 ** 31})
        if P == 1:
            ids = [0, 0, 1, 2]
        return random_window(2, 60, P, seed=P % 1009, ids=ids, winners=(0, 1, 2, 3)) + (P, {})
    if kind == "filter":
        return random_window(3, 400, 45, seed=3, other=0.2) + (45, {"players": (0, 7, 31, 44)})
    if kind == "nobody":
        return random_window(3, 50, 45, seed=4) + (45, {"players": ()})
    if kind == "sym":  # sym:K:winners -- winners "12": exactly one winner bit in every match
        K, w = arg.split(":")
        K, M, P = SYM[int(K)]
        return random_window(K, M, P, seed=40 + K, winners=tuple(int(c) for c in w), other=0.1) + (P, {})
    if kind == "cut":
        K, M, P = CUT
        return random_window(K, M, P, seed=8, winners=(0, 1, 2, 3), other=0.2) + (P, {})
    if kind == "planted":
        return planted_window() + (100, {})
    raise KeyError(name)


HAND_CASES = ["hand:%d" % K for K in (1, 2, 3, 4, 5)]
RUN_CASES = ["run:%d" % n for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 3)] + ["edge_a", "edge_b", "long"]
WIDE_CASES = ["wide:" + n for n in WIDE]
OTHER_CASES = ["filter", "nobody", "sym:3:012", "sym:3:12", "sym:5:012", "sym:5:12", "cut", "planted"]


@functools.lru_cache(maxsize=None)
def oracle(name):
    rec, rows, P, opt = case(name)
    return pairs_dict(rec, rows, P, opt.get("modes"), opt.get("players"))


@functools.lru_cache(maxsize=None)
def expected(name):
    return table_of(oracle(name))


def run(name, device, cuts=(), **kw):
    """The table of a case on ``device``, its window added in one piece or cut at ``cuts``."""
    rec, rows, P, opt = case(name)
    table = PairTable(P, device, **dict(opt, **kw))
    edges = [0, *cuts, rec.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        table.add(rec[a:b].to(device), rows[a:b].to(device))
    return table


@functools.lru_cache(maxsize=None)
def host_table(name):
    t = run(name, "cpu")
    return t.keys, t.counts


def same(table, want, what=""):
    keys, counts = table.keys, table.counts
    assert keys.dtype == torch.int64 and keys.dim() == 1 and counts.dtype == torch.int32
    assert tuple(counts.shape) == (keys.shape[0], 4)
    assert torch.equal(keys.cpu(), want[0]), (what, keys.shape, want[0].shape)
    bad = (counts.cpu() != want[1]).any(dim=1).nonzero().reshape(-1)[:5].tolist()
    assert torch.equal(counts.cpu(), want[1]), (what, bad, counts.cpu()[bad].tolist(), want[1][bad].tolist())


def check_case(name, device):
    table = run(name, device)
    assert table.keys.device.type == torch.device(device).type == table.counts.device.type
    same(table, expected(name), name)
    if torch.device(device).type != "cpu":
        same(table, host_table(name), name + " (host mirror)")
    return table


# ------------------------------------------------------------------ checks
def check_hand_built(K, device):
    table = check_case("hand:%d" % K, device)
    d = oracle("hand:%d" % K)
    names = ("with_games", "with_wins", "vs_games", "vs_wins")
    assert d and all(a != b and 0 <= a < HAND_P and 0 <= b < HAND_P for a, b in d)  # no self row, nobody out of range
    # slots 0 and 2K - 1 meet as opponents in the two plain matches, under both winner bits (twice, once
    # reversed) and under neither
    got = table.pair(0, 2 * K - 1)
    assert got == dict(zip(names, d[(0, 2 * K - 1)])) and got["vs_games"] >= 5 and got["with_games"] == 0
    back = table.pair(2 * K - 1, 0)
    assert 0 < got["vs_wins"] < got["vs_games"] == back["vs_games"]
    # both bits are a win for either side (twice), neither bit for nobody (once)
    assert got["vs_wins"] + back["vs_wins"] == got["vs_games"] + 2 - 1
    if K > 1:  # the aliased player is counted per slot: one match puts it on both sides of player 1
        assert d[(3, 1)][0] >= 1 and d[(3, 1)][2] >= 1 and d[(1, 3)][2] >= 1


def check_guarded_bitmap(device):
    """Ids -1, P and beyond in occupied slots under a filter whose bitmap lies between guard
    words with every bit set, as are the bits from P up of its last word: an id probed
    outside [0, P) would make a row."""
    for K in (1, 3):
        rec, rows, P, opt = case("hand:%d" % K)
        players = (0, 3, 8)
        table = PairTable(P, device, players=players, **opt)
        words = table.bitmap.numel()
        big = torch.full((words + 8,), -1, dtype=torch.int32, device=device)
        big[4:4 + words] = table.bitmap | torch.tensor(-1 << P, dtype=torch.int32, device=device)
        table.bitmap = big[4:4 + words]
        table.add(rec.to(device), rows.to(device))
        want = pairs_dict(rec, rows, P, opt["modes"], players)
        assert K == 1 or want
        same(table, table_of(want), "guarded %d" % K)


def check_run_edges(name, device):
    check_constants()
    table = check_case(name, device)
    if name.startswith("run:"):
        n = int(name.split(":")[1])
        assert table.keys.tolist() == [1, 1 << 32] and table.counts[:, 2].tolist() == [n, n]
        # roster 0 carries the winner bit in the matches with meta1 1 and 3, roster 1 with 2 and 3
        assert table.counts[0].tolist() == [0, 0, n, (n + 2) // 4 + n // 4]
    if name == "edge_b":
        assert (table.keys >> 32).tolist() == [0, 1, 5, 5] and table.counts[:, 2].tolist() == [TILE, 5, TILE, 5]
    if name == "edge_a":
        assert (table.keys & 0xFFFFFFFF).tolist() == [1, 2, 0, 0] and table.counts[:, 2].tolist() == [TILE, 5, TILE, 5]


def check_cut_invariance(device):
    """One history as 1, 3 and 11 windows, and with ``max_entries`` forced small: more than 8
    segments, so the eager compaction runs."""
    K, M, P = CUT
    want = expected("cut")
    assert want[0].numel() > TILE  # the compaction walks more than one tile
    same(run("cut", device), want, "one window")
    same(run("cut", device, (200, 201)), want, "three windows")
    eleven = run("cut", device, tuple(range(60, M, 60))[:10])
    assert 1 <= len(eleven._segments) <= 8  # compacted on the way
    same(eleven, want, "eleven windows")
    small = run("cut", device, max_entries=ENTRIES[K] * 40 + 7)  # 40 matches per call: 17 calls
    same(small, want, "small max_entries")
    empty = PairTable(P, device)
    assert empty.keys.shape == (0,) and empty.counts.shape == (0, 4)
    rec, rows, _, _ = case("cut")
    empty.add(rec[:0].to(device), rows[:0].to(device))
    assert empty.keys.numel() == 0 and empty.pair(1, 2)["vs_games"] == 0


def check_symmetries(K, device):
    for winners, strict in (("012", False), ("12", True)):
        name = "sym:%d:%s" % (K, winners)
        table = check_case(name, device)
        d = oracle(name)
        keys, counts = table.keys.cpu(), table.counts.cpu().to(torch.int64)
        a, b = keys >> 32, keys & 0xFFFFFFFF
        mirror = torch.searchsorted(keys, (b << 32) | a)
        assert torch.equal(keys[mirror], (b << 32) | a)  # (b, a) is a row whenever (a, b) is
        other = counts[mirror]
        assert torch.equal(counts[:, :2], other[:, :2])  # with_* is symmetric
        assert torch.equal(counts[:, 2], other[:, 2])    # vs_games is symmetric
        both = counts[:, 3] + other[:, 3]
        # a match with neither winner bit is a win for nobody (one with both bits would be a win for either
        # side, which the hand-built windows hold)
        assert bool((both == counts[:, 2]).all() if strict else (both <= counts[:, 2]).all())
        assert strict or bool((both < counts[:, 2]).any())
        assert int(counts[:, 0].sum()) == sum(v[0] for v in d.values())
        assert int(counts[:, 0].sum() + counts[:, 2].sum()) == sum(v[0] + v[2] for v in d.values()) > TILE


def check_repeatable(name, device):
    first = run(name, device)
    again = run(name, device)
    assert torch.equal(first.keys, again.keys) and torch.equal(first.counts, again.counts)


def _ranked(d, p, col, by, min_games):
    """The oracle's partners of p: (player, games, wins), best first, ties by partner id."""
    rows = [(b, v[col], v[col + 1]) for (a, b), v in d.items() if a == p and v[col] >= max(1, min_games)]
    score = (lambda r: r[1]) if by == "games" else (lambda r: r[2] / r[1])
    return sorted(rows, key=lambda r: (-score(r), r[0]))


def check_queries(device):
    table = check_case("planted", device)
    d = oracle("planted")
    names = ("with_games", "with_wins", "vs_games", "vs_wins")
    (ta, tb), (da, db) = PLANT["trader"], PLANT["duo"]
    assert table.pair(ta, tb) == dict(zip(names, d[(ta, tb)])) == dict(zip(names, (0, 0, 60, 60)))
    assert table.pair(tb, ta) == dict(zip(names, (0, 0, 60, 0)))
    assert table.pair(da, db)["with_games"] == 80 and table.pair(da, 7) == dict.fromkeys(names, 0)
    for p in (ta, da, 55, 99):
        for relation, col in (("with", 0), ("against", 2)):
            for by in ("games", "win_rate"):
                for min_games, top in ((1, 10), (2, 4), (3, 1000)):
                    got = table.partners(p, relation, top=top, min_games=min_games, by=by)
                    want = _ranked(d, p, col, by, min_games)[:top]
                    assert list(zip(*(got[k].cpu().tolist() for k in ("player", "games", "wins")))) == want, \
                        (p, relation, by, min_games)
    assert len({v[2] for (a, b), v in d.items() if a == 55}) < sum(1 for a, b in d if a == 55)  # ties exist
    assert table.partners(ta, "against", top=1)["player"].tolist() == [tb]
    assert table.partners(da, "with", top=1)["player"].tolist() == [db]
    assert table.n_partners(ta) == sum(1 for a, b in d if a == ta)
    duos = {k: v.cpu().tolist() for k, v in table.duos(10).items()}
    want = sorted(((a, b, v[0], v[1]) for (a, b), v in d.items() if a < b and v[0] >= 10), key=lambda r: (-r[2], r[0], r[1]))
    assert list(zip(duos["a"], duos["b"], duos["games"], duos["wins"])) == want and want[0][:3] == (da, db, 80)
    sus = {k: v.cpu().tolist() for k, v in table.suspects(5, 0.9).items()}
    want = sorted(((a, b, v[2], v[3]) for (a, b), v in d.items() if v[2] >= 5 and v[3] / v[2] >= 0.9),
                  key=lambda r: (-r[2], r[0], r[1]))
    assert list(zip(sus["a"], sus["b"], sus["games"], sus["wins"])) == want and want[0] == (ta, tb, 60, 60)
    for bad in (lambda: table.pair(0, 100), lambda: table.partners(-1), lambda: table.partners(1, "near"),
                lambda: table.partners(1, by="luck")):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("a bad query was accepted")


def arena_window(spec, arena):
    """(rec, rows) of the whole history of a one-rank arena, on the CPU."""
    rec = make_stream(spec.stream_spec(), spec.total_matches, spec.players, K=spec.team_size)
    return rec, arena.filled_rows().cpu()


def check_arena_pairs(spec, device):
    from analyzer_amd.runtime.rerate import rerate_resident, stream_records

    _, _, arena = rerate_resident(spec, device, free_bytes=RC.FREE)
    rec_of = stream_records(spec, device)
    rec, rows = arena_window(spec, arena)
    table = arena.pairs(spec.players, rec_of)
    same(table, table_of(pairs_dict(rec, rows, spec.players)), "arena")
    assert int(table.counts[:, 0].sum()) > spec.total_matches  # most matches are rated
    ranked = arena.pairs(spec.players, rec_of, modes=("ranked",), players=(5, 7))
    same(ranked, table_of(pairs_dict(rec, rows, spec.players, ("ranked",), (5, 7))), "arena, filtered")
    return arena, table


def check_cli(device, *extra):
    """``rerate --pairs 5,7`` against ``arena.pairs(...).partners``."""
    from analyzer_amd.runtime.rerate import RerateSpec, rerate_resident, stream_records

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    ok = subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--matches", "900", "--players", "120",
                         "--window", "400", "--records", "resident", "--pairs", "5,7", *extra],
                        capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"pairs"')]
    assert [ln["pairs"] for ln in lines] == [5, 7]
    spec = RerateSpec(total_matches=900, players=120, team_size=3, window=400, seed=2024)
    _, _, arena = rerate_resident(spec, device, free_bytes=RC.FREE)
    table = arena.pairs(120, stream_records(spec, device))
    for line in lines:
        p = line["pairs"]
        assert line["partners"] == table.n_partners(p) > 0 and line["rank"] == 0
        for relation in ("with", "against"):
            cols = {k: v.cpu().tolist() for k, v in table.partners(p, relation, top=5).items()}
            assert line[relation] == [{"player": q, "games": g, "wins": w}
                                      for q, g, w in zip(cols["player"], cols["games"], cols["wins"])]
            assert len(line[relation]) == 5
    return lines
