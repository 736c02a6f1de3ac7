"""Helpers of the ladder tests (test_ladder.py on the CPU, test_ladder_gpu.py on the device):
rosters, the oracle and the checks both suites share.

The oracle knows nothing of the sort key: an fp32 score, the ranked mask, and Python's
``sorted`` over ``(-float64(score + 0), id)``.
"""
import functools
import hashlib
import json

import numpy as np
import torch

from analyzer_amd.config import MODES
from analyzer_amd.ops.ladder import build_ladder

TRACKS = ("shared",) + MODES
TILE = 8192  # the radix sort's tile (csrc/radix_sort.hip)
SIZES = (0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
INF = float("inf")
NAN = float("nan")


def track_granule(name):
    return 0 if name == "shared" else 1 + MODES.index(name.replace("trueskill_", ""))


# ------------------------------------------------------------------ rosters
def empty_state(P):
    """All tracks NULL (NaN mu and sigma), zero tags: ``Roster.empty``'s state."""
    st = np.zeros((P, 32), dtype=np.float32)
    st[:, 0::2] = np.nan
    return st


def set_track(st, name, mu, sigma):
    g = 4 * track_granule(name)
    st[:, g] = np.asarray(mu, dtype=np.float32)
    st[:, g + 2] = np.asarray(sigma, dtype=np.float32)
    return st


@functools.lru_cache(maxsize=None)
def _random_state(P, seed):
    """Every track populated: a fifth NULL (half of those with a stored sigma), scores with
    ties (mu on a grid of 25, four sigmas), garbage in the spare granule."""
    rng = np.random.default_rng(seed)
    st = empty_state(P)
    for g in range(7):
        mu = (np.round(rng.normal(1500.0, 400.0, P) / 25.0) * 25.0).astype(np.float32)
        sg = rng.choice(np.array([50.0, 125.0, 250.0, 500.0], dtype=np.float32), P)
        null = rng.random(P) < 0.2
        mu[null] = np.nan
        sg[null & (rng.random(P) < 0.5)] = np.nan
        st[:, 4 * g], st[:, 4 * g + 2] = mu, sg
    st[:, 28:32] = rng.normal(0.0, 1e3, (P, 4)).astype(np.float32)
    return st


def random_state(P, seed=11):
    return _random_state(P, seed).copy()


def live_tags(st, seed=5):
    """The same roster with arbitrary bits, NaN patterns included, in every tag word
    (floats 1 and 3 of every granule), as after a device launch."""
    rng = np.random.default_rng(seed)
    out = st.copy()
    bits = out.view(np.uint32)
    tags = rng.integers(0, 1 << 32, (st.shape[0], 16), dtype=np.uint64).astype(np.uint32)
    nan = rng.random((st.shape[0], 16)) < 0.25  # quiet and signalling NaNs of both signs
    tags[nan] |= 0x7f800001
    bits[:, 1::2] = tags
    return out


SPECIALS = (
    (INF, 0.0), (-INF, 0.0),                 # +-inf
    (0.0, 0.0), (-0.0, 0.0), (5.0, 5.0),     # +0, -0 (ties with +0), 5 - 5
    (1e-40, 0.0), (-1e-40, 0.0),             # denormal scores
    (3e38, 0.0), (-3e38, 0.0), (3e38, -3e38),  # the last overflows to +inf
    (1.0, 3e38), (-5.0, 2.0), (-1234.5, 0.25),  # negative scores
    (INF, INF),                              # inf - inf: unranked
    (NAN, 1.0), (1.0, NAN), (NAN, NAN),      # NULL and half-NULL
    (1e-40, 1e-40), (2e-40, 1e-40),          # denormal arithmetic: +0 and 1e-40
    (1500.0, 250.0), (1250.0, 0.0),          # a plain tie
)


def special_state(P=3 * len(SPECIALS) + 7):
    """The special values on every track, each track rotated so that ties land on other ids."""
    st = empty_state(P)
    for g, name in enumerate(TRACKS):
        pairs = [SPECIALS[(i + 5 * g) % len(SPECIALS)] for i in range(P)]
        set_track(st, name, [p[0] for p in pairs], [p[1] for p in pairs])
    return st


# ------------------------------------------------------------------ oracle
def oracle(st, track, score="conservative", max_sigma=None):
    """(order int32 [R], score bits uint32 [R], rank int32 [P]) of one track of a numpy state."""
    g = 4 * track_granule(track)
    mu, sg = st[:, g].astype(np.float32), st[:, g + 2].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((mu - sg) if score == "conservative" else mu.copy()) + np.float32(0.0)
        assert s.dtype == np.float32
        bound = np.float32(INF if max_sigma is None else max_sigma)
        ranked = ~np.isnan(s) & (sg <= bound)
    ids = [i for i in range(st.shape[0]) if ranked[i]]
    order = np.array(sorted(ids, key=lambda i: (-float(s[i]), i)), dtype=np.int32)
    rank = np.full(st.shape[0], -1, dtype=np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32)
    return order, s[order].view(np.uint32), rank


def outputs(lad, track):
    """A built ladder's (order, score bits, rank) of a track as numpy arrays."""
    return (lad.order(track).cpu().numpy(), lad.score(track).cpu().numpy().view(np.uint32),
            lad.rank(track).cpu().numpy())


def assert_same(got, want, what):
    for name, a, b in zip(("order", "score bits", "rank"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s is %s %s, expected %s %s" % (
            what, name, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a, b), "%s: %s differs at %s" % (what, name, np.flatnonzero(a != b)[:8])


def check(st, device, tracks=TRACKS, score="conservative", max_sigma=None, what=""):
    """Build the ladder of numpy state ``st`` on ``device`` and hold it to the oracle --
    and, on a GPU, bit for bit to the host mirror.  Returns the ladder."""
    dev = torch.device(device)
    state = torch.from_numpy(st.copy()).to(dev)
    before = state.clone()
    lad = build_ladder(state, tracks, score=score, max_sigma=max_sigma)
    host = build_ladder(torch.from_numpy(st.copy()), tracks, score=score, max_sigma=max_sigma) \
        if dev.type != "cpu" else None
    assert torch.equal(state.view(torch.int32), before.view(torch.int32)), "the roster was written"
    for t in tracks:
        got = outputs(lad, t)
        label = "%s track %s P=%d" % (what, t, st.shape[0])
        assert lad.ranked(t) == got[0].shape[0] == got[1].shape[0]
        assert_same(got, oracle(st, t, score, max_sigma), label + " vs oracle")
        if host is not None:
            assert lad.ranked(t) == host.ranked(t)
            assert_same(got, outputs(host, t), label + " vs host mirror")
        assert np.array_equal(got[2][got[0]], np.arange(got[0].size)), label + ": rank[order[i]] != i"
    return lad


# ------------------------------------------------------------------ shared checks
def check_sizes(P, device):
    st = random_state(P)
    check(st, device, what="random")
    check(st, device, tracks=("shared", "blitz"), score="mu", what="random mu")


def check_live_tags(device):
    st = random_state(TILE + 1)
    tagged = live_tags(st)
    assert not np.array_equal(st.view(np.uint32)[:, 1::2], tagged.view(np.uint32)[:, 1::2])
    a, b = check(st, device, what="zero tags"), check(tagged, device, what="live tags")
    for t in TRACKS:
        assert_same(outputs(b, t), outputs(a, t), "live tags vs zero tags, track %s" % t)


def check_all_null(device):
    P = 65
    lad = check(empty_state(P), device, what="all NULL")
    for t in TRACKS:
        assert lad.ranked(t) == 0 and (lad.rank(t) == -1).all() and lad.rank(t).shape == (P,)
        assert all(x.numel() == 0 for x in lad.top(t, 5))
        rank, score, pct = lad.lookup(t, [0, 64])
        assert rank.tolist() == [-1, -1] and torch.isnan(score).all() and torch.isnan(pct).all()
        assert lad.cutoff(t, 0.01) != lad.cutoff(t, 0.01)


def check_all_tied(device):
    P = 3 * TILE + 5
    st = set_track(empty_state(P), "shared", np.full(P, 1500.0), np.full(P, 250.0))
    lad = check(st, device, tracks=("shared",), what="all tied")
    assert np.array_equal(lad.order("shared").cpu().numpy(), np.arange(P, dtype=np.int32))


def check_few_distinct(device):
    P = 2 * TILE + 1
    rng = np.random.default_rng(3)
    mu = rng.choice(np.array([-40.0, 0.0, 1e-40, 1500.0, 1525.0], dtype=np.float32), P)
    st = set_track(empty_state(P), "ranked", mu, np.zeros(P))
    lad = check(st, device, tracks=("ranked",), what="five scores")
    assert len(set(lad.score("ranked").cpu().numpy().view(np.uint32).tolist())) == 5


def check_specials(device):
    st = special_state()
    for score in ("conservative", "mu"):
        lad = check(st, device, score=score, what="specials " + score)
    lad = check(st, device, tracks=("shared",), what="specials")
    g = outputs(lad, "shared")
    # track 0 is not rotated: player i holds SPECIALS[i]
    pos_inf, zero, tiny, neg_tiny, inf_inf, null = 0, (2, 3, 4), 5, 6, 13, 14
    assert SPECIALS[tiny] == (1e-40, 0.0) and SPECIALS[neg_tiny] == (-1e-40, 0.0) and SPECIALS[inf_inf] == (INF, INF)
    rank = g[2]
    assert rank[pos_inf] == 0 and rank[inf_inf] == -1 and rank[null] == -1
    # +0, -0 and 5 - 5 tie and go by id; the denormals sit right around them
    assert rank[zero[0]] < rank[zero[1]] < rank[zero[2]]
    assert rank[tiny] < rank[zero[0]] and rank[neg_tiny] > rank[zero[2]]
    bits = dict(zip(g[0].tolist(), g[1].tolist()))
    assert bits[zero[1]] == 0 and bits[tiny] == int(np.float32(1e-40).view(np.uint32)) != 0
    assert bits[neg_tiny] == int(np.float32(-1e-40).view(np.uint32))


def check_max_sigma(device):
    bound = np.float32(250.0)
    up, down = np.nextafter(bound, np.float32(INF)), np.nextafter(bound, np.float32(-INF))
    sigma = np.array([bound, up, down, NAN, 0.0, INF, bound, up], dtype=np.float32)
    st = set_track(empty_state(8), "shared", np.arange(8, dtype=np.float32) * 10.0 + 1000.0, sigma)
    for score in ("conservative", "mu"):
        lad = check(st, device, tracks=("shared",), score=score, max_sigma=float(bound), what="max_sigma " + score)
        assert (lad.rank("shared").cpu() >= 0).tolist() == [True, False, True, False, True, False, True, False]
        # without a bound only the NaN sigma drops out (mu - inf = -inf is a score)
        free = check(st, device, tracks=("shared",), score=score, what="no bound " + score)
        assert (free.rank("shared").cpu() >= 0).tolist() == [True, True, True, False, True, True, True, True]
    big = random_state(TILE + 1)
    check(big, device, max_sigma=125.0, what="max_sigma 125")


def check_multi_track(device):
    st = random_state(TILE + 1, seed=23)
    state = torch.from_numpy(st).to(device)
    full = build_ladder(state, TRACKS)
    subset = build_ladder(state, ("5v5_ranked", "shared", "trueskill_blitz"))
    assert subset.tracks == ("shared", "blitz", "5v5_ranked")
    for t in TRACKS:
        one = build_ladder(state, (t,))
        assert_same(outputs(full, t), outputs(one, t), "seven tracks vs one, %s" % t)
        assert_same(outputs(full, t), oracle(st, t), "seven tracks vs oracle, %s" % t)
        if t in subset.tracks:
            assert_same(outputs(subset, t), outputs(one, t), "subset vs one, %s" % t)
    assert_same(outputs(subset, "trueskill_blitz"), outputs(subset, "blitz"), "both spellings")
    # a mode nobody played
    played = set_track(empty_state(65), "shared", np.arange(65.0), np.ones(65))
    lad = check(played, device, tracks=("shared", "br"), what="unplayed mode")
    assert lad.ranked("shared") == 65 and lad.ranked("br") == 0


def check_repeatable(device):
    st = random_state(3 * TILE + 5, seed=31)
    state = torch.from_numpy(st).to(device)
    attrs = torch.rand(st.shape[0], 4).to(device)
    keep_state, keep_attrs = state.clone(), attrs.clone()
    a, b = build_ladder(state, TRACKS), build_ladder(state, TRACKS)
    for t in TRACKS:
        assert_same(outputs(a, t), outputs(b, t), "two builds, %s" % t)
        assert a.ranked(t) == b.ranked(t)
    assert torch.equal(state.view(torch.int32), keep_state.view(torch.int32))
    assert torch.equal(attrs.view(torch.int32), keep_attrs.view(torch.int32))


def check_api(device):
    """top / lookup / cutoff against the plain outputs."""
    st = random_state(TILE - 1, seed=41)
    state = torch.from_numpy(st).to(device)
    lad = build_ladder(state, ("ranked",))
    order, bits, rank = oracle(st, "ranked")
    R = order.size
    assert lad.ranked("ranked") == R and lad.num_players == st.shape[0]
    ids, mu, sigma, score = (x.cpu().numpy() for x in lad.top("ranked", 7))
    assert np.array_equal(ids, order[:7]) and np.array_equal(score.view(np.uint32), bits[:7])
    assert np.array_equal(mu, st[order[:7], 8]) and np.array_equal(sigma, st[order[:7], 10])
    assert lad.top("ranked", 10 * R)[0].numel() == R
    unranked = int(np.flatnonzero(rank < 0)[0])
    probe = [int(order[0]), int(order[R // 2]), int(order[-1]), unranked]
    r, s, pct = (x.cpu().numpy() for x in lad.lookup("ranked", probe))
    assert r.tolist() == [0, R // 2, R - 1, -1] and pct.dtype == np.float64
    assert pct[:3].tolist() == [1.0, 1.0 - (R // 2) / R, 1.0 - (R - 1) / R] and np.isnan(pct[3]) and np.isnan(s[3])
    assert np.array_equal(s[:3].view(np.uint32), bits[[0, R // 2, R - 1]])
    for q in (0.0, 0.01, 0.5, 1.0):
        want = np.array(bits[min(int(q * R), R - 1)], dtype=np.uint32).view(np.float32)
        assert lad.cutoff("ranked", q) == float(want)


def check_cli(device, capsys):
    """The re-rate command line's ladder lines against build_ladder on the same run's roster."""
    from analyzer_amd.runtime import rerate

    args = ["--matches", "3000", "--players", "300", "--window", "1000", "--device", str(device),
            "--ladder", "shared,ranked", "--ladder-top", "5", "--ladder-rank", "7,123"]
    assert rerate.main(args) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 3 and "ladder" not in lines[0]
    spec = rerate.RerateSpec(total_matches=3000, players=300, window=1000)
    _, roster = rerate.run(spec, device)
    sha = hashlib.sha256(roster.state[:, 0::2].contiguous().cpu().numpy().tobytes()).hexdigest()
    assert sha == lines[0]["roster_sha256"]
    lad = build_ladder(roster, ("shared", "ranked"))
    for line, t in zip(lines[1:], ("shared", "ranked")):
        assert line["ladder"] == t and line["score"] == "conservative" and line["players"] == 300
        assert line["ranked"] == lad.ranked(t) > 5
        ids, mu, sigma, score = (x.cpu().tolist() for x in lad.top(t, 5))
        assert line["top"] == [{"rank": i, "player": ids[i], "mu": mu[i], "sigma": sigma[i], "score": score[i]}
                               for i in range(5)]
        rank, sc, pct = (x.cpu().tolist() for x in lad.lookup(t, [7, 123]))
        assert line["ranks"] == [{"player": p, "rank": rank[i], "score": sc[i], "percentile": pct[i]}
                                 for i, p in enumerate((7, 123))]
        assert all(r["rank"] >= 0 for r in line["ranks"])
    # without --ladder the output is the one result line, as before
    assert rerate.main(args[:8]) == 0
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]) == 1
