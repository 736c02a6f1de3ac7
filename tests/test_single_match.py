"""One match at a time against a 50-digit oracle, at the numeric edges the stream
generators never reach: |t| from 0 to ~40 (every documented error regime of
csrc/rate_dev.h ``vw_pair``, the upset branch, the pdf underflow), sigma from 1 to 2000,
mode tracks far from the shared track, the error statuses with their "publish the
untouched values" path, the seeding edges and players repeated inside a match.

Cases, oracle and the per-element error budget: single_match_cases.py; derivation and
measured worst ratios: docs/ARCHITECTURE.md "Single-match error budget".  The CPU tests
check the fp64 host mirror and a numpy-fp32 transcription of ``rate_pair`` against the
same oracle and budget as the ``gpu`` tests check the device."""
import copy

import numpy as np
import pytest
import torch

from analyzer_amd.models.match_rater import trueskill_seed
from analyzer_amd.ops.rate import ERR_NUMERIC, ERR_SEED, ERR_SIGMA, RATED, BatchRater
from analyzer_amd.runtime.objects import Player

import single_match_cases as C
from engine_parity import object_run
from test_rate_dev_vw import _coefficients, _vw32

KS = (1, 2, 3, 4, 5)


def rate_on(device, roster, rec, K, **kw):
    """(result, roster after, rater) of one launch on ``device`` (the fp64 host mirror on
    the CPU); the device launch must raise no executor flag."""
    br = BatchRater(host_fp64=True)
    roster = roster.to(device)
    res = br.rate(roster, rec.to(device), K, **kw)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
        assert br.error_flags(device).cpu().tolist() == [0, 0, 0]
    return res, roster, br


# ------------------------------------------------------------------ the grid
def check_grid_within_budget(K, device, what):
    roster, rec, base, cases = C.grid_window(K)
    res, after, _ = rate_on(device, roster, rec, K)
    C.assert_rated(res)
    orc, rows = C.grid_oracle(K), C.both_copies(K)
    worst = C.assert_within_budget(C.result_fields(res), orc, C.grid(K), rows, "%s K=%d records" % (what, K))
    # the roster after the window: every player played once, so it holds the posteriors
    stored = C.roster_fields(after, cases, base)
    stored["delta"], stored["quality"] = C.result_fields(res)["delta"], C.result_fields(res)["quality"]
    C.assert_within_budget(stored, orc, C.grid(K), rows, "%s K=%d roster" % (what, K))
    return worst


@pytest.mark.parametrize("K", KS)
def test_host_fp64_within_budget(K):
    check_grid_within_budget(K, "cpu", "fp64 host")


def emulate_fp32(cases, coefficients=None, vw=_vw32):
    """numpy-fp32 transcription of rate_dev.h ``rate_pair``: IEEE division, sqrt and exp2
    in place of the hardware approximations, the team sums in slot order."""
    f = np.float32
    p, q, k = coefficients or _coefficients()
    beta2, tau2 = f(C.BETA) * f(C.BETA), f(C.TAU) * f(C.TAU)
    M, S = len(cases), 2 * cases[0].K
    out = {name: np.full((M, S), np.nan, dtype=f) for name in C.FIELDS}
    out["quality"] = np.zeros(M, dtype=f)
    with np.errstate(all="ignore"):
        for i, c in enumerate(cases):
            pr, slots = C.priors(c), c.slots()
            n = len(slots)
            tie, win0 = c.outcome == "tie", c.outcome != "win1"
            pm = np.array([[pr[j][0], pr[j][2]] for j in slots], dtype=f)
            ps = np.array([[pr[j][1], pr[j][3]] for j in slots], dtype=f)
            lsg = np.array([[1.0 if (j < c.K) == win0 else -1.0] for j in slots], dtype=f)
            s2 = ps * ps + tau2
            x01, x23 = np.zeros(2, dtype=f), np.zeros(2, dtype=f)
            for r in range(n):
                x01 = x01 + s2[r]
                x23 = x23 + lsg[r] * pm[r]
            nb2 = f(n) * beta2
            c2 = x01 + nb2
            rc = f(1) / np.sqrt(c2)
            t = x23 * rc
            v, w = (a.astype(f) for a in vw(t, p, q, k))
            if tie:
                v, w = -t, np.ones(2, dtype=f)
            nm = pm + s2 * ((v * rc) * lsg)
            ns = np.sqrt(s2 - s2 * s2 * (w * (rc * rc)))
            rd = f(1) / (c2[1] - f(n) * tau2)
            out["quality"][i] = np.sqrt(nb2 * rd * np.exp2(x23[1] * x23[1] * rd * f(-1.4426950408889634)))
            assert nm.dtype == f and ns.dtype == f and out["quality"].dtype == f
            for r, j in enumerate(slots):
                out["s_mu"][i, j], out["m_mu"][i, j] = nm[r]
                out["s_sig"][i, j], out["m_sig"][i, j] = ns[r]
                out["delta"][i, j] = (nm[r, 0] - ns[r, 0]) - (pm[r, 0] - ps[r, 0])
    return out


@pytest.mark.parametrize("K", KS)
def test_device_formula_emulation_within_budget(K):
    """The formula of ``rate_pair`` alone, with exactly rounded fp32 operations, fits
    the budget: what the device may add is the hardware approximations' 1 ulp each."""
    C.assert_within_budget(emulate_fp32(C.grid(K)), C.grid_oracle(K), C.grid(K), None, "fp32 emulation K=%d" % K)


def _factor_graph_cases():
    picks = []
    for K, want in ((1, [("tie", None), ("win1", -18.0), ("win0", 3.0), ("win0", 13.5), ("win1", -42.0)]),
                    (3, [("win0", 0.0), ("win1", -5.0), ("tie", None)]), (5, [("win1", 1.0), ("win0", 6.0)])):
        t = C.grid_oracle(K)["t"][:, 0]
        for n1 in sorted({K, max(1, K - 1)}):
            for outcome, target in want:
                idx = [i for i, c in enumerate(C.grid(K)) if c.outcome == outcome and c.n1 == n1]
                i = idx[len(idx) // 2] if target is None else min(idx, key=lambda i: abs(t[i] - target))
                picks.append((K, i))
    return picks  # fifteen, uneven teams among them


def test_oracle_agrees_with_factor_graph():
    """The closed-form oracle equals the expectation-propagation factor graph (the
    computation the reference runs) at 50 digits: ``TrueSkill(backend="mpmath").rate``
    to fp64 (it returns floats), and the ``run_ep`` call it makes to 1e-30 (ties: at 100
    working digits, see below)."""
    mp = C._mp()
    from analyzer_amd.models.factor_graph import run_ep
    from analyzer_amd.models.gaussian import Rating
    from analyzer_amd.models.trueskill import TrueSkill

    env = TrueSkill(backend="mpmath", mu=1500, sigma=1000, beta=C.BETA, tau=C.TAU, draw_probability=0)
    picks = _factor_graph_cases()
    seen = set()
    assert len(picks) >= 12
    for K, i in picks:
        c = C.grid(K)[i]
        t = C.grid_oracle(K)["t"][i, 0]
        seen |= {c.outcome, "uneven" if c.n1 != c.n0 else "even", "upset" if c.outcome != "tie" and t < -15 else ""}
        pr, exp = C.priors(c), C.shared_track_mp(c)
        teams = [[j for j in c.slots() if (j < K) == (side == 0)] for side in (0, 1)]
        w0, w1 = c.winners()
        ranks = [int(not w0), int(not w1)]
        order = sorted(range(2), key=lambda k: ranks[k])

        def graph():
            groups = [[Rating(mp.mpf(pr[j][0]), mp.mpf(pr[j][1])) for j in team] for team in teams]
            ep = run_ep([groups[k] for k in order], [ranks[k] for k in order], [[1] * len(groups[k]) for k in order],
                        beta=mp.mpf(C.BETA), tau=mp.mpf(C.TAU), draw_probability=mp.mpf(0), num=env.num)
            return env.rate(groups, ranks), ep

        def worst(ep):
            return max(max(abs(mu / exp[j][0] - 1), abs(sigma / exp[j][1] - 1))
                       for pos, k in enumerate(order) for (mu, sigma), j in zip(ep[pos], teams[k]))

        rated, ep = graph()
        if c.outcome == "tie":
            # the graph rates a tie through a draw margin of ppf(0.5) ~ -1e-34 (models/special.py
            # make_erfcinv), whose cdf difference cancels ~34 of the 50 digits: measured 3.6e-19
            # here.  With 100 working digits that rounding is gone and the graph is the limit.
            assert worst(ep) < mp.mpf("1e-15"), (c.label, t)
            with mp.workdps(100):
                ep = graph()[1]
                assert worst(ep) < mp.mpf("1e-30"), (c.label, t)
        else:
            assert worst(ep) < mp.mpf("1e-30"), (c.label, t)
        for k in range(2):
            for r, j in zip(rated[k], teams[k]):
                assert r.mu == pytest.approx(float(exp[j][0]), rel=3e-16, abs=0)
                assert r.sigma == pytest.approx(float(exp[j][1]), rel=3e-16, abs=0)
    assert {"tie", "win0", "win1", "uneven", "even", "upset"} <= seen


# ------------------------------------------------------------------ hand-built cases
def _ordinary(K, rng, n1=None, outcome="win0", mode=1, stored_mode=True, **kw):
    S = 2 * K
    mu = [C.f32(rng.uniform(1200, 2400)) for _ in range(S)]
    sig = [C.f32(rng.uniform(80, 400)) for _ in range(S)]
    mmu = [C.f32(m + rng.uniform(-400, 400)) if stored_mode else None for m in mu]
    msig = [C.f32(rng.uniform(80, 400)) if stored_mode else None for _ in range(S)]
    return C.Case(K, mu, sig, mmu, msig, K if n1 is None else n1, outcome, mode=mode, **kw)


ERROR_CASES = (  # name, slot, what to store there, expected status
    ("shared sigma 0", 0, dict(sig=0.0), ERR_SIGMA),
    ("shared sigma NaN", 1, dict(sig=float("nan")), ERR_SIGMA),
    ("mode sigma 0", 2, dict(msig=0.0), ERR_SIGMA),
    ("stored mu +inf", 3, dict(mu=float("inf")), ERR_NUMERIC),
    ("stored sigma +inf", 4, dict(sig=float("inf")), ERR_NUMERIC),
    ("no rating, no tier, no rank points", 5, dict(mu=None, attrs=(None, None, None)), ERR_SEED),
    ("no rating, tier 30", 5, dict(mu=None, attrs=(None, None, 30.0)), ERR_SEED),
    ("no rating, tier 7.5", 0, dict(mu=None, attrs=(0.0, None, 7.5)), ERR_SEED),
    ("mode sigma 0, followed in another mode", 4, dict(msig=0.0), ERR_SIGMA),
)
OTHER_MODE = len(ERROR_CASES) - 1  # this one's successor is its own six players, in a mode they never played


def error_window():
    """K = 3: the defective matches E, then per E a match F of its five sound players
    and one fresh player in the defective slot, then E's six players again (G).  A match
    that holds a player with a defective shared track, or none and no seed, can never
    rate (the stored state stays as it is), so F is the successor that must come out
    RATED from the untouched priors, and G shows the defective player's own successor
    was released too.  Only a defective mode track leaves the same six players a match
    that rates -- in another mode: the last case's F."""
    K, S = 3, 6
    rng = np.random.default_rng(9)
    n = len(ERROR_CASES)
    E, F, G = [], [], []
    for i, (name, slot, bad, _) in enumerate(ERROR_CASES):
        ok = _ordinary(K, rng, outcome=C.OUTCOMES[i % 3], label=dict(case=name))
        e = copy.deepcopy(ok)
        for key, val in bad.items():
            if key == "attrs":
                e.attrs = {slot: val}
            else:
                getattr(e, key)[slot] = val
        if e.mu[slot] is None:
            e.sig[slot] = None
        E.append(e)
        f = copy.deepcopy(ok)  # the sound five keep E's priors; ``slot`` is a fresh player's
        f.same_as, f.outcome = i, C.OUTCOMES[(i + 1) % 3]
        if i == OTHER_MODE:
            f.mode, f.mmu, f.msig = 2, [None] * S, [None] * S
        else:
            f.fresh = {slot: 3 * n * S + i}
        F.append(f)
        g = copy.deepcopy(e)
        g.same_as = i
        G.append(g)
    return E + F + G, n


def check_error_statuses(device):
    cases, n = error_window()
    roster, rec, base = C.build_window(cases, extra_players=n)
    before = roster.state.clone()
    res, after, _ = rate_on(device, roster, rec, 3)
    status = res.status.cpu().numpy().astype(int)
    expect = [c[3] for c in ERROR_CASES]
    assert list(status[:n]) == expect == [5, 5, 5, 7, 7, 4, 4, 4, 5] and list(status[2 * n:]) == expect
    assert (status[n:2 * n] == RATED).all()
    got = C.result_fields(res)
    for k in C.FIELDS + ("quality",):
        assert np.isnan(got[k][:n]).all() and np.isnan(got[k][2 * n:]).all(), k
    # the successors rated from the original priors of the five sound players: the error
    # path published the untouched values and released them
    F = cases[n:2 * n]
    C.assert_within_budget({k: v[n:2 * n] for k, v in got.items()}, C.oracle(F), F, None,
                           "%s error follow-ups" % device)
    # the defective players' stored values are still the original bits (OTHER_MODE's player
    # was rated by its F on the shared and another mode's track: its defective track is)
    bits = lambda st: st[:, 0::2].clone().view(torch.int32)  # noqa: E731
    bad = [int(base[i]) + ERROR_CASES[i][1] for i in range(n)]
    now, was = bits(after.state.cpu()[bad]), bits(before[bad])
    assert torch.equal(now[:OTHER_MODE], was[:OTHER_MODE]) and torch.equal(now[OTHER_MODE, 4:6], was[OTHER_MODE, 4:6])
    assert not torch.equal(now[OTHER_MODE, 0:2], was[OTHER_MODE, 0:2])
    return res


def test_host_error_statuses_and_untouched_state():
    check_error_statuses("cpu")


SEED_EDGES = (  # (ranked, blitz, tier) of the unrated player
    (0.0, 2500.0, None), (0.0, 0.0, 15.0), (100.0, 2500.0, None), (2500.0, 100.0, 3.0),
    (None, None, -1.0), (None, None, 0.0), (None, None, 29.0),
)


def check_seed_edges(device):
    K, S = 3, 6
    rng = np.random.default_rng(4)
    cases, slot_of = [], []
    for i, attrs in enumerate(SEED_EDGES):
        c = _ordinary(K, rng, outcome=C.OUTCOMES[i % 3], mode=i % 6, label=dict(attrs=attrs))
        j = i % S
        c.mu[j], c.sig[j], c.attrs = None, None, {j: attrs}
        if i % 2 == 0:  # the mode track falls back to the seed as well
            c.mmu[j], c.msig[j] = None, None
        cases.append(c)
        slot_of.append(j)
    roster, rec, base = C.build_window(cases)
    first = torch.full_like(roster.state, float("nan")).to(device)
    res, after, _ = rate_on(device, roster, rec, K, first_prior=first)
    C.assert_rated(res)
    first = first.cpu().numpy().astype(np.float64)
    for i, (c, j) in enumerate(zip(cases, slot_of)):
        ranked, blitz, tier = c.attrs[j]
        mu, sig = trueskill_seed(Player(skill_tier=None if tier is None else int(tier), rank_points_ranked=ranked,
                                        rank_points_blitz=blitz), 500)
        p = int(base[i]) + j
        # the reference's seed, to the two fp32 roundings the stored prior takes (the
        # table entry or 2/3 sigma, then the sum)
        assert abs(first[p, 0] - mu) <= 2 * C.U * abs(mu) and abs(first[p, 2] - sig) <= C.U * sig, (c.label, first[p])
        c.seed = {j: (first[p, 0], first[p, 2])}
    got = C.result_fields(res)
    C.assert_within_budget(got, C.oracle(cases), cases, None, "%s seed edges" % device)
    for i, j in enumerate(slot_of):
        assert got["delta"][i, j] == 0.0


def test_host_seed_edges():
    check_seed_edges("cpu")


def alias_cases(K):
    rng = np.random.default_rng(40 + K)
    S = 2 * K
    own = list(range(S))
    two = [0, 0] + own[2:]                                  # one player in two slots of one team
    both = own[:K] + [0] + own[K + 1:]                      # one player on both teams
    three = [0, 0, 0] + own[3:]                             # one player in all three slots (K = 3: a whole team)
    whole = [0] * K + [K] * K                               # each team one player K times
    cases = []
    for i, players in enumerate((two, both, three, whole, three)):
        c = _ordinary(K, rng, outcome=C.OUTCOMES[i % 3], mode=(i + 1) % 6, stored_mode=i != 2, players=players,
                      n1=K - 1 if i == 4 else K, label=dict(alias=players))
        cases.append(c)
    return cases


def alias_oracle(K):
    """Oracle of the aliased cases, its semantics pinned by the per-object rater: every
    slot rates from the pre-match prior, a later slot's delta is against the earlier
    slot's posterior, the roster keeps the last slot's values."""
    cases = alias_cases(K)
    orc = C.oracle(cases)
    roster, rec, base = C.build_window(cases)
    ref = object_run(roster, rec, K)
    assert (ref["status"] == RATED).all()
    for k in C.FIELDS + ("quality",):
        np.testing.assert_allclose(ref[k], orc[k], rtol=1e-12, atol=1e-9, equal_nan=True, err_msg=k)
    last = {}
    for i, c in enumerate(cases):
        for j in c.slots():
            last[int(base[i]) + c.players[j]] = (i, j, 1 + c.mode)
    for p, (i, j, g) in last.items():
        exp = [orc["s_mu"][i, j], orc["s_sig"][i, j], orc["m_mu"][i, j], orc["m_sig"][i, j]]
        np.testing.assert_allclose([*ref["state"][p, 0], *ref["state"][p, g]], exp, rtol=2 * C.U)
    return cases, orc, last


def check_aliased(K, device):
    cases, orc, last = alias_oracle(K)
    roster, rec, base = C.build_window(cases)
    res, after, _ = rate_on(device, roster, rec, K)
    C.assert_rated(res)
    got = C.result_fields(res)
    C.assert_within_budget(got, orc, cases, None, "%s aliased K=%d" % (device, K))
    st = after.state.cpu().numpy()
    for p, (i, j, g) in last.items():  # the roster holds the last slot's record values
        assert [st[p, 0], st[p, 2], st[p, 4 * g], st[p, 4 * g + 2]] == \
            [got["s_mu"][i, j], got["s_sig"][i, j], got["m_mu"][i, j], got["m_sig"][i, j]]


@pytest.mark.parametrize("K", (3, 5))
def test_host_aliased_players(K):
    check_aliased(K, "cpu")


# ------------------------------------------------------------------ the device
@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_device_within_budget(gpu_device, K):
    """(a) Measured on MI355X: docs/ARCHITECTURE.md "Single-match error budget"."""
    check_grid_within_budget(K, gpu_device, "device")


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_device_copies_and_roster_bits(gpu_device, K):
    """(b) The grid's two copies (other lane groups, other chunks) give the same bits,
    and what a match publishes to the roster is what it records."""
    roster, rec, base, cases = C.grid_window(K)
    res, after, _ = rate_on(gpu_device, roster, rec, K)
    n = len(C.grid(K))
    got = {k: torch.from_numpy(v).view(torch.int32) for k, v in C.result_fields(res).items()}
    inv = torch.from_numpy(np.argsort(C.grid_perm(K)))
    for k, v in got.items():
        assert torch.equal(v[:n], v[n:][inv]), k
    stored = C.roster_fields(after, cases, base)
    for k, v in stored.items():
        assert torch.equal(torch.from_numpy(v).view(torch.int32), got[k]), k


@pytest.mark.gpu
def test_device_error_statuses_match_host(gpu_device):
    """(c)"""
    host, dev = check_error_statuses("cpu"), check_error_statuses(gpu_device)
    assert torch.equal(host.status, dev.status.cpu())


@pytest.mark.gpu
def test_device_seed_edges(gpu_device):
    """(d)"""
    check_seed_edges(gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("K", (3, 5))
def test_device_aliased_players(gpu_device, K):
    """(e)"""
    check_aliased(K, gpu_device)
