"""Shared cases of the through-time tests (test_through_time.py on the CPU,
test_through_time_gpu.py on the device): the oracle, the tolerance, the histories and the
checks that run the same way on either device.

The oracle is written from the model in the module docstring of ops/through_time.py, not from
csrc/: plain Python loops over chains and matches -- the sequential recursions and the Jacobi
schedule -- in 50-digit mpmath numbers.  What it takes as given is K14 (``match_priors``, tested
on its own), whose raw priors it resolves with its own fp32 ``resolve``.

Tolerance.  The curves are fp32 roundings of fp64 work, so a value is held to

    ulp32(E) / 2 + E64

of the oracle's E.  E64 is the fp64 part: the worst distance of the host mirror from the oracle
before the rounding to fp32 (its fp64 cavities and messages give the fp64 marginal), measured
over the oracle cases below at every S, times 8 for the order of operations.  Measured:
E64_MEASURED (``test_oracle`` prints the figure of a run and holds it to E64).  The
kernels compose the same chains as scan elements in another order and are held to twice the
bound against the mirror, the rule K16 uses."""
import functools
import types

import mpmath
import numpy as np
import torch

import hindsight_cases as H
from analyzer_amd.models.tiers import vst_table
from analyzer_amd.ops import ThroughTime
from analyzer_amd.ops.native import native
from analyzer_amd.ops.rate import BatchRater
from analyzer_amd.ops.scorecard import chain_of, match_priors
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream, play_out

TILE = 4096            # csrc/kernels.h kTttTile; checked below
E64_MEASURED = 4.1e-12  # mu points: the worst |mirror fp64 - oracle| over the oracle cases (4.02e-12; test_oracle)
E64 = 8 * E64_MEASURED
DIGITS = 50
SNAPSHOTS = (0, 1, 3, 8)
CFG = H.CFG
TAU = H.TAU


def check_constants():
    assert int(native().TTT_TILE) == TILE == H.TILE


def bound(e):
    """ulp32(E) / 2 + E64 of oracle (or reference) values ``e``."""
    return 0.5 * H.ulp32(e) + E64


# ------------------------------------------------------------------ histories
def start_of(roster):
    """What ``ThroughTime`` takes, copied from a roster before it is rated."""
    return types.SimpleNamespace(state=roster.state.clone(), attrs=roster.attrs.clone())


def on(start, device):
    return types.SimpleNamespace(state=start.state.to(device), attrs=start.attrs.to(device))


def rate(rec, P, device, seed, K=None):
    """(start, rec, rows) on the CPU: ``rec`` rated by ``BatchRater`` on ``device`` from a fresh
    roster of P players with NULL tracks."""
    K = K or (rec.shape[1] - 2) // 2
    roster = make_roster(RosterSpec(num_players=P, seed=seed, p_rated=0.5, p_mode_rated=0.5), device=device)
    start = start_of(roster)
    res = BatchRater(CFG).rate(roster, rec.to(device), K)
    return on(start, "cpu"), rec.cpu(), res.packed.cpu().clone()


def records(K, ids, seed, mode=None):
    """Full-roster records of the players ``ids`` [M, 2K] with random modes and winners (one
    match in twelve a tie)."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, dtype=np.int64)
    M, S = ids.shape
    rec = np.zeros((M, S + 2), dtype=np.int64)
    rec[:, :S] = ids
    mode = rng.integers(0, 6, M) if mode is None else np.broadcast_to(mode, (M,))
    rec[:, S] = mode | (K << 8) | (K << 16) | (2 << 24)
    rec[:, S + 1] = np.where(rng.random(M) < 1 / 12, 0, rng.integers(1, 3, M))
    return torch.from_numpy(rec.astype(np.int32))


ORACLE_P = 30


@functools.lru_cache(maxsize=None)
def mixed(K, device, M=240):
    """(start, rec, rows, P): the ``RATED_SPEC`` mix (ties, AFK, uneven, invalid and unsupported
    rows) over 30 players, with twins and ids outside [0, P) put in."""
    P = ORACLE_P
    rec = make_stream(StreamSpec(team_size=K, seed=250 + K, modes=H.ALL_MODES, **H.RATED_SPEC), M, P, K=K,
                      device="cpu").clone()
    rng = np.random.default_rng(260 + K)
    r = rec.numpy()
    for m in np.flatnonzero(rng.random(M) < 0.06):
        r[m, K] = r[m, 0]  # a twin across the rosters
        if K > 1:
            r[m, 1] = r[m, 0]  # and within one
    for m in np.flatnonzero(rng.random(M) < 0.04):
        r[m, int(rng.integers(0, 2 * K))] = int(rng.choice([-1, P, P + 5, 2 ** 31 - 1]))
    start, rec, rows = rate(rec, P, device, seed=240 + K, K=K)
    st = rows.view(torch.int32).numpy().view(np.uint32)[:, 10 * K + 1] & 0xFF
    assert {0, 1, 2, 3} <= set(st.tolist()) and (st == 8).any()
    return start, rec, rows, P


@functools.lru_cache(maxsize=None)
def league(device, M=300, P=6, seed=31):
    """(start, rec, rows, P): six players, every match a 3v3 of all of them in one mode, the
    outcomes played out from latent skills with a seed."""
    rng = np.random.default_rng(seed)
    ids = np.argsort(rng.random((M, P)), axis=1)
    rec = records(3, ids, seed + 1, mode=1)
    skill = torch.tensor(rng.normal(1500.0, 500.0, P))
    rec = play_out(rec, skill, float(CFG.beta), seed + 2)
    return (*rate(rec, P, device, seed=seed + 3), P)


@functools.lru_cache(maxsize=None)
def singles(M=700):
    """(start, rec, rows, P): 1v1 matches over 2 M distinct players, every chain one element.
    Every player is rated on every track and the history is rated on the host's fp64 path, so the
    rows are the correctly rounded filter: nothing is seeded (the fp64 host rater seeds in fp64,
    K20 resolves in fp32 as the device does, and a seeded prior differs between the two in its
    last fp32 digit) and no fp32 arithmetic of the device rater stands between the rows and the
    closed form.  The kernels are given these rows too."""
    P, ids = 2 * M, np.arange(2 * M).reshape(M, 2)
    roster = make_roster(RosterSpec(num_players=P, seed=42, p_rated=1.0, p_mode_rated=1.0), device="cpu")
    start = start_of(roster)
    rows = BatchRater(CFG, host_fp64=True).rate(roster, records(1, ids, 41), 1).packed.clone()
    return start, records(1, ids, 41), rows, P


@functools.lru_cache(maxsize=None)
def singles_mixed(device, M=700):
    """The same matches from a roster with NULL tracks, rated on ``device``: seeded priors, and on
    a GPU the rater's fp32 arithmetic."""
    ids = np.arange(2 * M).reshape(M, 2)
    return (*rate(records(1, ids, 41), 2 * M, device, seed=42), 2 * M)


@functools.lru_cache(maxsize=None)
def shape(name, device):
    """The scan shapes: (start, rec, rows, P)."""
    rng = np.random.default_rng(50)
    if name == "tiles":  # chains of ~450 elements that span tiles
        P, ids = 40, np.argsort(rng.random((3000, 40)), axis=1)[:, :6]
    elif name == "every":  # one chain of 5,000 elements through the stitch
        P, ids = 6, np.stack([np.zeros(5000, dtype=np.int64), 1 + np.arange(5000) % 5], axis=1)
    elif name == "inner":  # runs inside the tiles only
        P, ids = 5000, rng.integers(0, 5000, (3000, 6))
    elif name == "edges":
        P, ids = H.tile_edges()[2], H.tile_edges()[0][:, :2].numpy()
    else:
        raise KeyError(name)
    K = ids.shape[1] // 2
    return (*rate(records(K, ids, 51), P, device, seed=52), P)


# ------------------------------------------------------------------ running the code under test
def fit(device, start, rec, rows, sweeps, track="shared", tau=TAU, **kw):
    """(smoothed [M, S, 2] fp32 numpy, Fit, ThroughTime) of a history on ``device``."""
    tt = ThroughTime(on(start, device), track=track, cfg=H.cfg_tau(tau))
    res = tt.fit(rec.to(device), rows.to(device), sweeps=sweeps, **kw)
    assert res.smoothed.device.type == torch.device(device).type and res.smoothed.dtype == torch.float32
    assert tuple(res.smoothed.shape) == (rec.shape[0], rec.shape[1] - 2, 2)
    assert len(res.residual) == res.sweeps <= sweeps
    return res.smoothed.cpu().numpy(), res, tt


def marginal64(tt):
    """The fp64 marginal (mu, sigma) [n, 2] of the last fit from its cavities and messages."""
    _, _, cav, msg = tt._last
    cav, msg = cav.cpu().numpy(), msg.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        pc = 1.0 / cav[:, 1]
        pm = pc + msg[:, 1]
        return np.stack([(cav[:, 0] * pc + msg[:, 0]) / pm, np.sqrt(1.0 / pm)], axis=1)


# ------------------------------------------------------------------ the oracle
def live_slots(rec, P):
    r = rec.numpy().astype(np.int64)
    S = r.shape[1] - 2
    K = S // 2
    ids, mode, n0, n1 = r[:, :S], r[:, S] & 0xFF, (r[:, S] >> 8) & 0xFF, (r[:, S] >> 16) & 0xFF
    pos = np.concatenate([np.arange(K), np.arange(K)])
    size = np.concatenate([np.repeat(n0[:, None], K, 1), np.repeat(n1[:, None], K, 1)], axis=1)
    return (pos[None, :] < size) & (ids >= 0) & (ids < P) & (mode < 6)[:, None]


def resolve(pr, attr, vst, us):
    """The resolved (shared mu, sigma, mode mu, sigma) of raw stored values in fp32 -- seeding a
    NULL shared track, the mode track falling back to the shared one -- or None."""
    f = np.float32
    sh_mu, sh_sig, md_mu, md_sig = (f(x) for x in pr)
    if np.isnan(sh_mu):
        rr, rb, tier = (f(x) for x in attr[:3])
        rp = f("nan")
        if rr == rr and rr != 0:
            rp = rr
        if rb == rb and rb != 0 and (rp != rp or rb > rp):
            rp = rb
        if rp == rp:
            sh_sig = f(us) * f(2.0 / 3.0)
            sh_mu = rp + sh_sig
        else:
            if tier != tier or float(int(tier)) != float(tier) or not -1 <= int(tier) <= 29:
                return None
            sh_sig = f(us)
            sh_mu = f(vst[int(tier) + 1]) + sh_sig
    elif sh_sig != sh_sig or sh_sig == 0:
        return None
    if np.isnan(md_mu):
        md_mu, md_sig = sh_mu, sh_sig
    elif md_sig != md_sig or md_sig == 0:
        return None
    return sh_mu, sh_sig, md_mu, md_sig


class Exact:
    """Per snapshot S the exact marginals of the elements ``at`` (flat slot indices) as hi + lo
    pairs; the counters; the residuals of the sweeps."""

    def __init__(self, at, snaps, counters, residual):
        self.at, self.snaps, self.counters, self.residual = at, snaps, counters, residual


def oracle(start, rec, rows, P, track="shared", tau=TAU, sweeps=max(SNAPSHOTS), snapshots=SNAPSHOTS, damping=1.0):
    mp = mpmath.mpf
    S = rec.shape[1] - 2
    K = S // 2
    r = rec.numpy().astype(np.int64)
    ids = r[:, :S]
    live = live_slots(rec, P)
    clean = rows.clone()
    clean[:, :5 * S] = 1.0
    cand = H.elements(rec, clean, P, track)[0]
    elem, _, mu32, sg32, _ = H.elements(rec, rows, P, track)
    raw = match_priors(chain_of(start.state).clone(), rec, rows).numpy()
    vst = np.asarray(vst_table(), dtype=np.float32)
    attrs = start.attrs.numpy()
    us = float(CFG.unknown_player_sigma)
    bad = flat = inconsistent = 0
    with mpmath.workdps(DIGITS):
        q, beta2 = mp(float(tau)) ** 2, mp(float(CFG.beta)) ** 2
        L, pre, chains, active = {}, {}, {}, []
        for m in range(r.shape[0]):
            if not cand[m].any():
                continue
            res = {j: resolve(raw[m, :, j], attrs[ids[m, j]], vst, us) for j in range(S) if live[m, j]}
            if any(v is None for v in res.values()):
                inconsistent += 1
                continue
            ok = True
            for j in np.flatnonzero(cand[m]):
                if not elem[m, j]:
                    bad += 1
                    ok = False
                    continue
                i = m * S + int(j)
                m_pre, s_pre = res[j][0:2] if track == "shared" else res[j][2:4]
                m_pre, v_pre = mp(float(m_pre)), mp(float(s_pre)) ** 2 + q
                p = mp(float(sg32[m, j])) ** 2
                try:
                    pi, h = 1 / p - 1 / v_pre, mp(float(mu32[m, j])) / p - m_pre / v_pre
                except ZeroDivisionError:
                    pi = mp(-1)
                if not (mpmath.isfinite(pi) and pi >= 0):
                    pi = h = mp(0)
                    flat += 1
                L[i], pre[i] = (h, pi), (m_pre, v_pre)
                chains.setdefault(int(ids[m, j]), []).append(i)
            if ok:
                active.append(m)
        at = np.array(sorted(L), dtype=np.int64)
        snaps, residual, before = {}, [], None
        for k in range(sweeps + 1):
            cav, marg = {}, {}
            for chain in chains.values():
                fwd = {}
                fm, fv = pre[chain[0]]
                for i in chain:
                    fwd[i] = (fm, fv)
                    pi, h = 1 / fv + L[i][1], fm / fv + L[i][0]
                    fm, fv = h / pi, 1 / pi + q
                hb = pib = mp(0)
                for i in reversed(chain):
                    fm, fv = fwd[i]
                    pc, hc = 1 / fv + pib, fm / fv + hb
                    cav[i] = (hc / pc, 1 / pc)
                    pm = pc + L[i][1]
                    marg[i] = ((hc + L[i][0]) / pm, 1 / pm)
                    hs, ps = hb + L[i][0], pib + L[i][1]
                    hb, pib = hs / (1 + q * ps), ps / (1 + q * ps)
            if before is not None:
                residual.append(float(max([abs(marg[i][0] - before[i][0]) for i in marg], default=mp(0))))
            before = marg
            if k in snapshots:
                snaps[k] = (np.array([H._split(marg[i][0]) for i in at]).reshape(-1, 2),
                            np.array([H._split(mpmath.sqrt(marg[i][1])) for i in at]).reshape(-1, 2))
            if k == sweeps:
                break
            fresh = {}
            for m in active:
                own = {}
                for j in range(S):
                    if live[m, j]:
                        e = max(x for x in range(S) if live[m, x] and ids[m, x] == ids[m, j])
                        own[j] = cav[m * S + e]
                d = sum((c[0] if j < K else -c[0]) for j, c in own.items())
                c2 = len(own) * beta2 + sum(c[1] for c in own.values())
                w0, w1 = bool(r[m, S + 1] & 1), bool(r[m, S + 1] & 2)
                if w0 == w1:
                    a0, wf = -d / c2, mp(1)
                else:
                    c, sgn = mpmath.sqrt(c2), (1 if w0 else -1)
                    t = sgn * d / c
                    v = mpmath.npdf(t) / mpmath.ncdf(t)
                    a0, wf = sgn * v / c, v * (v + t)
                g = wf / c2
                for j in np.flatnonzero(elem[m]):
                    mu_c, s2 = own[int(j)]
                    den = 1 - s2 * g
                    fresh[m * S + int(j)] = (((a0 if j < K else -a0) + mu_c * g) / den, g / den)
            for i, (h, pi) in fresh.items():
                L[i] = ((1 - damping) * L[i][0] + damping * h, (1 - damping) * L[i][1] + damping * pi)
    return Exact(at, snaps, (bad, flat, inconsistent), residual)


def distance(got, ex, s):
    """(|mu - E|, |sigma - E|) of values ``got`` [n, 2] at the oracle's elements, snapshot s."""
    e_mu, e_sigma = ex.snaps[s]
    v = np.asarray(got, dtype=np.float64).reshape(-1, 2)[ex.at]
    return np.abs((v[:, 0] - e_mu[:, 0]) - e_mu[:, 1]), np.abs((v[:, 1] - e_sigma[:, 0]) - e_sigma[:, 1])


def check_layout(out, at, what):
    """Values at the elements ``at`` (flat indices) and NaN everywhere else."""
    g = np.asarray(out).reshape(-1, 2)
    has = np.zeros(len(g), dtype=bool)
    has[at] = True
    nan = np.isnan(g)
    assert (nan[:, 0] == nan[:, 1]).all() and nan[~has].all() and not nan[has].any(), what


def check_against_oracle(out, ex, s, what):
    check_layout(out, ex.at, what)
    err_mu, err_sigma = distance(out, ex, s)
    b_mu, b_sigma = bound(ex.snaps[s][0][:, 0]), bound(ex.snaps[s][1][:, 0])
    worst = (float((err_mu / b_mu).max(initial=0.0)), float((err_sigma / b_sigma).max(initial=0.0)))
    print("%s: %d elements, worst error / bound: mu %.3f sigma %.3f" % (what, len(ex.at), *worst))
    assert (err_mu <= b_mu).all() and (err_sigma <= b_sigma).all(), (what, worst)


def check_against_mirror(out, mirror, what, factor=2.0):
    """The kernels' curves against the host mirror's at ``factor`` times the bound."""
    g, h = np.asarray(out, dtype=np.float64).reshape(-1, 2), np.asarray(mirror, dtype=np.float64).reshape(-1, 2)
    assert (np.isnan(g) == np.isnan(h)).all(), what
    has = ~np.isnan(h[:, 0])
    err = np.abs(g[has] - h[has])
    b = factor * bound(np.maximum(np.abs(g[has]), np.abs(h[has])))
    worst = float((err / b).max(initial=0.0))
    print("%s: %d elements, worst |device - mirror| / (%g x bound): %.3f" % (what, int(has.sum()), factor, worst))
    assert (err <= b).all(), (what, worst)


# ------------------------------------------------------------------ the checks
def hindsight_of(device, rec, rows, P, track, tau=TAU):
    return H.run(device, rec, rows, P, track=track, tau=tau)[0]


def check_equals_hindsight(device, K=3):
    """S = 0 is K16: the forward messages reproduce the filter.  Within the sum of the budgets."""
    start, rec, rows, P = mixed(K, device)
    for track in ("shared", "ranked"):
        out, res, _ = fit(device, start, rec, rows, 0, track=track)
        assert res.sweeps == 0 and res.residual == []
        hs = hindsight_of(device, rec, rows, P, track)
        elem, ids, mu, _, _ = H.elements(rec, rows, P, track)
        assert (np.isnan(out[..., 0]) == ~elem).all() and (np.isnan(hs[..., 0]) == ~elem).all() and elem.any()
        n = np.bincount(ids[elem], minlength=P).astype(np.float64)
        top = np.zeros(P)
        np.maximum.at(top, ids[elem], np.abs(mu[elem].astype(np.float64)))
        b_mu, b_sigma = H.budget(n[ids[elem]], top[ids[elem]], hs[elem][:, 0], hs[elem][:, 1])
        err = np.abs(out[elem].astype(np.float64) - hs[elem].astype(np.float64))
        allow_mu, allow_sigma = b_mu + bound(hs[elem][:, 0]), b_sigma + bound(hs[elem][:, 1])
        print("S = 0 against hindsight, %s on %s: worst / allowed: mu %.3f sigma %.3f"
              % (track, device, (err[:, 0] / allow_mu).max(), (err[:, 1] / allow_sigma).max()))
        assert (err[:, 0] <= allow_mu).all() and (err[:, 1] <= allow_sigma).all(), track


def check_singles(device):
    """One element per player: the cavity is the prior, so no message ever moves and the curves
    are the rows' filtered values for any S, to ulp32 / 2 + E64; every residual is within that
    too (the first is the fp32 rounding of the rows themselves)."""
    start, rec, rows, P = singles()
    out, res, tt = fit(device, start, rec, rows, 5)
    elem, _, mu, sigma, _ = H.elements(rec, rows, P)
    assert elem.all() and res.sweeps == 5 and (tt.bad, tt.flat, tt.inconsistent) == (0, 0, 0)
    err_mu = np.abs(out[..., 0].astype(np.float64) - mu.astype(np.float64))
    err_sigma = np.abs(out[..., 1].astype(np.float64) - sigma.astype(np.float64))
    print("one element per player on %s: worst / bound: mu %.3f sigma %.3f, residuals %s"
          % (device, (err_mu / bound(mu)).max(), (err_sigma / bound(sigma)).max(), res.residual))
    assert (err_mu <= bound(mu)).all() and (err_sigma <= bound(sigma)).all()
    assert max(res.residual) <= float(bound(np.abs(mu).max()))


def check_singles_exact(device):
    """The same matches from a roster with NULL tracks, rated on ``device``, against the oracle:
    the curves after 0 sweeps are the rows, after 5 the exact posteriors, the residuals after the
    first are nothing.  How far these rows are from the exact posteriors -- fp64 against fp32
    seeds on the host path (measured 2.75 bounds for mu, 1.64 for sigma), the rater's fp32 arithmetic on a GPU
    -- is printed, not asserted: it is not K20's."""
    start, rec, rows, P = singles_mixed(device)
    ex = oracle(start, rec, rows, P, sweeps=5, snapshots=(0, 5))
    assert ex.counters == (0, 0, 0) and len(ex.at) == 2 * rec.shape[0]
    for s in (0, 5):
        out, res, _ = fit(device, start, rec, rows, s)
        check_against_oracle(out, ex, s, "one element per player after %d sweeps on %s" % (s, device))
    _, _, mu, sigma, _ = H.elements(rec, rows, P)
    off = distance(np.stack([mu, sigma], axis=-1), ex, 5)
    print("the rows against the exact posteriors, worst / bound: mu %.3f sigma %.3f"
          % ((off[0] / bound(ex.snaps[5][0][:, 0])).max(), (off[1] / bound(ex.snaps[5][1][:, 0])).max()))
    assert np.allclose(res.residual, ex.residual, rtol=0, atol=2 * E64) and max(res.residual[1:]) <= E64


def fp64_slack(rec, rows, P):
    """What two fp64 paths may differ by before any rounding to fp32, on chains longer than the
    oracle cases E64 was measured on: E64 and K16's per-element fp64 budget c n u max|mu| (the
    same kind of composition along a chain of n elements), for each path."""
    elem, ids, mu, _, _ = H.elements(rec, rows, P)
    n = np.bincount(ids[elem], minlength=P).max(initial=0)
    top = float(np.abs(mu[elem].astype(np.float64)).max(initial=0.0))
    return 2 * (E64 + H.C * n * H.U * top)


def check_shape(device, name, mirror_device="cpu", sweeps=2, tau=TAU):
    """The kernels against the host mirror on one scan shape: the curves at twice the bound; the
    fp64 residuals and finals within ``fp64_slack``."""
    start, rec, rows, P = shape(name, device)
    out, res, tt = fit(device, start, rec, rows, sweeps, tau=tau)
    ref, mres, mt = fit(mirror_device, start, rec, rows, sweeps, tau=tau)
    assert (tt.bad, tt.flat, tt.inconsistent) == (mt.bad, mt.flat, mt.inconsistent)
    check_against_mirror(out, ref, "%s, tau %g, on %s" % (name, tau, device))
    slack = fp64_slack(rec, rows, P)
    print("%s: residuals %s against the mirror's %s, slack %.2e" % (name, res.residual, mres.residual, slack))
    assert np.allclose(res.residual, mres.residual, rtol=0, atol=2 * slack), (res.residual, mres.residual)
    fin, mfin = tt.final().cpu().numpy(), mt.final().cpu().numpy()
    assert (np.isnan(fin) == np.isnan(mfin)).all() and not np.isnan(fin).all()
    assert np.allclose(fin[~np.isnan(fin)], mfin[~np.isnan(mfin)], rtol=0, atol=slack)
    return out


def check_small(device):
    """n = 0 and n = 1 histories, and no players."""
    start, rec, rows, P = mixed(2, device)
    out, res, tt = fit(device, start, rec[:0], rows[:0], 3)
    assert out.shape == (0, 4, 2) and res.sweeps == 3 and res.residual == [0.0] * 3
    assert bool(torch.isnan(tt.final()).all())
    st = rows.view(torch.int32).numpy().view(np.uint32)[:, 21] & 0xFF
    m = int(np.flatnonzero(st == 0)[0])
    elem, _, mu, sigma, _ = H.elements(rec[m:m + 1], rows[m:m + 1], P)
    out, res, tt = fit(device, start, rec[m:m + 1], rows[m:m + 1], 3)
    assert elem.any() and (np.isnan(out[..., 0]) == ~elem).all() and len(res.residual) == 3
    out, res, tt = fit(device, start, rec[m:m + 1], rows[m:m + 1], 0)  # chains of one element: the filtered values
    assert (np.isnan(out[..., 0]) == ~elem).all()
    if tt.flat == 0:
        assert (np.abs(out[elem][:, 0].astype(np.float64) - mu[elem]) <= bound(mu[elem])).all()
        assert (np.abs(out[elem][:, 1].astype(np.float64) - sigma[elem]) <= bound(sigma[elem])).all()
    none = types.SimpleNamespace(state=start.state[:0], attrs=start.attrs[:0])
    out, res, _ = fit(device, none, rec, rows, 2)
    assert np.isnan(out).all() and res.residual == [0.0, 0.0]


LEAGUE_SWEEPS = 40  # the issue's prototype reached 9e-11 in 30; this league takes 35 to pass 1e-6 (0.6 per sweep)


def check_convergence(device):
    """The six-player league: the undamped residual falls below 1e-6 within LEAGUE_SWEEPS,
    ``tol`` stops there, damping 0.5 reaches the same fp64 marginals within 1e-4 after 60 sweeps,
    and the curves are not K16's."""
    start, rec, rows, P = league(device)
    out, res, tt = fit(device, start, rec, rows, LEAGUE_SWEEPS)
    print("league on %s: residuals %s" % (device, ["%.2e" % x for x in res.residual]))
    assert res.sweeps == LEAGUE_SWEEPS and min(res.residual) < 1e-6
    assert all(b < a for a, b in zip(res.residual, res.residual[1:]))  # monotone, as on the prototype
    first = next(k for k, x in enumerate(res.residual) if x < 1e-6)
    full = marginal64(tt)
    stopped, sres, _ = fit(device, start, rec, rows, LEAGUE_SWEEPS, tol=1e-6)
    assert sres.sweeps == first + 1 < LEAGUE_SWEEPS and sres.residual[-1] < 1e-6
    assert all(x >= 1e-6 for x in sres.residual[:-1])
    damped, dres, dt = fit(device, start, rec, rows, 60, damping=0.5)
    elem = ~np.isnan(out[..., 0])
    gap = np.abs(marginal64(dt)[elem.ravel()] - full[elem.ravel()]).max()
    print("league on %s: damped against undamped %.2e, damped residual %.2e" % (device, gap, dres.residual[-1]))
    assert gap < 1e-4
    hs = hindsight_of(device, rec, rows, P, "shared")
    away = np.abs(out[elem][:, 0].astype(np.float64) - hs[elem][:, 0].astype(np.float64)).max()
    print("league on %s: max |mu_tt - mu_hindsight| = %.1f" % (device, away))
    assert away > 10
    fin = tt.final().cpu().numpy()
    ids = rec.numpy()[:, :6]
    for p in range(P):
        m = int(np.flatnonzero((ids == p).any(axis=1))[-1])
        j = int(np.flatnonzero(ids[m] == p)[-1])
        assert np.abs(fin[p] - out[m, j]).max() <= float(H.ulp32(out[m, j]).max())
    return out


def check_counters(device):
    """bad, flat and inconsistent on hand-made rows, and an object started from the wrong roster."""
    start, rec, rows, P = mixed(2, device)
    _, _, tt = fit(device, start, rec, rows, 1)
    assert (tt.bad, tt.inconsistent) == (0, 0)
    elem = H.elements(rec, rows, P)[0]
    # a filtered sigma above the walked prior's: a negative message, flat
    poisoned = rows.clone()
    hit = np.argwhere(elem)[:40:4]
    for n, (m, j) in enumerate(hit):  # each above the one before: the next prior of the same player
        poisoned[m, 4 + j] = 5000.0 * (n + 1)
    out, _, tt2 = fit(device, start, rec, poisoned, 2)
    assert tt2.flat >= tt.flat + len(hit) and tt2.bad == 0 and not np.isnan(out[elem]).any()
    # values that are no numbers: bad, no element, the match frozen
    poisoned = rows.clone()
    for n, (m, j) in enumerate(hit):
        poisoned[m, (0, 4)[n % 2] + j] = (float("nan"), float("inf"), -3.0)[n % 3]
    want_bad = H.elements(rec, poisoned, P)[4]
    out, _, tt3 = fit(device, start, rec, poisoned, 2)
    assert tt3.bad == want_bad > 0
    # a poisoned row is the next prior of its player (K14): where that does not resolve, the
    # whole match has no elements and is inconsistent
    left, nan = H.elements(rec, poisoned, P)[0], np.isnan(out[..., 0])
    lost = (nan & left).any(axis=1)
    assert nan[~left].all() and nan[lost].all() and int(lost.sum()) == tt3.inconsistent > 0
    # the wrong roster: every track NULL and no attribute to seed from
    wrong = types.SimpleNamespace(state=torch.full_like(start.state, float("nan")),
                                  attrs=torch.full_like(start.attrs, float("nan")))
    out, _, tt4 = fit(device, wrong, rec, rows, 1)
    assert tt4.inconsistent > 0 and np.isnan(out[..., 0]).sum() > (~elem).sum()
    st = rows.view(torch.int32).numpy().view(np.uint32)[:, 21] & 0xFF
    assert tt4.inconsistent <= int((st == 0).sum())


ARENA = dict(total_matches=2000, players=120, team_size=3, window=800, seed=2024)


def check_arena(device):
    """``RecordArena.through_time`` over the three windows of a 2,000-match re-rate: the rows of
    the listed players, with the curves ``ThroughTime.fit`` gives on the joined history."""
    from analyzer_amd.runtime.rerate import RerateSpec, rerate_resident, start_roster, stream_records

    spec = RerateSpec(**ARENA)
    roster0 = start_roster(spec, None, torch.device(device))
    _, _, arena = rerate_resident(spec, device, free_bytes=1 << 40)
    assert len(list(arena.windows())) == 3
    rec_of = stream_records(spec, device)
    rec, rows = rec_of(0, spec.total_matches), arena.filled_rows()
    players = [5, 7, 119]
    for track in ("shared", "ranked"):
        cols = {k: v.cpu().numpy() for k, v in arena.through_time(roster0, rec_of, players, sweeps=3,
                                                                  track=track).items()}
        res = ThroughTime(roster0, track=track).fit(rec, rows, sweeps=3)
        elem, ids, mu, sigma, _ = H.elements(rec.cpu(), rows.cpu(), spec.players, track)
        mine = np.flatnonzero(elem.ravel() & np.isin(ids.ravel(), players))
        assert len(mine) > 10 and (cols["match"] * 6 + cols["slot"] == mine).all()
        assert (cols["player"] == ids.ravel()[mine]).all()
        assert (H.bits(cols["mu"]) == H.bits(mu.ravel()[mine])).all()
        assert (H.bits(cols["sigma"]) == H.bits(sigma.ravel()[mine])).all()
        want = res.smoothed.cpu().numpy().reshape(-1, 2)[mine]
        assert (H.bits(cols["mu_tt"]) == H.bits(want[:, 0])).all()
        assert (H.bits(cols["sigma_tt"]) == H.bits(want[:, 1])).all()
        assert cols["residual"].tolist() == res.residual and len(res.residual) == 3
    return arena, roster0
