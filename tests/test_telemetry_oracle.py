"""K8 telemetry aggregation against the exact per-event oracle of telemetry_cases.py, on
every path: the fp32 host mirror and the CPU fused path (no GPU needed), the standalone
kernel in its three implementations, and the fused executor paths (``-m gpu``).

Every path gets the same assertions (telemetry_cases.check): ``stats`` is pre-filled with
-1 and every row must be overwritten; counts and the malformed counter are exact; grid
values (and everything built on them) compare with ``==``; general / cancelling / wide
values stay within B = 1.02 (n + 2) 2^-24 sum|v| per cell; cells with Inf / NaN hold
exactly the oracle's verdict and their neighbours stay clean.  The budget and the
measured worst err / B per path are in docs/ARCHITECTURE.md ("Telemetry error budget").
"""
import numpy as np
import pytest
import torch

import telemetry_cases as TC
from analyzer_amd.ops import rate as R
from analyzer_amd.ops.native import native
from analyzer_amd.ops.telemetry import Telemetry, TelemetrySpec, aggregate, aggregate_reference, make_telemetry

KS = (1, 2, 3, 4, 5)
FUSED_KS = (1, 3, 5)  # the library instantiates fused launches for every K = 1..5
IMPL_NAMES = {"1": "mfma_span", "0": "lds_atomics", "2": "rows"}
# executor paths: (ANA_TELE_ROLE, ANA_TELE_FUSE_MAX above the window?)
FUSED_PATHS = {"inline": (-1, True), "mfma_after_rating": (-1, False), "idle_wave_tiles": (0, True),
               "dedicated_waves": (2, True)}


def sentinel(M, K, device="cpu"):
    return torch.full((M, 2 * K, TC.FEATURES), -1.0, dtype=torch.float32, device=device)


def run_host(c):
    stats = sentinel(c.M, c.K)
    bad = native().telemetry(c.evoff, c.events, c.K, stats, torch.zeros(1, dtype=torch.int32))
    return stats, int(bad)


def run_cpu_fused(c, rec=None):
    """BatchRater.rate on CPU tensors: the host rater, then the host mirror.  This path
    reports no malformed count (telemetry_errors reads the device control words)."""
    rec = TC.stream_for(c.K, c.M) if rec is None else rec
    stats = sentinel(c.M, c.K)
    R.BatchRater().rate(TC.fused_roster(), rec, c.K, telemetry=(c.evoff, c.events, stats))
    return stats, None


def run_standalone(c, device):
    stats = sentinel(c.M, c.K, device)
    bad = torch.zeros(1, dtype=torch.int32, device=device)
    aggregate(Telemetry(c.evoff.to(device), c.events.to(device)), c.K, stats, bad)
    torch.cuda.synchronize()
    return stats.cpu(), int(bad.item())


# ------------------------------------------------------------------------- CPU tests
def test_case_builders_place_what_they_claim():
    """Properties the cases must keep having (most are asserted inside the builders)."""
    for K in KS:
        assert TC.max_row_tiles_per_chunk(TC.case("density/one", K).evoff, K) >= TC.MIN_TILES_ONE[K]
        o = TC.oracle_of(TC.case("values/nonfinite", K))
        sums = o.verdict[..., list(TC.SUM_COLS)]
        assert all((sums == v).any() for v in (TC.POS_INF, TC.NEG_INF, TC.IS_NAN))
        assert o.malformed >= 4 * 14 and not o.verdict[..., list(TC.COUNT_COLS)].any()
        g = TC.oracle_of(TC.case("values/grid", K))
        assert float(g.sabs.max()) < TC.GRID_CELL_MAX and float(g.sabs.max()) >= 2.0 ** 15
        w = TC.oracle_of(TC.case("wrap", K))
        assert w.malformed == 3 and w.exact[65536:, :, 7].sum() > 100
        assert TC.oracle_of(TC.case("offset", K)).malformed == 0
        z = TC.oracle_of(TC.case("values/negzero", K))
        assert ((z.n[:, 0] > 0) & (z.sabs[:, 0] == 0)).sum() >= 40
    assert TC.case("density/bursty", 3).M == TC.M_SMALL and TC.case("wrap", 3).M == TC.WRAP_M


def test_aggregate_reference_agrees_with_the_oracle():
    """The fp64 numpy oracle of the older tests, on a generated stream with malformed
    and infinite events: equal to the per-event oracle (fp64 sums of <= 90 fp32 values
    between 1 and 1000 are exact)."""
    from analyzer_amd.ops.synth import StreamSpec, make_stream

    K, M = 3, 700
    rec = make_stream(StreamSpec(team_size=K, seed=43, p_uneven=0.2), M, 300, K=K)
    tel = make_telemetry(TelemetrySpec(seed=5, min_events=0, max_events=90), rec, K)
    ev = tel.events.clone()
    ev[::53, 0] = (ev[::53, 0] & ~0xFF) | (2 * K)  # slot out of range
    ev[7::61, 0] += 1 << 16                        # tag names the next match
    ev[11::67, 0] = (ev[11::67, 0] & ~0xFF00) | (3 << 8)
    ev[:, 1].view(torch.float32)[11::67] = float("inf")
    o = TC.oracle(tel.evoff, ev, K)
    assert o.malformed > 20 and (o.verdict == TC.POS_INF).any()
    assert np.array_equal(aggregate_reference(Telemetry(tel.evoff, ev), K), o.exact)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", TC.ALL_NAMES)
def test_host_mirror_vs_oracle(name, K):
    c = TC.case(name, K)
    stats, bad = run_host(c)
    TC.check(stats.numpy(), bad, TC.oracle_of(c), c.cls, "path=host " + c.label)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", TC.ALL_NAMES)
def test_cpu_fused_path_vs_oracle(name, K):
    c = TC.case(name, K)
    stats, bad = run_cpu_fused(c)
    TC.check(stats.numpy(), bad, TC.oracle_of(c), c.cls, "path=cpu_fused " + c.label)


@pytest.mark.parametrize("M,values", [(2000, "grid"), (2000, "general"), (TC.WRAP_M, "grid")])
@pytest.mark.parametrize("K", FUSED_KS)
def test_host_paths_on_the_fused_family(K, M, values):
    fc = TC.fused_case(K, M, values)
    for c in (fc.case, fc.clean):
        stats, bad = run_host(c)
        TC.check(stats.numpy(), bad, TC.oracle_of(c), c.cls, "path=host " + c.label)
    assert TC.oracle_of(fc.case).malformed >= 2 * (M // 97) and TC.oracle_of(fc.clean).malformed == 0
    stats, bad = run_cpu_fused(fc.case, fc.rec)
    TC.check(stats.numpy(), bad, TC.oracle_of(fc.case), fc.case.cls, "path=cpu_fused " + fc.case.label)


# ------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("impl", ["1", "0", "2"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", TC.ALL_NAMES)
def test_standalone_kernel_vs_oracle(gpu_device, monkeypatch, name, K, impl):
    """The standalone kernel: one-hot MFMA over 63-match spans (impl 1), LDS float
    atomics (impl 0), one lane per stat row (impl 2; also the host mirror's bits)."""
    monkeypatch.setenv("ANA_TELE_IMPL", impl)
    c = TC.case(name, K)
    stats, bad = run_standalone(c, gpu_device)
    TC.check(stats.numpy(), bad, TC.oracle_of(c), c.cls, "path=%s %s" % (IMPL_NAMES[impl], c.label))
    if impl == "2":  # row sums in event order, as the host mirror: the same bits
        assert torch.equal(TC.canon_bits(stats), TC.canon_bits(run_host(c)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("impl", ["1", "2"])
@pytest.mark.parametrize("K", KS)
def test_standalone_kernel_is_deterministic(gpu_device, monkeypatch, K, impl):
    """Impl 1 (the stream order fixes every MFMA) and impl 2 (event order per row) give
    the same bits on every run."""
    monkeypatch.setenv("ANA_TELE_IMPL", impl)
    for name in ("values/general", "values/cancel", "density/bursty"):
        c = TC.case(name, K)
        a, b = run_standalone(c, gpu_device)[0], run_standalone(c, gpu_device)[0]
        assert torch.equal(TC.canon_bits(a), TC.canon_bits(b)), name


@pytest.mark.gpu
@pytest.mark.parametrize("M,values", [(2000, "grid"), (2000, "general"), (TC.WRAP_M, "grid")])
@pytest.mark.parametrize("K", FUSED_KS)
@pytest.mark.parametrize("path", list(FUSED_PATHS))
def test_fused_paths_vs_oracle(gpu_device, monkeypatch, path, K, M, values):
    """Aggregation inside (or right after) the rating launch: inline fold in the lane
    groups, the MFMA span kernel after the rating (past ANA_TELE_FUSE_MAX), 16-match
    MFMA tiles on idle waves, 63-match spans on dedicated waves.  K = 1, 3, 5 (the
    library instantiates every K = 1..5 for fused launches).  Same assertions as the
    standalone kernel; ratings and roster are bit-identical to a launch without
    telemetry; the malformed counter is per launch."""
    role, above = FUSED_PATHS[path]
    monkeypatch.setenv("ANA_TELE_ROLE", str(role))
    monkeypatch.setenv("ANA_TELE_FUSE_MAX", str(1 << 30 if above else M // 2))
    fc = TC.fused_case(K, M, values)
    c = fc.case
    rec = fc.rec.to(gpu_device)
    a, b = TC.fused_roster(gpu_device), TC.fused_roster(gpu_device)
    br = R.BatchRater()
    assert br.fuses((c.evoff, None, None), M) == above
    stats = sentinel(M, K, gpu_device)
    ra = br.rate(a, rec, K, telemetry=(c.evoff.to(gpu_device), c.events.to(gpu_device), stats))
    bad = br.telemetry_errors(gpu_device)
    print("stale retries %s: %d" % (path, br.stale_retries(gpu_device)))
    rb = R.BatchRater().rate(b, rec, K)
    assert torch.equal(ra.status.cpu(), torch.from_numpy(fc.status))
    assert torch.equal(ra.status, rb.status)
    assert torch.equal(TC.canon_bits(a.state), TC.canon_bits(b.state))
    for f in ("quality", "s_mu", "s_sig", "delta", "m_mu", "m_sig"):
        assert torch.equal(TC.canon_bits(getattr(ra, f)), TC.canon_bits(getattr(rb, f))), f
    TC.check(stats.cpu().numpy(), bad, TC.oracle_of(c), c.cls, "path=%s %s" % (path, c.label))
    # a second launch of the same rater on clean events: the counter starts over
    cl = fc.clean
    stats.fill_(-1.0)
    br.rate(a, rec, K, telemetry=(cl.evoff.to(gpu_device), cl.events.to(gpu_device), stats))
    TC.check(stats.cpu().numpy(), br.telemetry_errors(gpu_device), TC.oracle_of(cl), cl.cls,
             "path=%s %s" % (path, cl.label))
