"""Through time (K20) on the CPU: the host mirror of ``ttt_fit`` -- the forward and backward
recursions as plain loops -- against the 50-digit oracle of through_time_cases.py,
``ThroughTime``, ``RecordArena.through_time`` and the ``--through-time`` command line."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from analyzer_amd.ops import ThroughTime
from analyzer_amd.ops.native import native

import hindsight_cases as H
import through_time_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants():
    T.check_constants()


@pytest.mark.parametrize("K", H.KS)
def test_oracle(K):
    """The mirror after S in {0, 1, 3, 8} sweeps within ulp32 / 2 + E64 of the oracle; its fp64
    marginals, before the rounding, within E64 itself (measured over these cases: 4.02e-12,
    that is E64 / 8); the counters and the residuals the oracle's."""
    start, rec, rows, P = T.mixed(K, "cpu")
    ex = T.oracle(start, rec, rows, P)
    assert len(ex.at) > 240 * K
    worst = 0.0
    for s in T.SNAPSHOTS:
        out, res, tt = T.fit("cpu", start, rec, rows, s)
        assert (tt.bad, tt.flat, tt.inconsistent) == ex.counters
        T.check_against_oracle(out, ex, s, "K=%d after %d sweeps" % (K, s))
        err = T.distance(T.marginal64(tt), ex, s)
        worst = max(worst, float(err[0].max()), float(err[1].max()))
        assert np.allclose(res.residual, ex.residual[:s], rtol=0, atol=2 * T.E64)
    print("K=%d: worst fp64 distance of the mirror from the oracle %.3e (E64_MEASURED %.1e)"
          % (K, worst, T.E64_MEASURED))
    assert worst <= T.E64


def test_oracle_mode_track_and_damping():
    start, rec, rows, P = T.mixed(3, "cpu")
    ex = T.oracle(start, rec, rows, P, track="ranked", sweeps=3, snapshots=(3,), damping=0.5)
    out, _, tt = T.fit("cpu", start, rec, rows, 3, track="ranked", damping=0.5)
    assert (tt.bad, tt.flat, tt.inconsistent) == ex.counters
    T.check_against_oracle(out, ex, 3, "ranked track, damping 0.5")
    modes, ranked = rec.numpy()[:, 6] & 0xFF, H.MODES.index("ranked")
    assert np.isnan(out[modes != ranked]).all() and not np.isnan(out[modes == ranked]).all()


def test_zero_sweeps_is_hindsight():
    T.check_equals_hindsight("cpu")


def test_one_element_per_player():
    T.check_singles("cpu")


def test_one_element_per_player_seeded_is_the_exact_posterior():
    T.check_singles_exact("cpu")


def test_convergence_and_not_hindsight():
    T.check_convergence("cpu")


def test_small_histories():
    T.check_small("cpu")


def test_tau_zero():
    start, rec, rows, P = T.mixed(2, "cpu")
    ex = T.oracle(start, rec, rows, P, tau=0.0, sweeps=2, snapshots=(2,))
    out, _, _ = T.fit("cpu", start, rec, rows, 2, tau=0.0)
    T.check_against_oracle(out, ex, 2, "tau = 0")


def test_counters_and_wrong_roster():
    T.check_counters("cpu")


def test_bad_arguments():
    start, rec, rows, P = T.mixed(2, "cpu")
    for track in ("mode", "chess", 3):
        with pytest.raises(ValueError):
            ThroughTime(start, track=track)
    with pytest.raises(ValueError):
        ThroughTime(start, cfg=H.cfg_tau(-1.0))
    with pytest.raises(ValueError):
        ThroughTime(types.SimpleNamespace(state=start.state.double(), attrs=start.attrs))
    tt = ThroughTime(start)
    for kw in ({"sweeps": -1}, {"sweeps": 2.5}, {"damping": 0.0}, {"damping": 1.5}, {"damping": float("nan")},
               {"tol": -1.0}, {"tol": float("nan")}):
        with pytest.raises(ValueError):
            tt.fit(rec, rows, **kw)
    with pytest.raises(ValueError):
        tt.fit(rec.long(), rows)
    with pytest.raises(ValueError):
        tt.fit(rec, rows.double())
    with pytest.raises(ValueError):
        tt.fit(rec, rows[:-1])
    with pytest.raises(ValueError):
        tt.fit(rec[:, :-1].contiguous(), rows)
    tt.max_slots = 4 * (rec.shape[0] - 1)
    with pytest.raises(ValueError, match="MAX_SLOTS"):
        tt.fit(rec, rows)
    assert bool(torch.isnan(ThroughTime(start).final()).all())
    priors = torch.zeros((rec.shape[0], 8), dtype=torch.float32)
    vst = tt.vst
    for args in ((rec, rows, priors[:, :4].contiguous(), None, vst, P, 1e6, 10.0, 500.0, 0, 0, 1, -1.0, 1.0),
                 (rec, rows, priors, None, vst, P, 1e6, -1.0, 500.0, 0, 0, 1, -1.0, 1.0),
                 (rec, rows, priors, None, vst, P, 1e6, 10.0, 500.0, 2, 0, 1, -1.0, 1.0),
                 (rec, rows, priors, None, vst, P, 1e6, 10.0, 500.0, 1, 6, 1, -1.0, 1.0),
                 (rec, rows, priors, None, vst, P, 1e6, 10.0, 500.0, 0, 0, -1, -1.0, 1.0),
                 (rec, rows, priors, None, vst, P, 1e6, 10.0, 500.0, 0, 0, 1, -1.0, 0.0),
                 (rec, rows, priors, None, vst[:5].contiguous(), P, 1e6, 10.0, 500.0, 0, 0, 1, -1.0, 1.0)):
        with pytest.raises(RuntimeError):
            native().ttt_fit(*args)


def test_arena_through_time(monkeypatch):
    import analyzer_amd.runtime.records as records

    arena, roster0 = T.check_arena("cpu")
    arena.size = 2
    with pytest.raises(ValueError):
        arena.through_time(roster0, lambda lo, hi: None, [5])
    arena.size = 1

    class Small(ThroughTime):  # a fit that takes 600 slots: the arena holds 12,000
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.max_slots = 600

    monkeypatch.setattr(records, "ThroughTime", Small)
    with pytest.raises(ValueError, match="MAX_SLOTS"):
        arena.through_time(roster0, lambda lo, hi: None, [5])


CLI = ["--matches", str(T.ARENA["total_matches"]), "--players", str(T.ARENA["players"]), "--window",
       str(T.ARENA["window"])]


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", "cpu", *CLI, *args],
                          capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)


def test_cli_through_time():
    from analyzer_amd.runtime.rerate import RerateSpec, rerate_resident, start_roster, stream_records

    ok = _cli("--records", "resident", "--arena-free-bytes", str(1 << 30), "--through-time", "5,7",
              "--through-time-track", "ranked", "--through-time-sweeps", "3", "--hindsight", "5")
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith('{"through_time"')]
    assert [ln["through_time"] for ln in lines] == [5, 7]
    assert sum(ln.startswith('{"hindsight"') for ln in ok.stdout.splitlines()) == 1
    spec = RerateSpec(**T.ARENA)
    roster0 = start_roster(spec, None, torch.device("cpu"))
    _, _, arena = rerate_resident(spec, "cpu", free_bytes=1 << 40)
    cols = arena.through_time(roster0, stream_records(spec, "cpu"), [5, 7], sweeps=3, track="ranked")
    for line in lines:
        sel = (cols["player"] == line["through_time"]).nonzero().reshape(-1)
        assert line["track"] == "ranked" and line["records"] == sel.numel() > 0 and line["sweeps"] == 3
        assert line["match"] == sorted(line["match"]) and line["residual"] == cols["residual"].tolist()[-1]
        for name in ("match", "mu", "sigma", "mu_tt", "sigma_tt"):
            assert line[name] == cols[name][sel].tolist(), name


def test_cli_through_time_argument_errors():
    for args in (("--through-time", "5"), ("--records", "resident", "--through-time", "5,120"),
                 ("--records", "resident", "--through-time", "5", "--through-time-track", "chess"),
                 ("--records", "resident", "--through-time", "5", "--through-time-sweeps", "-1"),
                 ("--records", "resident", "--through-time-sweeps", "3")):
        bad = _cli(*args)
        assert bad.returncode == 2 and "--through-time" in bad.stderr, (args, bad.stderr)
