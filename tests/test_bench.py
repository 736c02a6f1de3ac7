"""bench.py argument contract (CPU): BASELINE config defaults, the merge precision
default and the rank-count check that runs before any GPU call."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ("COMM_DTYPE", "SWEEPS", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)


def test_config_defaults():
    a = bench.parse([])
    assert (a.config, a.team_size, a.matches_per_gpu, a.players) == (2, 3, 10_000_000, 1_000_000)
    a = bench.parse(["--config", "3"])
    assert (a.team_size, a.matches_per_gpu) == (5, 12_500_000)
    a = bench.parse(["--config", "5"])
    assert (a.players, a.matches_per_gpu, a.ring) == (10_000_000, 16_000_000, 2)
    a = bench.parse(["--config", "2", "--matches-per-gpu", "1250000"])
    assert a.matches_per_gpu == 1_250_000


def test_merge_precision_default(monkeypatch):
    # one sweep: bf16 messages (accuracy identical to fp32, profiles/r2/slice_size_accuracy.log;
    # fp32 range in RCCL's sums); config 5 keeps BASELINE's fp16 moments
    assert bench.parse([]).comm_dtype == "bf16"
    assert bench.parse(["--config", "5"]).comm_dtype == "fp16"
    # causal re-sweeps aim at the exact result: fp32 unless asked otherwise
    assert bench.parse(["--sweeps", "4"]).comm_dtype == "fp32"
    assert bench.parse(["--sweeps", "4", "--comm-dtype", "bf16"]).comm_dtype == "bf16"
    monkeypatch.setenv("COMM_DTYPE", "fp32")
    assert bench.parse([]).comm_dtype == "fp32"


def test_world_size_must_match_gpus(monkeypatch):
    # under torchrun, --gpus must equal WORLD_SIZE; checked before the GPU is touched
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--gpus 3 but WORLD_SIZE=2"):
        bench.main(["--gpus", "3"])


def test_merges_per_step():
    a = bench.parse(["--merges-per-step", "8"])
    assert a.merges_per_step == 8 and a.matches_per_gpu == 10_000_000  # same matches per step
    with pytest.raises(SystemExit):
        bench.parse(["--merges-per-step", "3"])   # must divide the step
    with pytest.raises(SystemExit):
        bench.parse(["--config", "4", "--merges-per-step", "2"])


def test_merges_per_step_default_is_accuracy_bounded(monkeypatch):
    """One GPU has nothing to merge (one window per step); N > 1 merges N times per
    step so that one sweep keeps Spearman(mu - sigma) >= 0.99 against the exact
    sequential result (profiles/r3/merges_vs_ranks.log); causal re-sweeps are
    exact already and keep one window."""
    assert bench.parse([]).merges_per_step == 1
    # one merge per rank's worth of concurrency: k = the largest power of two <= N (<= 8)
    assert bench.parse(["--gpus", "8"]).merges_per_step == 8
    assert bench.parse(["--gpus", "4"]).merges_per_step == 4
    assert bench.parse(["--gpus", "6"]).merges_per_step == 4
    assert bench.parse(["--gpus", "2", "--config", "3"]).merges_per_step == 2
    # 5v5 has 10 appearances a match: twice the merges from N = 4 (merges_vs_ranks_5v5.log)
    assert bench.parse(["--gpus", "4", "--config", "3"]).merges_per_step == 8
    assert bench.parse(["--gpus", "8", "--config", "3"]).merges_per_step == 16
    # config 5 (10M players): one merge per step meets the fidelity bars at N = 8
    assert bench.parse(["--gpus", "8", "--config", "5"]).merges_per_step == 1
    assert bench.parse(["--gpus", "8", "--sweeps", "8"]).merges_per_step == 1
    assert bench.parse(["--gpus", "8", "--config", "4"]).merges_per_step == 1
    assert bench.parse(["--gpus", "8", "--merges-per-step", "2"]).merges_per_step == 2
    monkeypatch.setenv("WORLD_SIZE", "4")
    assert bench.parse([]).merges_per_step == 4
    assert bench.parse([]).accuracy == 1


def test_shared_card_blocks():
    """Ranks sharing a card (gloo rehearsal) split the executor grid; one rank per GPU
    (RCCL, or world <= GPUs) keeps the default."""
    assert bench.shared_card_blocks(8, 8, "nccl") == 0
    assert bench.shared_card_blocks(8, 1, "nccl") == 0
    assert bench.shared_card_blocks(2, 2, "gloo") == 0
    assert bench.shared_card_blocks(2, 1, "gloo") == 256
    assert bench.shared_card_blocks(8, 1, "gloo") == 64
    assert bench.shared_card_blocks(6, 2, "gloo") == 170
    assert bench.shared_card_blocks(64, 1, "gloo") == 16


def _run_on_cpu(capsys, *extra):
    import json

    capsys.readouterr()
    assert bench.main(["--device", "cpu", "--gpus", "1", "--players", "3000", "--matches-per-gpu", "5000",
                       "--steps", "3", "--warmup", "1"] + list(extra)) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_lean_and_full_adds_the_checks(capsys):
    """A plain run times its steps and prints the line: no status check, no fp64
    verification, no accuracy pass.  --full (the N > 1 accuracy pass, see
    test_multi_rank_json_contract_on_cpu) changes nothing else on one rank; --verify
    stays an option of its own."""
    a = bench.parse([])
    assert not (a.full or a.check or a.verify or a.dump_outputs)
    j = _run_on_cpu(capsys)
    assert j["full"] is False and j["verify"] is None and j["accuracy"] is None
    assert (j["steps"], j["warmup"]) == (3, 1) and j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(5000 / (j["ms_per_step"] / 1000.0))
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in j
    j = _run_on_cpu(capsys, "--full", "--verify")
    assert j["full"] is True and j["accuracy"] is None
    assert j["verify"]["status_mismatch"] == 0 and j["verify"]["matches"] == 5000
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_writes_the_last_steps_results(tmp_path, capsys):
    """--dump-outputs: finite float arrays of the last timed step's records and roster
    (NULL = NaN entries as 0, marked in <name>_null), the same from run to run, and what
    rating the same windows by hand gives."""
    import numpy as np
    import torch

    from analyzer_amd.ops.rate import BatchRater, RateResult
    from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream

    a, b = tmp_path / "a", tmp_path / "b"
    _run_on_cpu(capsys, "--dump-outputs", str(a))
    _run_on_cpu(capsys, "--dump-outputs", str(b))
    names = sorted(p.name for p in a.iterdir())
    values = tuple(f for f in RateResult.FIELDS if f != "status") + ("roster_mu", "roster_sigma")
    assert names == sorted(n + ".npy" for n in values + tuple(v + "_null" for v in values)
                           + ("status", "record_rows", "roster_rows"))
    got = {n[:-4]: np.load(str(a / n)) for n in names}
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_MAX_BYTES
    for n in names:
        assert got[n[:-4]].dtype in (np.float32, np.float64) and np.isfinite(got[n[:-4]]).all(), n
        assert np.array_equal(got[n[:-4]], np.load(str(b / n)), equal_nan=True), n
    assert got["s_mu"].shape == (5000, 6) and got["roster_mu"].shape == (3000, 8)
    assert np.array_equal(got["record_rows"], np.arange(5000))
    # 1 warm-up + 3 timed steps over a ring of 4 windows: the last step rates window 3
    roster = make_roster(RosterSpec(num_players=3000, seed=2024))
    spec = StreamSpec(team_size=3, seed=2025)
    rater = BatchRater()
    for w in range(4):
        res = rater.rate(roster, make_stream(spec, 5000, 3000, K=3, base=w * 5000), 3)
    assert np.array_equal(got["status"], res.status.float().numpy())
    for name, want in (("s_mu", res.s_mu), ("m_sig", res.m_sig), ("quality", res.quality),
                       ("roster_mu", roster.state[:, 0::4]), ("roster_sigma", roster.state[:, 2::4])):
        want = want.numpy()
        assert np.array_equal(got[name + "_null"], np.isnan(want).astype(np.float32)), name
        assert np.array_equal(got[name], np.nan_to_num(want, nan=0.0)), name
    assert got["s_mu_null"].any() and got["roster_mu_null"].any() and not got["s_mu_null"].all()
    # a larger output is sampled: sorted distinct rows, the same for the same seed
    rows = bench._sample_rows(10 * bench.DUMP_ROWS, 7)
    assert rows.numel() == bench.DUMP_ROWS and bool((rows[1:] > rows[:-1]).all()) and int(rows[-1]) < 10 * bench.DUMP_ROWS
    assert torch.equal(rows, bench._sample_rows(10 * bench.DUMP_ROWS, 7))


def _spawn_on_cpu(tmp_path, n, *extra):
    import json
    import subprocess

    env = dict(os.environ, ANA_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(var, None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--device", "cpu", "--gpus", str(n),
                          "--players", "2000", "--matches-per-gpu", str(1000 * n), "--steps", "2", "--warmup", "1"]
                         + list(extra), cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 only
    return json.loads(lines[0])


def test_plain_multi_rank_run_skips_the_accuracy_pass(tmp_path):
    """Without --full an N > 1 run times its steps and prints the line: no accuracy block."""
    j = _spawn_on_cpu(tmp_path, 2)
    assert j["n_gpus"] == 2 and j["full"] is False and j["accuracy"] is None and j["merge_ms"]["buckets"] >= 1


@pytest.mark.parametrize("n", [2, 4, 8])
def test_multi_rank_json_contract_on_cpu(tmp_path, n):
    """The N > 1 path of the driver contract end to end on the CPU (``--device cpu``:
    host mirror, gloo): bench.py spawns its own N ranks (127.0.0.1 rendezvous), runs
    one-prepass-per-step DP steps with a merge after each of k = N windows, and rank 0
    prints ONE JSON line with the N > 1 keys -- the rank count, the merge split with the
    prepass placement and, under --full, the accuracy block with the per-participant
    record errors and the merge decodes' clamp count."""
    j = _spawn_on_cpu(tmp_path, n, "--full")
    k = min(n, 8)
    assert j["n_gpus"] == n and j["rccl_world"] == n and j["dist_backend"] == "gloo" and j["device"] == "cpu"
    # the mode names the backend that merged (a gloo rehearsal never claims RCCL)
    assert "gloo posterior merge" in j["config"]["mode"] and "RCCL" not in j["config"]["mode"]
    assert j["config"]["parallelism"] == "dp%d" % n and j["config"]["merges_per_step"] == k
    assert j["value"] == pytest.approx(n * 1000 * n / (j["ms_per_step"] / 1000.0))
    mm = j["merge_ms"]
    assert mm["prepass_placement"] and mm["buckets"] >= 1
    assert mm["collective"]  # which exchange merged (split / scan / bucketed all-reduce)
    acc = j["accuracy"]
    for key in ("records_dmu_median", "records_dmu_p99", "records_dmu_max", "spearman_mu_minus_sigma"):
        assert acc[key] is not None, key
    assert acc["merge_clamp_hits"] == 0
