"""Device-resident record arena and player-history queries on the CPU: the host
mirror of ``records_select`` (K10) against a plain Python loop, the arena's geometry,
sizing plan and persistence, and ``records="resident"`` re-rates against the digest
mode (gloo for the two-rank case)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from analyzer_amd.ops.rate import AFK, RateResult
from analyzer_amd.runtime.records import RESERVE_FRACTION, RecordArena, local_extent, player_bitmap
from analyzer_amd.runtime.rerate import ArenaDoesNotFit, RerateSpec, rerate_resident, run, window_slice

import records_cases as C
from test_distributed import run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ K10 host mirror
@pytest.mark.parametrize("K,M,P", C.shapes(), ids=C.SHAPE_IDS)
def test_select_host_mirror_equals_python_loop(K, M, P):
    rec, rows = C.rated_window(K, M, P)
    for name, ids in C.query_sets(P, seed=M).items():
        hits = C.select(rec, rows, 77, P, ids, "cpu")
        assert hits.dtype == torch.int32 and hits.dim() == 2 and hits.shape[1] == 12, name
        assert torch.equal(hits, C.select_ref(rec, rows, 77, P, ids)), name
        assert hits.shape[0] == 0 if name == "empty" else (M < 100 or hits.shape[0] > 0), name
        assert torch.equal(hits, C.select(rec, rows, 77, P, ids, "cpu")), name  # the same bits on every call


def test_select_shapes_straddle_the_kernel_tile():
    C.check_tile()


def test_select_afk_matches_keep_their_nan_fields():
    rec, rows = C.rated_window(1, 3000, 400)
    hits = C.select(rec, rows, 0, 400, range(400), "cpu")
    afk = hits[(hits[:, 3] >> 8) == AFK]
    assert afk.shape[0] > 20
    assert bool(torch.isnan(afk[:, 4:9].contiguous().view(torch.float32)).any())
    assert torch.equal(hits, C.select_ref(rec, rows, 0, 400, range(400)))


def test_select_match_index_is_64_bit():
    rec, rows = C.rated_window(3, 257, 33)
    base = 5_000_000_000
    hits = C.select(rec, rows, base, 33, range(33), "cpu")
    assert hits.shape[0] > 257 and bool((hits[:, 1] == 1).all())  # match_hi
    assert torch.equal(hits, C.select_ref(rec, rows, base, 33, range(33)))
    from analyzer_amd.runtime.records import hits_columns

    m = hits_columns(hits)["match"]
    assert int(m.min()) >= base and int(m.max()) < base + 257 and bool((m[1:] >= m[:-1]).all())


def test_select_hand_built_records():
    C.check_hand_built("cpu")


def test_player_bitmap_words():
    bm = player_bitmap([0, 31, 32, 44, 44, -3, 45, 1000], 45, "cpu")
    assert bm.dtype == torch.int32 and bm.tolist() == [1 - 2 ** 31, 1 | (1 << 12)]
    assert player_bitmap([], 45, "cpu").tolist() == [0, 0]


def test_select_rejects_mismatched_inputs():
    rec, rows = C.rated_window(3, 257, 33)
    bm = player_bitmap([1], 33, "cpu")
    with pytest.raises(RuntimeError):
        C.records_select(rec, rows[:100], 0, 33, bm)     # rows of other matches
    with pytest.raises(RuntimeError):
        C.records_select(rec, rows, 0, 33 + 64, bm)      # a bitmap too short for P
    with pytest.raises(RuntimeError):
        C.records_select(rec, rows[:, :16].contiguous(), 0, 33, bm)  # not packed rows of K = 3


# ------------------------------------------------------------------ the arena
def test_from_packed_is_what_allocate_builds():
    a = RateResult.allocate(10, 4, "cpu")
    b = RateResult.from_packed(a.packed, 4)
    for f in RateResult.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.data_ptr() == y.data_ptr() and x.shape == y.shape and x.stride() == y.stride() and x.dtype == y.dtype
    assert b.packed is a.packed
    with pytest.raises(ValueError):
        RateResult.from_packed(a.packed, 3)


def test_arena_geometry_and_filled_extent():
    spec = RerateSpec(total_matches=5000, players=10, team_size=3, window=700)
    size = 3
    held = 0
    for rank in range(size):
        n = local_extent(spec.total_matches, spec.window, rank, size)
        held += n
        arena = RecordArena(n, 3, "cpu", rank=rank, size=size, window=spec.window)
        rows = torch.arange(n, dtype=torch.int64)
        g = arena.global_match(rows)
        assert torch.equal(arena.local_row(g), rows) and int(arena.local_row(int(g[-1]))) == n - 1
        # the rank's blocks, back to back
        blocks = [window_slice(spec, w, rank, size) for w in range(3)]
        assert torch.equal(g, torch.cat([torch.arange(lo, hi) for lo, hi in blocks]))
        with pytest.raises(IndexError):
            arena.local_row(int(g[0]) + spec.window)  # the next rank's block
        # filled in order; nothing is readable before it was filled
        with pytest.raises(IndexError):
            arena.result(*blocks[0])
        with pytest.raises(IndexError):
            arena.result(*blocks[1], fill=True)
        res = arena.result(*blocks[0], fill=True)
        assert res.packed.data_ptr() == arena.rows.data_ptr() and res.packed.shape == (700, 32)
        arena.commit()
        assert arena.filled == 700 and arena.result(*blocks[0]).s_mu.shape == (700, 6)
        assert list(arena.windows()) == [blocks[0]]
        with pytest.raises(IndexError):
            arena.result(*blocks[1])
    assert held == spec.total_matches
    with pytest.raises(ValueError):
        RecordArena(10, 3, "cpu", first_match=5, window=10)  # not the start of a window


def test_plan_fits_flips_at_the_reserve():
    assert RESERVE_FRACTION == 0.10
    total, matches = 1_000_000, 7200
    need = matches * 128 + total // 10
    for players in (0, 10):
        roster = players * 144
        at = RecordArena.plan(matches, 3, free_bytes=need + roster, total_bytes=total, roster_players=players)
        below = RecordArena.plan(matches, 3, free_bytes=need + roster - 1, total_bytes=total, roster_players=players)
        assert at["fits"] is True and below["fits"] is False
        assert at["row_bytes"] == 128 and at["arena_bytes_per_rank"] == matches * 128 and at["roster_bytes"] == roster
        assert at["free_bytes"] == need + roster and at["total_bytes"] == total and at["reserve_bytes"] == total // 10
    wide = RecordArena.plan(1000, 5, size=8, free_bytes=1 << 30)
    assert wide["row_bytes"] == 256 and wide["arena_bytes_per_rank"] == 125 * 256 and wide["total_bytes"] == 1 << 30
    # with the window: the largest rank's blocks, exactly
    assert RecordArena.plan(1000, 3, size=2, free_bytes=1 << 30, window=300)["matches_per_rank"] == 600
    with pytest.raises(ArenaDoesNotFit) as e:
        rerate_resident(C.SPEC3, "cpu", free_bytes=5000 * 128)  # the whole free memory: no reserve left
    assert e.value.plan["fits"] is False


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "analyzer_amd.runtime.rerate", "--device", "cpu", "--matches", "900",
                           "--players", "120", "--window", "400", "--records", "resident", *args],
                          capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)


def test_cli_plan_history_export(tmp_path):
    path = str(tmp_path / "rows.bin")
    ok = _cli("--arena-free-bytes", str(1 << 30), "--history", "5,7", "--export-records", path)
    assert ok.returncode == 0, ok.stderr
    lines = [json.loads(ln) for ln in ok.stdout.splitlines() if ln.startswith("{")]
    plan = lines[0]["arena_plan"]
    assert plan["fits"] and plan["arena_bytes_per_rank"] == 900 * 128 and plan["roster_bytes"] == 120 * 144
    assert lines[1]["matches"] == 900 and lines[1]["arena_rows"] == 900
    five, seven = lines[2], lines[3]
    assert five["player"] == 5 and seven["player"] == 7 and five["records"] == len(five["match"]) > 0
    assert five["match"] == sorted(five["match"]) and len(five["s_mu"]) == five["records"]
    assert lines[4]["exported"] == path and os.path.getsize(path) == 900 * 128 == lines[4]["bytes"]
    assert RecordArena.load(path).filled == 900
    # the arena would take all but less than the reserve: the report, then exit code 2
    no = _cli("--arena-free-bytes", str(900 * 128 + 120 * 144 + 100))
    assert no.returncode == 2 and "does not fit" in no.stderr
    report = json.loads(no.stdout.splitlines()[0])["arena_plan"]
    assert report["fits"] is False and len(no.stdout.splitlines()) == 1


# ------------------------------------------------------------------ resident re-rates
@pytest.fixture(scope="module")
def resident3():
    return C.check_resident_equals_digest(C.SPEC3, "cpu")


def test_resident_rows_equal_digest_run_rows(resident3):
    arena, rows = resident3
    assert arena.rows.shape == (5000, 32) and list(arena.windows())[-1] == (4800, 5000)


def test_resident_rows_equal_digest_run_rows_5v5():
    arena, _ = C.check_resident_equals_digest(C.SPEC5, "cpu")
    assert arena.rows.shape == (1700, 64)


def test_history_equals_brute_force_join(resident3):
    C.check_history(C.SPEC3, *resident3, "cpu")


def test_history_of_a_player_who_never_played():
    C.check_player_who_never_played("cpu")


def test_kill_and_resume_fills_a_fresh_arena(resident3, tmp_path):
    arena = C.check_kill_and_resume(C.SPEC3, "cpu", tmp_path, resident3[0])
    # history over the resumed arena: only what it holds
    C.check_history(C.SPEC3, arena, resident3[1], "cpu")


def test_export_load_round_trip(resident3, tmp_path):
    C.check_export_load(resident3[0], "cpu", tmp_path)


def test_run_requires_an_arena_that_matches():
    with pytest.raises(ValueError):
        run(C.SPEC3, "cpu", records="resident")
    with pytest.raises(ValueError):
        run(C.SPEC3, "cpu", records="resident", arena=RecordArena(5000, 5, "cpu", window=1200))
    with pytest.raises(ValueError):
        run(C.SPEC3, "cpu", records="digest", arena=RecordArena(5000, 3, "cpu", window=1200))


def _two_ranks(rank, size, spec):
    K = spec.team_size
    _, _, rows = C.digest_run(spec, "cpu")
    metrics, roster, arena = rerate_resident(spec, "cpu", free_bytes=C.FREE)
    local = torch.arange(arena.filled, dtype=torch.int64)
    g = arena.global_match(local)
    blocks = [window_slice(spec, w, rank, size) for w in range(int(metrics["windows"]))]
    return {"rows_equal": torch.equal(C.payload(arena.filled_rows(), K), C.payload(rows, K)),
            "filled": arena.filled, "global": g, "inverse_ok": torch.equal(arena.local_row(g), local),
            "blocks": torch.cat([torch.arange(lo, hi) for lo, hi in blocks]),
            "windows": [list(w) for w in arena.windows()]}


def test_resident_rerate_two_ranks(tmp_path):
    spec = RerateSpec(total_matches=1300, players=500, team_size=3, window=200, seed=5)
    res = run_ranks(_two_ranks, 2, tmp_path, spec)
    assert [r["filled"] for r in res] == [700, 600]
    for rank, r in enumerate(res):
        assert r["rows_equal"] and r["inverse_ok"] and torch.equal(r["global"], r["blocks"])
        assert r["windows"][0] == [rank * 200, rank * 200 + 200]
    both = torch.cat([r["global"] for r in res]).sort().values
    assert torch.equal(both, torch.arange(1300))
