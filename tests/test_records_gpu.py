"""Device-resident record arena on the MI355X: the ``records_select`` kernels (K10,
csrc/select.hip) against their host mirror, bit for bit, and ``records="resident"``
re-rates, history, kill / resume and export / load on the device."""
import pytest
import torch

from analyzer_amd.ops.rate import AFK, RateResult

import records_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K,M,P", C.shapes(), ids=C.SHAPE_IDS)
def test_select_device_equals_host_mirror(gpu_device, K, M, P):
    rec, rows = C.rated_window(K, M, P)
    drec, drows = rec.to(gpu_device), rows.to(gpu_device)
    for name, ids in C.query_sets(P, seed=M).items():
        bitmap = C.player_bitmap(ids, P, gpu_device)
        assert torch.equal(bitmap.cpu(), C.player_bitmap(ids, P, "cpu")), name
        hits = C.records_select(drec, drows, 77, P, bitmap)
        assert hits.is_cuda and hits.dtype == torch.int32 and hits.dim() == 2 and hits.shape[1] == 12, name
        host = C.select(rec, rows, 77, P, ids, "cpu")
        assert hits.shape[0] == host.shape[0] and torch.equal(hits.cpu(), host), name
        assert hits.shape[0] == 0 if name == "empty" else (M < 100 or hits.shape[0] > 0), name
        assert torch.equal(C.records_select(drec, drows, 77, P, bitmap), hits), name  # the same bits on every run


def test_select_device_afk_matches_keep_their_nan_fields(gpu_device):
    rec, rows = C.rated_window(1, 3000, 400)
    hits = C.select(rec, rows, 0, 400, range(400), gpu_device).cpu()
    afk = hits[(hits[:, 3] >> 8) == AFK]
    assert afk.shape[0] > 20 and bool(torch.isnan(afk[:, 4:9].contiguous().view(torch.float32)).any())
    assert torch.equal(hits, C.select(rec, rows, 0, 400, range(400), "cpu"))


def test_select_device_match_index_is_64_bit(gpu_device):
    rec, rows = C.rated_window(3, 257, 33)
    base = 5_000_000_000
    hits = C.select(rec, rows, base, 33, range(33), gpu_device).cpu()
    assert hits.shape[0] > 257 and bool((hits[:, 1] == 1).all())  # match_hi
    assert torch.equal(hits, C.select(rec, rows, base, 33, range(33), "cpu"))


def test_select_device_hand_built_records(gpu_device):
    C.check_hand_built(gpu_device)


@pytest.fixture(scope="module")
def resident3(gpu_device):
    return C.check_resident_equals_digest(C.SPEC3, gpu_device)


def test_resident_rows_equal_digest_run_rows_on_device(resident3):
    arena, rows = resident3
    assert arena.rows.is_cuda and arena.rows.shape == (5000, 32)
    # the device run computes what the host mirror's resident run computes, to fp32 rounding
    _, _, host = C.rerate_resident(C.SPEC3, "cpu", free_bytes=C.FREE)
    status = lambda a: RateResult.from_packed(a.filled_rows(), 3).status.cpu()  # noqa: E731
    assert torch.equal(status(arena), status(host))


def test_resident_rows_equal_digest_run_rows_5v5_on_device(gpu_device):
    arena, _ = C.check_resident_equals_digest(C.SPEC5, gpu_device)
    assert arena.rows.shape == (1700, 64)


def test_history_equals_brute_force_join_on_device(resident3, gpu_device):
    C.check_history(C.SPEC3, *resident3, gpu_device)


def test_history_of_a_player_who_never_played_on_device(gpu_device):
    C.check_player_who_never_played(gpu_device)


def test_kill_and_resume_fills_a_fresh_arena_on_device(resident3, gpu_device, tmp_path):
    arena = C.check_kill_and_resume(C.SPEC3, gpu_device, tmp_path, resident3[0])
    C.check_history(C.SPEC3, arena, resident3[1], gpu_device)


def test_export_load_round_trip_on_device(resident3, gpu_device, tmp_path):
    C.check_export_load(resident3[0], gpu_device, tmp_path)
