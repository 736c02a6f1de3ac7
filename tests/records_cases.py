"""Shared cases of the record-arena tests (test_records.py on the CPU,
test_records_gpu.py on the device): rated windows to select from, a plain Python
reference of ``records_select``, hand-built records, and the re-rate comparisons
that run the same way on either device."""
import functools

import numpy as np
import pytest
import torch

from analyzer_amd.ops.native import native
from analyzer_amd.ops.rate import (AFK, ERR_BAD_RECORD, INVALID_ROSTERS, NOT_PROCESSED, RATED, UNSUPPORTED_MODE,
                                   BatchRater, RateResult)
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream
from analyzer_amd.runtime import checkpoint
from analyzer_amd.runtime.records import RecordArena, player_bitmap, records_select
from analyzer_amd.runtime.rerate import InjectedFault, RerateSpec, rerate_resident, run, stream_records


TILE = 2048  # matches per workgroup of the select kernels (csrc/kernels.h kSelectTile; checked below)


def shapes():
    """(K, M, P): one match, a wave / workgroup-iteration edge with a bitmap word edge,
    one past the kernel's tile, several tiles, the 8-B-aligned record sizes (K = 2, 4)
    and every vector-load path (K = 1..5)."""
    return [(3, 1, 10), (3, 257, 33), (2, TILE + 1, 64), (1, 3000, 400), (4, 1000, 100), (5, 5000, 700)]


def check_tile():
    assert int(native().SELECT_TILE) == TILE and int(native().HIT_WORDS) == 12


SHAPE_IDS = ["K3-M1", "K3-M257", "K2-tile+1", "K1-M3000", "K4-M1000", "K5-M5000"]
FREE = 1 << 40  # the arenas of these tests are never sized from the real free memory


@functools.lru_cache(maxsize=None)
def rated_window(K, M, P):
    """(rec, rows) on the CPU: a stream with AFK, unsupported and uneven matches, rated
    by the host mirror once and shared (never modified) by the tests that select from it."""
    roster = make_roster(RosterSpec(num_players=P, seed=3 + K))
    rec = make_stream(StreamSpec(team_size=K, seed=17 + M, p_afk=0.05, p_unsupported=0.05, p_uneven=0.1), M, P, K=K)
    res = BatchRater().rate(roster, rec, K)
    return rec, res.packed


def query_sets(P, seed=0):
    g = torch.Generator().manual_seed(seed)
    some = torch.randperm(P, generator=g)[:max(1, round(0.05 * P))]
    return {"empty": [], "one": [int(torch.randint(P, (1,), generator=g))], "every": list(range(P)),
            "random5%": sorted(int(p) for p in some)}


def select_ref(rec, rows, base, P, ids):
    """``records_select`` as a plain loop: hits [n, 12] int32."""
    r_ = rec.numpy()
    w_ = rows.view(torch.int32).numpy()
    M, S = r_.shape[0], r_.shape[1] - 2
    K = S // 2
    query = {int(p) for p in ids if 0 <= int(p) < P}
    out = []
    for m in range(M):
        r = r_[m]
        m0 = int(r[S]) & 0xFFFFFFFF
        n0, n1 = (m0 >> 8) & 0xFF, (m0 >> 16) & 0xFF
        for j in range(S):
            if (j if j < K else j - K) >= (n0 if j < K else n1):
                continue
            p = int(r[j])
            if p < 0 or p >= P or p not in query:
                continue
            st = int(w_[m, 5 * S + 1]) & 0xFF
            if st not in (RATED, AFK, INVALID_ROSTERS):
                break
            g = base + m
            out.append([g & 0xFFFFFFFF, g >> 32, p, j | (st << 8)] + [int(w_[m, f * S + j]) for f in range(5)]
                       + [int(w_[m, 5 * S]), int(r[S]), int(r[S + 1])])
    a = np.array(out, dtype=np.int64).reshape(-1, 12).astype(np.uint32).view(np.int32)
    return torch.from_numpy(a.copy())


def select(rec, rows, base, P, ids, device):
    return records_select(rec.to(device), rows.to(device), base, P, player_bitmap(ids, P, device))


# ------------------------------------------------------------------ hand-built records
HAND_P = 45  # P % 32 != 0
HAND_QUERY = [7, 44]


def hand_built():
    """K = 3 records with rows of random bit patterns (NaNs included) under chosen status
    bytes; returns (rec, rows, expected (match, slot) pairs of the query [7, HAND_P - 1])."""
    K, S = 3, 6
    meta0 = lambda mode, n0, n1, nr=2: mode | (n0 << 8) | (n1 << 16) | (nr << 24)  # noqa: E731
    cases = [
        # players,                         meta0,             meta1, status,           hits (slots)
        ([7, 1, 2, 7, 3, 4],               meta0(1, 3, 3),    1,     RATED,            [0, 3]),  # both teams
        ([5, 6, 44, 8, 9, 10],             meta0(0, 3, 3),    2,     RATED,            [2]),     # player P - 1
        ([11, 12, 7, 13, 14, 44],          meta0(2, 2, 2),    1,     RATED,            []),      # past n0 / n1
        ([7, 45, 2, 2 ** 31 - 1, -5, 3],   meta0(1, 3, 3),    1,     ERR_BAD_RECORD,   []),      # ids outside [0, P)
        ([7, 1, 2, 44, 3, 4],              meta0(255, 3, 3),  1,     UNSUPPORTED_MODE, []),      # nothing written
        ([15, 7, 2, 16, 3, 4],             meta0(1, 3, 3),    1 | 4 | (2 << 8), AFK,   [1]),     # AFK: NULL fields
        ([15, 1, 2, 16, 44, 4],            meta0(1, 3, 3, 3), 1,     INVALID_ROSTERS,  [4]),
        ([7, 1, 2, 16, 3, 44],             meta0(1, 3, 3),    1,     NOT_PROCESSED,    []),
        ([20, 21, 22, 23, 24, 25],         meta0(1, 3, 3),    1,     RATED,            []),      # nobody queried
    ]
    M = len(cases)
    rec = torch.tensor([c[0] + [c[1], c[2]] for c in cases], dtype=torch.int64).to(torch.int32)
    g = torch.Generator().manual_seed(5)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (M, RateResult.row_floats(K)), generator=g, dtype=torch.int64)
    words[5, :5 * S] = 0x7FC00000  # the AFK match's slot fields are NULL
    words[:, 5 * S + 1] = torch.tensor([c[3] for c in cases]) | 0x5A5A00  # only the low byte is the status
    rows = words.to(torch.int32).view(torch.float32)
    expect = [(m, j) for m, c in enumerate(cases) for j in c[4]]
    return rec, rows, expect


def check_hand_built(device):
    rec, rows, expect = hand_built()
    base = 1000
    hits = select(rec, rows, base, HAND_P, HAND_QUERY, device).cpu()
    assert [(int(h[0]) - base, int(h[3]) & 0xFF) for h in hits] == expect
    assert torch.equal(hits, select_ref(rec, rows, base, HAND_P, HAND_QUERY))
    afk = hits[(hits[:, 3] >> 8) == AFK]
    assert afk.shape[0] == 1 and bool((afk[0, 4:9] == 0x7FC00000).all())  # the NaN stays that NaN
    # ids >= P or < 0 in the query itself are dropped, not probed
    assert torch.equal(select(rec, rows, base, HAND_P, HAND_QUERY + [45, 99, -1, 2 ** 31 - 1], device).cpu(), hits)


# ------------------------------------------------------------------ re-rate comparisons
SPEC3 = RerateSpec(total_matches=5000, players=300, team_size=3, window=1200)  # the last window is short
SPEC5 = RerateSpec(total_matches=1700, players=200, team_size=5, window=500)


def payload(rows, K):
    """The defined part of packed rows as integers: the 5 * 2K slot fields and the quality
    as int32 bit patterns, and the status byte.  The rest of a row (the status word's upper
    bytes, the padding up to the row length for K != 3) is never written by the host mirror
    and holds whatever its ``torch.empty`` memory held."""
    n = 5 * 2 * K + 1
    return torch.cat([rows.view(torch.int32)[:, :n], (rows.view(torch.int32)[:, n:n + 1] & 0xFF)], dim=1).cpu()


def digest_run(spec, device, **kw):
    clones = {}
    metrics, roster = run(spec, device, records="digest",
                          on_window=lambda g, res: clones.__setitem__(g, res.packed.clone()), **kw)
    return metrics, roster, torch.cat([clones[g] for g in sorted(clones)])


def same_roster(a, b):
    return torch.equal(a.state[:, 0::2].cpu().nan_to_num(-7), b.state[:, 0::2].cpu().nan_to_num(-7))


def check_resident_equals_digest(spec, device):
    """Returns (arena, the digest run's rows) for further checks."""
    dm, droster, rows = digest_run(spec, device)
    rm, rroster, arena = rerate_resident(spec, device, free_bytes=FREE)
    K = spec.team_size
    assert arena.filled == spec.total_matches == arena.matches and arena.first_match == 0
    assert arena.rows.device.type == torch.device(device).type
    assert torch.equal(payload(arena.filled_rows(), K), payload(rows, K))
    assert rm["window_digests"] == dm["window_digests"]
    assert len(rm["window_digests"]) == -(-spec.total_matches // spec.window)
    assert same_roster(rroster, droster)
    for k in ("matches", "rated", "afk", "match_records", "participant_records"):
        assert rm[k] == dm[k]
    return arena, rows


def brute_force_history(spec, rows, players, lo=0):
    """Join of the digest run's rows [lo, total) with the regenerated stream."""
    rec = make_stream(spec.stream_spec(), spec.total_matches - lo, spec.players, K=spec.team_size, base=lo)
    return select_ref(rec, rows[lo:].cpu(), lo, spec.players, players)


def never_played(spec):
    rec = make_stream(spec.stream_spec(), spec.total_matches, spec.players, K=spec.team_size)
    seen = torch.zeros(spec.players, dtype=torch.bool)
    ids = rec[:, :2 * spec.team_size].reshape(-1).to(torch.int64)
    seen[ids[(ids >= 0) & (ids < spec.players)]] = True
    return [int(p) for p in (~seen).nonzero().reshape(-1)]


def check_history(spec, arena, rows, device):
    players = [0, 3, 17, 42, 99, 150, 151, 222, 298, 299]
    hist = arena.history(players, spec.players, stream_records(spec, device))
    ref = brute_force_history(spec, rows, players, arena.first_match)
    n = ref.shape[0]
    assert n > 50 and hist["match"].dtype == torch.int64 and hist["match"].shape[0] == n
    m = hist["match"].cpu()
    assert bool((m[1:] >= m[:-1]).all()) and int(m[0]) >= arena.first_match
    assert torch.equal(m, (ref[:, 0].to(torch.int64) & 0xFFFFFFFF) | (ref[:, 1].to(torch.int64) << 32))
    assert torch.equal(hist["player"].cpu(), ref[:, 2])
    assert torch.equal(hist["slot"].cpu(), ref[:, 3] & 0xFF) and torch.equal(hist["status"].cpu(), ref[:, 3] >> 8)
    for i, name in enumerate(("s_mu", "s_sig", "delta", "m_mu", "m_sig", "quality")):
        assert hist[name].dtype == torch.float32
        assert torch.equal(hist[name].cpu().view(torch.int32), ref[:, 4 + i])
    assert torch.equal(hist["meta"].cpu(), ref[:, 10:12])
    assert bool((hist["status"] == AFK).any()) and bool(torch.isnan(hist["delta"]).any())


# every one of SPEC3's 300 players plays; this history is sparse enough to leave some out
SPEC_SPARSE = RerateSpec(total_matches=700, players=6000, team_size=3, window=300)


def check_player_who_never_played(device):
    spec = SPEC_SPARSE
    idle = never_played(spec)
    assert idle
    _, _, arena = rerate_resident(spec, device, free_bytes=FREE)
    rec_of = stream_records(spec, device)
    nobody = arena.history(idle[:1], spec.players, rec_of)
    assert all(v.shape[0] == 0 for v in nobody.values()) and nobody["meta"].shape == (0, 2)
    played = int(make_stream(spec.stream_spec(), 1, spec.players, K=3)[0, 0])
    both = arena.history([idle[0], played], spec.players, rec_of)
    assert both["match"].shape[0] >= 1 and bool((both["player"] == played).all())


def check_kill_and_resume(spec, device, tmp_path, full_arena):
    d = str(tmp_path / "ck")
    with pytest.raises(InjectedFault):
        rerate_resident(spec, device, checkpoint_dir=d, checkpoint_every=2, fault_kill_after=3, free_bytes=FREE)
    _, meta = checkpoint.load(d + "/latest")
    assert meta["windows_done"] == 2 and meta["records"] == "resident" and meta["arena_extent"] == 2 * spec.window
    metrics, _, arena = rerate_resident(spec, device, checkpoint_dir=d, checkpoint_every=2, free_bytes=FREE)
    off = 2 * spec.window
    assert metrics["resumed_from_window"] == 2 and meta["next_offset"] == off
    assert arena.first_match == off and arena.filled == arena.matches == spec.total_matches - off
    K = spec.team_size
    assert torch.equal(payload(arena.filled_rows(), K), payload(full_arena.filled_rows()[off:], K))
    assert torch.equal(payload(arena.result(off, off + spec.window).packed, K),
                       payload(full_arena.result(off, off + spec.window).packed, K))
    with pytest.raises(IndexError):
        arena.result(0, spec.window)  # a window from before the resume point is not held
    return arena


def check_export_load(arena, device, tmp_path):
    from analyzer_amd.runtime import records

    path = str(tmp_path / "records.bin")
    slot = records.EXPORT_SLOT_BYTES
    records.EXPORT_SLOT_BYTES = 7 * 128 * 100 + 4  # many chunks through the two slots, a short last one
    try:
        nbytes = arena.export(path)
        assert nbytes == arena.filled * arena.W * 4
        back = RecordArena.load(path, device)
    finally:
        records.EXPORT_SLOT_BYTES = slot
    assert (back.K, back.W, back.filled, back.first_match, back.rank, back.size, back.window) == \
        (arena.K, arena.W, arena.filled, arena.first_match, arena.rank, arena.size, arena.window)
    assert back.rows.device.type == torch.device(device).type
    assert torch.equal(back.filled_rows().view(torch.int32).cpu(), arena.filled_rows().view(torch.int32).cpu())
    with open(path, "r+b") as f:
        f.truncate(nbytes - 4)
    with pytest.raises(ValueError):
        RecordArena.load(path, device)
