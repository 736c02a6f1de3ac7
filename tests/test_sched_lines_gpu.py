"""The chain path's links as whole lines (csrc/radix_sort.hip: sched_chain writes each link at
its slot's position in the partitioned arrays, one tile late through an LDS buffer, and
sched_unpartition carries the links back to slot order) against the C++ host mirror, bit for
bit on every stateful slot.  A prepass takes that path when it streams its input with
non-temporal loads, as the window pipeline's does beside the executor (ANA_SORT_NT=2 here);
tests/test_sched_chain_gpu.py covers the direct stores of a prepass alone.

Every case first proves on the CPU, from the records and the host links alone, that its input
has the property it is there for (``bucket_layout`` mirrors the partition: a bucket holds the
stateful slots of 4096 players in slot order, in tiles of 8192).  The shapes are the smallest
that have it: a bucket of a dozen tiles for the lag buffer, a one-player bucket, 256 buckets
with nearly empty runs, partial tiles, a match across two input tiles."""
import functools

import numpy as np
import pytest
import torch

from analyzer_amd.ops import rate as R
from analyzer_amd.ops.synth import RosterSpec, make_roster

from engine_parity import _stateful_slots
from test_engine_gpu import assert_close_to_fp64
from test_sched_chain_gpu import check_schedule, stream

pytestmark = pytest.mark.gpu

TILE = 8192  # slots per tile, of the partition's input and of a bucket
LOW = 12     # key bits a bucket's workgroup sorts by: 4096 players per bucket


@pytest.fixture(autouse=True)
def _chain_path(monkeypatch):
    monkeypatch.setenv("ANA_SCHED_CHAIN", "1")  # (unforced, windows this small take the LSD passes)
    monkeypatch.setenv("ANA_SORT_NT", "2")      # the prepass beside the executor: links as whole lines


def bucket_layout(rec, K, P):
    """(slot, player, bucket, tile of the bucket) of every stateful slot, in slot order: what
    the stable partition by the key bits above the low 12 makes of the window."""
    slots, _ = _stateful_slots(rec.numpy(), K, P)
    flat = np.flatnonzero(slots.reshape(-1))
    player = rec.numpy()[:, :2 * K].reshape(-1)[flat].astype(np.int64)
    bucket = player >> LOW
    pos = np.zeros(flat.size, np.int64)
    for b in np.unique(bucket):
        sel = bucket == b
        pos[sel] = np.arange(int(sel.sum()))
    return flat, player, bucket, pos // TILE


def link_tile_gaps(rec, K, P):
    """Per link between two consecutive slots of one player: how many bucket tiles apart."""
    flat, player, _, tile = bucket_layout(rec, K, P)
    order = np.lexsort((flat, player))
    same = player[order][1:] == player[order][:-1]
    return (tile[order][1:] - tile[order][:-1])[same]


def bucket_tiles(rec, K, P, b):
    _, _, bucket, tile = bucket_layout(rec, K, P)
    return int(tile[bucket == b].max()) + 1 if (bucket == b).any() else 0


@functools.lru_cache(maxsize=None)
def long_bucket():
    """P = 5000: bucket 0 (players 0..4095) takes four fifths of 120k slots."""
    return stream(5000, 20000, 3, p_hot=0.2, p_uneven=0.05)


@pytest.mark.parametrize("nt", ["2"])
def test_lag_buffer_and_older_tiles(gpu_device, monkeypatch, nt):
    """A bucket of 12 tiles: links resolved in the next tile (the LDS buffer), links deferred
    past it (the plain store at the bucket position, masked out of the flush), and the
    final flush.  The input has all three, by the host's own layout."""
    monkeypatch.setenv("ANA_SORT_NT", nt)
    P, K = 5000, 3
    rec = long_bucket()
    assert bucket_tiles(rec, K, P, 0) >= 12
    gaps = link_tile_gaps(rec, K, P)
    assert (gaps == 0).any() and (gaps == 1).any()
    assert (gaps > 2).any()  # some player's consecutive slots lie more than two bucket tiles apart
    check_schedule(rec, K, P, gpu_device)


def test_one_player_bucket(gpu_device):
    """4097 players: the second bucket holds player 4096 alone, its runs are 0 or 1 long."""
    P, M, K = 4097, 3000, 3
    rec = stream(P, M, K, p_hot=0.2, p_uneven=0.05)
    _, player, bucket, _ = bucket_layout(rec, K, P)
    assert (bucket == 1).any() and set(player[bucket == 1]) == {4096}
    check_schedule(rec, K, P, gpu_device)


@pytest.mark.parametrize("P,M", [(2**20 - 1, 3000), (2**20, 3000), (2**20 - 1, 1400)])
def test_full_width_short_runs(gpu_device, P, M):
    """256 buckets: with 18k slots the (tile, bucket) runs average less than a 128-B line (none
    of the 768 is empty, by count); with 8400 slots the second tile has 208, so many of its
    runs are empty.  (2^20 players need 21 key bits: that roster takes the LSD passes.)"""
    K = 3
    rec = stream(P, M, K, p_uneven=0.05)
    flat, _, bucket, _ = bucket_layout(rec, K, P)
    assert np.unique(bucket).size == 256
    runs = np.unique((flat // TILE) * 256 + bucket).size  # non-empty (input tile, bucket) runs
    assert flat.size / runs < 32
    if M == 1400:
        assert runs < 2 * 256 - 64  # at least 64 empty runs
    check_schedule(rec, K, P, gpu_device, untouched=True)


@pytest.mark.parametrize("M", [1366, 1500, 4097])
def test_partial_last_tile(gpu_device, M):
    """Slot counts that are no multiple of 8192.  1366 matches are 8196 slots: match 1365 lies
    across two input tiles, and the last tile has 4 slots and 252 empty runs."""
    P, K = 5000, 3
    rec = stream(P, M, K, p_hot=0.2)
    assert (M * 2 * K) % TILE != 0
    if M == 1366:
        m = TILE // (2 * K)
        assert m * 2 * K < TILE < (m + 1) * 2 * K
        rec[m] = rec[0]  # (a match that rates)
        slots, _ = _stateful_slots(rec.numpy(), K, P)
        assert slots.reshape(-1)[TILE - 2:TILE + 4].all()
    check_schedule(rec, K, P, gpu_device)


@pytest.mark.parametrize("K,M", [(1, 20000), (5, 4000)])
def test_team_sizes(gpu_device, K, M):
    """The slot -> match division by 2 and by 10, runs at odd alignments; bucket 0 of 4 tiles."""
    P = 5000
    rec = stream(P, M, K, p_hot=0.2, p_uneven=0.05)
    assert bucket_tiles(rec, K, P, 0) >= 3
    assert (link_tile_gaps(rec, K, P) > 1).any()
    check_schedule(rec, K, P, gpu_device)


@pytest.mark.parametrize("case", ["every_match", "twice", "skew3"])
def test_hot_players_and_duplicates(gpu_device, case):
    """The cases of test_chain_hot_players_and_duplicates with a bucket 0 of three tiles or
    more: one player with a run in every tile (its table entry and its deferred link renewed
    per tile), matches that name a player twice, a power-law stream."""
    K = 3
    if case == "skew3":
        P, M = 100_000, 20_000
        rec = stream(P, M, K, skew=3)
    else:
        P, M = 5000, 6000
        rec = stream(P, M, K, seed=1)
        if case == "every_match":
            rec[:, 0] = 7
        else:
            rec[::3, K] = rec[::3, 0]
            rec[1::7, 1] = rec[1::7, 0]
    tiles0 = bucket_tiles(rec, K, P, 0)
    assert tiles0 >= 3
    if case == "every_match":
        _, player, _, tile = bucket_layout(rec, K, P)
        assert np.unique(tile[player == 7]).size == tiles0
    check_schedule(rec, K, P, gpu_device)


@pytest.mark.parametrize("P", [3000, 5000, 2**20 - 1])
def test_stateless_slots_stay_untouched(gpu_device, P):
    """AFK, unsupported and invalid matches, short rosters.  Their key "no state" has a bucket
    of its own that nobody chains (5000 players), shares the last chained bucket with players
    (2^20 - 1: all 256 digits are taken), or there is no partition at all (3000)."""
    M, K = 3000, 3
    rec = stream(P, M, K, p_afk=0.2, p_unsupported=0.1, p_uneven=0.2, p_bad_rosters=0.1)
    slots, _ = _stateful_slots(rec.numpy(), K, P)
    assert 0.2 < (~slots).mean() < 0.8
    nb = ((P - 1) >> LOW) + 1
    assert (nb < 256) == (P == 5000) or P == 3000
    check_schedule(rec, K, P, gpu_device, untouched=True)


@pytest.mark.parametrize("parts", ["2", "3"])
def test_link_parts_change_nothing(gpu_device, monkeypatch, parts):
    """ANA_LINK_PARTS no longer splits this path (one chain launch in the kernel trace): the
    links are the host's, and no other slot is written."""
    monkeypatch.setenv("ANA_LINK_PARTS", parts)
    P, M, K = 5000, 6000, 3
    rec = stream(P, M, K, p_hot=0.2, p_afk=0.1)
    assert bucket_tiles(rec, K, P, 0) >= 3
    check_schedule(rec, K, P, gpu_device, untouched=True)


def test_rates_like_host_on_the_new_links(gpu_device):
    """One window end to end over the 12-tile bucket: statuses equal, ratings within the
    device-vs-fp64 tolerance of test_engine_gpu, no error flag."""
    P, K = 5000, 3
    rec = long_bucket()
    roster = make_roster(RosterSpec(num_players=P, seed=3))
    host = roster.clone()
    rh = R.BatchRater(host_fp64=True).rate(host, rec, K)
    dev = roster.to(gpu_device)
    rater = R.BatchRater()
    rd = rater.rate(dev, rec.to(gpu_device), K)
    assert int(rater.error_flags(gpu_device).sum()) == 0
    np.testing.assert_array_equal(rd.status.cpu().numpy(), rh.status.numpy())
    assert_close_to_fp64(rd, dev, rh, host)
