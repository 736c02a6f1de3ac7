"""The schedule prepass's chain path (csrc/radix_sort.hip sched_chain: one partition by the
high key bits, then one workgroup per bucket with a last-occurrence table in LDS) against
the C++ host mirror, bit for bit, next to the three LSD passes (ANA_SCHED_CHAIN=0).

A tile is 8192 slots and the chain's table holds 2^12 players, so the cases are small: one
to three tiles, rosters on both sides of 2^12 (no partition / two buckets) and of 2^20 (the
chain path's limit), hot players that span tiles, stateless slots, link parts."""
import numpy as np
import pytest
import torch

from analyzer_amd.ops import rate as R
from analyzer_amd.ops.synth import RosterSpec, StreamSpec, make_roster, make_stream

from engine_parity import _stateful_slots
from test_engine_gpu import assert_close_to_fp64

pytestmark = pytest.mark.gpu

CHAIN = pytest.mark.parametrize("chain", ["1", "0"])
SENTINEL = 0x5A5A5A5A


def check_schedule(rec, K, P, dev, untouched=False):
    """link (on every slot the host defines) and the readiness counts the executor derives
    from it, device against host.  ``untouched``: the device leaves every other slot alone."""
    br = R.BatchRater()
    link_h, deps_h = (t.clone() for t in br.schedule(rec, K, P))
    rec_d = rec.to(dev)
    if untouched:
        br.schedule(rec_d, K, P)[0].fill_(SENTINEL)  # the buffer the next schedule writes
    link_d, deps_d = br.schedule(rec_d, K, P)
    slots, first = _stateful_slots(rec.numpy(), K, P)
    link_d = link_d.cpu().numpy()
    np.testing.assert_array_equal(link_d[slots], link_h.numpy()[slots])
    assert int(deps_d.abs().sum()) == 0  # device counters start at 0
    need = (first & ((link_d & R.Schedule.HAS_PRED) != 0)).sum(1)
    rated = slots.any(1)
    np.testing.assert_array_equal(need[rated], deps_h.numpy()[rated])
    if untouched:
        assert (~slots).any()
        np.testing.assert_array_equal(link_d[~slots], np.int32(SENTINEL))


def stream(P, M, K, seed=0, **kw):
    kw.setdefault("p_afk", 0.05)
    return make_stream(StreamSpec(team_size=K, seed=P + M + seed, **kw), M, P, K=K)


# top == 0 (<= 4096 players, no partition): less than a tile; three tiles on both sides of
# the 12-bit boundary (4096 players: 13 key bits, two buckets, the second only "no state")
# two buckets: kend falls into a bucket that also holds players
# full width: most players once, many buckets per tile; 2^20 players: the LSD passes
# M = 1; 1366 * 6 = 8196 slots: a last tile of 4
@CHAIN
@pytest.mark.parametrize("P,M,K", [(50, 200, 3), (4095, 3000, 3), (4096, 3000, 3), (5000, 3000, 3),
                                   (1_000_000, 4000, 3), (2**20 - 1, 4000, 3), (2**20, 4000, 3),
                                   (5000, 2000, 1), (5000, 2000, 5), (5000, 1, 3), (3000, 1366, 3),
                                   (50, 3000, 3), (5000, 5000, 1), (5000, 3000, 2), (5000, 3000, 4)])
def test_chain_matches_host(gpu_device, monkeypatch, chain, P, M, K):
    monkeypatch.setenv("ANA_SCHED_CHAIN", chain)
    check_schedule(stream(P, M, K, p_hot=0.2, p_uneven=0.05), K, P, gpu_device)


@CHAIN
@pytest.mark.parametrize("case", ["every_match", "twice", "skew3"])
def test_chain_hot_players_and_duplicates(gpu_device, monkeypatch, chain, case):
    """One player in every match (a run through every tile of its bucket, the table entry
    rewritten per tile), matches that name a player twice (successor = the same match), and
    a power-law stream (large buckets, long runs)."""
    monkeypatch.setenv("ANA_SCHED_CHAIN", chain)
    K = 3
    if case == "skew3":
        P, M = 100_000, 20_000
        rec = stream(P, M, K, skew=3)
    else:
        P, M = 5000, 3000
        rec = stream(P, M, K, seed=1)
        if case == "every_match":
            rec[:, 0] = 4097
        else:
            rec[::3, K] = rec[::3, 0]
            rec[1::7, 1] = rec[1::7, 0]
    check_schedule(rec, K, P, gpu_device)


@CHAIN
@pytest.mark.parametrize("P", [3000, 5000])
def test_chain_skips_stateless_slots(gpu_device, monkeypatch, chain, P):
    """AFK, unsupported and invalid matches and short rosters: their slots (key = "no
    state") get no link and leave no trace in the links of the others."""
    monkeypatch.setenv("ANA_SCHED_CHAIN", chain)
    rec = stream(P, 3000, 3, p_afk=0.2, p_unsupported=0.1, p_uneven=0.2, p_bad_rosters=0.1)
    check_schedule(rec, 3, P, gpu_device, untouched=True)


@CHAIN
@pytest.mark.parametrize("parts", ["2", "3"])
def test_chain_link_parts(gpu_device, monkeypatch, chain, parts):
    monkeypatch.setenv("ANA_SCHED_CHAIN", chain)
    monkeypatch.setenv("ANA_LINK_PARTS", parts)
    check_schedule(stream(5000, 3000, 3, p_hot=0.2), 3, 5000, gpu_device, untouched=True)


@CHAIN
def test_chain_rates_like_host(gpu_device, monkeypatch, chain):
    """One window end to end: statuses equal, ratings within the device-vs-fp64 tolerance
    of test_engine_gpu, no error flag."""
    monkeypatch.setenv("ANA_SCHED_CHAIN", chain)
    P, M, K = 5000, 3000, 3
    roster = make_roster(RosterSpec(num_players=P, seed=3))
    rec = stream(P, M, K, p_hot=0.2)
    host = roster.clone()
    rh = R.BatchRater(host_fp64=True).rate(host, rec, K)
    dev = roster.to(gpu_device)
    rater = R.BatchRater()
    rd = rater.rate(dev, rec.to(gpu_device), K)
    assert int(rater.error_flags(gpu_device).sum()) == 0
    np.testing.assert_array_equal(rd.status.cpu().numpy(), rh.status.numpy())
    assert_close_to_fp64(rd, dev, rh, host)
