"""The posterior merge (K9: csrc/sweep.hip, csrc/sweep_core.h) against an independent
fp64 oracle: per-rank messages, the decode with both clamp floors and non-finite sums, the
scaled-prefix -> delta table, the causal record correction for K = 1..5 and the owner
block reduce of the split collective.

Cases, oracle, budgets and the fp32 transcription: merge_cases.py; derivation and measured
worst ratios: docs/ARCHITECTURE.md "Merge error budget".  The CPU tests hold the host
mirror and the transcription to the budgets; the ``gpu`` tests hold the device to the same
ones and pin the compressed kernels bit for bit to the fp32 path + torch's conversion."""
import numpy as np
import pytest
import torch

from analyzer_amd.ops.native import native
from analyzer_amd.parallel.comm import block_reduce_rows
from analyzer_amd.parallel.sweep import MergeClampError, SweepMerger

import merge_cases as C

US = C.UNKNOWN_SIGMA
MODES = ("raw", "scaled", "fp16", "bf16")


def _vst(dev):
    return torch.tensor(C.VST, dtype=torch.float32, device=dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _tile(arr):
    """Oracle rows of the grid -> rows of the tiled grid."""
    return np.concatenate([arr, arr[C.tiled_grid()[1]]])


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------ runners (host mirror or device)
def run_messages(dev, tab, scaled, prior="own", packed=None, strided=False):
    """fp32 messages [P, 16] of a table; ``prior``: "own" (the table's), "alias" (the start
    tensor itself) or "clone" (a copy of the start).  ``packed`` = wire name: the
    compressed operands (msg bits [P, 14] int16, cnt [P, 1]) instead, written into strided
    views of [P, 8]-word operand rows (as SweepMerger.op_views) if ``strided``."""
    s0 = C.base_tensor(tab.start).to(dev)
    a = {"own": lambda: C.base_tensor(tab.prior).to(dev), "alias": lambda: s0, "clone": lambda: s0.clone()}[prior]()
    ro = C.make_roster(tab.after, tab.attrs).to(dev)
    P = tab.P
    if packed is None:
        guard = torch.full((P + 1, 16), -77.0, device=dev)
        native().sweep_delta(s0, a, ro.state, ro.attrs, _vst(dev), US, scaled, guard[:P])
        _sync(dev)
        assert bool((guard[P] == -77.0).all())
        return guard[:P].cpu()
    dt = C.WIRE[packed]
    if strided:
        op = torch.zeros((P, 16), dtype=dt, device=dev)
        msg, cnt = op[:, :14], op.view(torch.int32)[:, 7:8]
    else:
        msg, cnt = torch.zeros((P, 14), dtype=dt, device=dev), torch.zeros((P, 1), dtype=torch.int32, device=dev)
    native().sweep_delta_packed(s0, a, ro.state, ro.attrs, _vst(dev), US, msg, cnt)
    _sync(dev)
    return msg.cpu().contiguous().view(torch.int16), cnt.cpu().contiguous()


def run_decode(dev, T, mode, msg=None, strided=False, prefix=None):
    """Decode table T in ``mode``; -> (rows [P, 32], base rows [P, 16], clamp count[, delta])."""
    P = T.P
    s0 = C.base_tensor(T.start).to(dev)
    ro = C.make_roster(T.start, T.attrs).to(dev)
    s, s2 = ro.state.clone(), torch.full((P, 16), -5.0, device=dev)
    clamps = torch.zeros(1, dtype=torch.int32, device=dev)
    if mode in ("raw", "scaled"):
        buf = T.buf(mode == "scaled") if msg is None else msg
        native().sweep_apply(s0, buf.to(dev), ro.attrs, s, s2, _vst(dev), US, mode == "scaled", clamps)
        _sync(dev)
        return s.cpu(), s2.cpu(), int(clamps.item())
    dt = C.WIRE[mode]
    half = torch.from_numpy(T.scaled.reshape(P, 14)).to(dt) if msg is None else msg
    if strided:
        op = torch.zeros((P, 16), dtype=dt, device=dev)
        m, c = op[:, :14], op.view(torch.int32)[:, 7:8]
        m.copy_(half)
        c.copy_(T.cnt())
    else:
        m, c = half.to(dev).contiguous(), T.cnt().to(dev)
    delta = torch.full((P, 16), -9.0, device=dev) if prefix is not None else None
    native().sweep_apply_packed(s0, m, c, ro.attrs, s, s2, _vst(dev), US, clamps,
                                None if prefix is None else prefix.to(dev), delta)
    _sync(dev)
    out = (s.cpu(), s2.cpu(), int(clamps.item()))
    return out + (delta.cpu(),) if prefix is not None else out


def decode_inputs(T, mode):
    """The message values [P, 7, 2] the decode of ``mode`` receives (wire modes: rounded)."""
    if mode in ("raw", "scaled"):
        return T.scaled if mode == "scaled" else T.raw
    half = torch.from_numpy(T.scaled.reshape(T.P, 14)).to(C.WIRE[mode])
    return half.float().numpy().reshape(T.P, 7, 2)


# ------------------------------------------------------------------ checks shared by CPU and GPU
def check_messages(dev, scaled):
    tab, _ = C.tiled_grid()
    buf = run_messages(dev, tab, scaled).numpy().astype(np.float64)
    msg, bud, touch = (_tile(x) for x in C.grid_messages(scaled))
    what = "%s %s messages" % (dev, "scaled" if scaled else "raw")
    w = {k: C.assert_budget(buf[:, i:14:2], msg[:, :, i], bud[:, :, i], "%s %s" % (what, k), tab.labels)
         for i, k in enumerate(("d_pi", "d_tau"))}
    assert np.array_equal(buf[:, 14:].astype(np.int64), touch), "touch fields"
    n = C.grid_table().P
    assert np.array_equal(buf[:n][C.tiled_grid()[1]], buf[n:]), "the two copies of the grid differ"
    for P in C.SIZES:  # whole groups past P leave together; nothing past P is written
        part = run_messages(dev, tab.take(np.arange(n, n + P)), scaled).numpy()
        assert np.array_equal(part.view(np.int32), buf[n:n + P].astype(np.float32).view(np.int32)), P
    return w


def check_decode(dev, mode):
    T = C.decode_table()
    vals = decode_inputs(T, mode)
    orc = C.decode_oracle(T, vals, mode != "raw")
    s, s2, clamps = run_decode(dev, T, mode)
    rows = s.view(T.P, 8, 4).numpy()
    what = "%s %s decode" % (dev, mode)
    w = {k: C.assert_budget(rows[:, :7, 2 * i], orc["out"][:, :7, i], orc["B"][:, :, i], "%s %s" % (what, k), T.labels)
         for i, k in enumerate(("mu", "sigma"))}
    assert (rows[:, :, 1] == 0).all() and (rows[:, :, 3] == 0).all(), "tags"
    assert torch.equal(_bits(s.view(T.P, 8, 4)[:, :, 0::2].reshape(T.P, 16)), _bits(s2)), "base rows != decoded rows"
    assert torch.equal(_bits(s2[:, 14:]), _bits(C.base_tensor(T.start)[:, 14:])), "granule 7"
    assert clamps == orc["clamps"] > 0, (clamps, orc["clamps"])
    seen = {b for row in orc["branch"] for b in row}
    assert {"idle", "nat", "var", "clamp", "nonfinite"} <= seen, seen
    # what a non-finite sum writes: the window-start value, bit for bit
    nf = np.array([[b == "nonfinite" for b in row] for row in orc["branch"]])
    assert torch.equal(_bits(s2).view(T.P, 8, 2)[:, :7][torch.from_numpy(nf)],
                       _bits(C.base_tensor(T.start)).view(T.P, 8, 2)[:, :7][torch.from_numpy(nf)])
    for P in C.SIZES:
        idx = np.arange(T.P - P, T.P) if P < 40 else np.arange(100, 100 + P)
        part = _SubTable(T, idx)
        ps, ps2, _ = run_decode(dev, part, mode)
        assert torch.equal(_bits(ps), _bits(s[idx])) and torch.equal(_bits(ps2), _bits(s2[idx])), P
    return w


class _SubTable:
    """Rows ``idx`` of a DecodeTable."""

    def __init__(self, T, idx):
        self.P, self.start, self.attrs = len(idx), T.start[idx], T.attrs[idx]
        self.scaled, self.raw, self.m = T.scaled[idx], T.raw[idx], T.m[idx]

    touch, buf, cnt = C.DecodeTable.touch, C.DecodeTable.buf, C.DecodeTable.cnt


def check_prefix_delta(dev, wire):
    tab, _ = C.tiled_grid()
    dt = C.WIRE[wire]
    msg = _tile(C.grid_messages(True)[0]).astype(np.float32).reshape(tab.P, 14)
    with np.errstate(all="ignore"):
        prefix = torch.from_numpy(msg).to(dt)
    vals = prefix.float().numpy().reshape(tab.P, 7, 2)
    exp, bud = np.zeros((tab.P, 8, 2)), np.zeros((tab.P, 8, 2))
    for p in range(tab.P):
        sd, c0 = C.seed_of(tab.attrs[p]), C.tr(tab.start[p], 0)
        for t in range(C.TRACKS):
            r = C.oracle_prefix_delta(t, C.tr(tab.start[p], t), c0, sd, float(vals[p, t, 0]), float(vals[p, t, 1]))
            exp[p, t], bud[p, t] = r[:2], r[2:]
    s0 = C.base_tensor(tab.start).to(dev)
    delta = torch.full((tab.P, 16), -9.0, device=dev)
    native().prefix_delta(s0, prefix.to(dev), torch.from_numpy(tab.attrs).to(dev), _vst(dev), US, delta)
    _sync(dev)
    got = delta.cpu().numpy().reshape(tab.P, 8, 2)
    what = "%s %s delta table" % (dev, wire)
    return {k: C.assert_budget(got[:, :, i], exp[:, :, i], bud[:, :, i], "%s %s" % (what, k), tab.labels)
            for i, k in enumerate(("d_pi", "d_tau"))}, delta.cpu(), prefix


def check_records(dev, K):
    rec, rows, delta = C.record_case(K)
    worst = 0.0
    for M in C.record_sizes(K):
        got = torch.from_numpy(rows[:M].copy()).to(dev)
        native().correct_records(torch.from_numpy(rec[:M].copy()).to(dev), K, got, torch.from_numpy(delta).to(dev))
        _sync(dev)
        worst = max(worst, C.check_records(got.cpu().numpy(), K, M, "%s K=%d M=%d records" % (dev, K, M)))
    return worst


def check_round_trip(dev, scaled):
    """One rank's message, decoded against the start, gives that rank's posterior: the
    decode budget with the message's own budget as the error its input carries."""
    gtab = C.grid_table()
    first = C.Table(gtab.start, gtab.start, gtab.after, gtab.attrs, gtab.labels)
    buf = run_messages(dev, first, scaled, prior="alias")
    T = _GridDecode(gtab)
    s, _, _ = run_decode(dev, T, "scaled" if scaled else "raw", msg=buf)
    msg, bud, touch = C.grid_messages(scaled, "first")
    return _check_against_after(gtab, s, msg, bud, touch, scaled, "%s %s round trip" % (dev, "scaled" if scaled else "raw"))


class _GridDecode:
    """The grid's start as a decode table (the messages are given; no touch counts on the wire)."""

    def __init__(self, gtab):
        self.P, self.start, self.attrs = gtab.P, gtab.start, gtab.attrs

    def cnt(self):
        return torch.zeros((self.P, 1), dtype=torch.int32)


def _check_against_after(gtab, s, msg, bud, touch, scaled, what):
    rows = s.view(gtab.P, 8, 4).numpy()
    exp, B = np.array(gtab.start, dtype=np.float64), np.zeros((gtab.P, 8, 2))
    held = 0
    skip = np.zeros((gtab.P, 8), dtype=bool)
    for p in range(gtab.P):
        sd, c0 = C.seed_of(gtab.attrs[p]), C.tr(gtab.start[p], 0)
        for t in range(C.TRACKS):
            m = int((touch[p, 0] >> (4 * t)) & 15 if t < 4 else (touch[p, 1] >> (4 * (t - 4))) & 15)
            r = C.oracle_decode(t, C.tr(gtab.start[p], t), c0, sd, msg[p, t, 0], msg[p, t, 1], m, scaled,
                                e_dp=bud[p, t, 0], e_dt=bud[p, t, 1])
            if r["branch"] == "nat" and r["rho"] < 0.125:
                exp[p, t], B[p, t] = gtab.after[p, t], (r["B_mu"], r["B_sg"])
                held += 1
            elif r["branch"] not in ("idle", "nobase"):
                skip[p, t] = True   # the oracle's call: the message's own error decides the side of a floor
    assert held > 300, held
    got = np.where(skip[:, :, None], exp, rows[:, :, 0::2])
    return {k: C.assert_budget(got[:, :7, i], exp[:, :7, i], B[:, :7, i], "%s %s" % (what, k), gtab.labels)
            for i, k in enumerate(("mu", "sigma"))}


def check_telescope(dev, scaled):
    """start + the message of the earlier rank (start -> prior) + this rank's message
    measured from that prior, decoded with the touch fields held at <= 1 (as the causal
    re-sweeps do), is this rank's posterior."""
    gtab = C.grid_table()
    earlier = C.Table(gtab.start, gtab.start, gtab.prior, gtab.attrs, gtab.labels)
    b0 = run_messages(dev, earlier, scaled, prior="clone")
    b1 = run_messages(dev, gtab, scaled)
    tot = b0 + b1
    x = tot[:, 14:].to(torch.int32)
    tot[:, 14:] = ((x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111).float()
    s, _, _ = run_decode(dev, _GridDecode(gtab), "scaled" if scaled else "raw", msg=tot)
    m0, e0, t0 = C.grid_messages(scaled, "prior")
    m1, e1, t1 = C.grid_messages(scaled, "after")
    touch = t0 | t1
    msg = m0 + m1
    bud = e0 + e1 + C.U * np.abs(msg) * (1 + C.U) + C.U * (e0 + e1)
    return _check_against_after(gtab, s, msg, bud, touch, scaled, "%s %s telescope" % (dev, "scaled" if scaled else "raw"))


def check_zero_message(dev, mode):
    gtab = C.grid_table()
    T = _GridDecode(gtab)
    z = torch.zeros((T.P, 16)) if mode in ("raw", "scaled") else torch.zeros((T.P, 14), dtype=C.WIRE[mode])
    s, s2, clamps = run_decode(dev, T, mode, msg=z)
    assert torch.equal(_bits(s), _bits(C.make_roster(gtab.start, gtab.attrs).state)), mode
    assert torch.equal(_bits(s2), _bits(C.base_tensor(gtab.start))) and clamps == 0, mode


def check_nonfinite_raises(dev, wire):
    """Every non-finite half on the wire is counted, SweepMerger.check raises, and the
    track is left at its start; so does the fp16 message of a seeded sigma-2000 track that
    fell to sigma 100 with a 300-point shift, built from roster values alone."""
    T = C.decode_table()
    idx = np.array([i for i, l in enumerate(T.labels) if l["kind"] == "nonfinite"])
    sub = _SubTable(T, idx)
    ro = C.make_roster(sub.start, sub.attrs).to(dev)
    m = SweepMerger(sub.P, dev, comm_dtype=wire, force=True)
    m.begin(ro)
    with np.errstate(all="ignore"):
        m.msg.copy_(torch.from_numpy(sub.scaled.reshape(sub.P, 14)).to(C.WIRE[wire]))
    m.cnt.copy_(sub.cnt())
    before = ro.state.clone()
    m.decode_packed(ro, into=m.start)
    assert m.clamp_hits() == sub.P == 36
    assert torch.equal(_bits(ro.state), _bits(before))
    with pytest.raises(MergeClampError):
        m.check()
    if wire != "fp16":
        return
    start, after = C._null_rows(3), C._null_rows(3)
    start[:, 0], after[:, 0] = (1500.0, 2000.0), (1800.0, 100.0)
    attrs = np.zeros((3, 4), dtype=np.float32)
    ro = C.make_roster(start, attrs).to(dev)
    m = SweepMerger(3, dev, comm_dtype="fp16", force=True)
    m.begin(ro)
    ro.state.copy_(C.make_roster(after, attrs).state)
    dp, dt, _, _, _ = C.oracle_message(0, (1500.0, 2000.0), (1500.0, 2000.0), (1500.0, 2000.0), (1800.0, 100.0), None, True)
    assert (dp, dt) == (399.0, 120000.0) and C.round_wire([dt], "fp16")[0] == 0x7C00
    m.messages_packed(ro)
    assert m.msg.cpu().view(torch.int16)[:, :2].tolist() == [[int(C.round_wire([399.0], "fp16")[0]), 0x7C00]] * 3
    m.decode_packed(ro, into=m.start)
    assert m.clamp_hits() == 3
    with pytest.raises(MergeClampError):
        m.check()


# ------------------------------------------------------------------ CPU: the oracle itself
def test_oracle_equal_losses_add_in_variance():
    """Equal losses are exact in variance space: sigma'^2 = sigma_B^2 + m Delta with
    Delta = sigma_B^2 (1 / x - 1) the variance one rank's loss adds."""
    T = C.decode_table()
    orc = C.decode_oracle(T, T.scaled, True)
    n = 0
    for p, l in enumerate(T.labels):
        if l["kind"] == "equal" and l["m"] >= 2:
            t, m = l["t"], l["m"]
            B = C.base_of(t, C.tr(T.start[p], t), C.tr(T.start[p], 0), C.seed_of(T.attrs[p]))
            x = 1.0 + float(T.scaled[p, t, 0]) / m
            assert orc["branch"][p][t] == "var"
            assert orc["out"][p, t, 1] ** 2 == pytest.approx(B[1] ** 2 * (1 + m * (1 / x - 1)), rel=1e-13)
            assert abs(x - 0.8) < 1e-6
            n += 1
    assert n == 7 * 3 * 5


def test_oracle_fp64_is_enough_where_messages_cancel():
    """The messages are the formulas that cancel hardest (x1 (mu1 - mu_B) - x0 (mu0 - mu_B)
    of two nearby values).  A 50-digit evaluation from the same fp32 inputs differs from the
    fp64 oracle by less than 2^-20 of the budget everywhere on the grid."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    gtab = C.grid_table()
    worst = 0.0
    for scaled in (False, True):
        msg, bud, _ = C.grid_messages(scaled)
        for p in range(gtab.P):
            sd, c0 = C.seed_of(gtab.attrs[p]), C.tr(gtab.start[p], 0)
            for t in range(C.TRACKS):
                if not bud[p, t, 0]:
                    continue
                c, a, b = (C.tr(x[p], t) for x in (gtab.start, gtab.prior, gtab.after))
                Bm, Bs = (mp.mpf(v) for v in C.base_of(t, c, c0, sd))
                a = (Bm, Bs) if a is None else (mp.mpf(a[0]), mp.mpf(a[1]))
                b = (mp.mpf(b[0]), mp.mpf(b[1]))
                if scaled:
                    x1, x0 = (Bs / b[1]) ** 2, (Bs / a[1]) ** 2
                    dp, dt = x1 - x0, x1 * (b[0] - Bm) - x0 * (a[0] - Bm)
                else:
                    dp, dt = 1 / b[1] ** 2 - 1 / a[1] ** 2, b[0] / b[1] ** 2 - a[0] / a[1] ** 2
                for got, exact, bd in ((msg[p, t, 0], dp, bud[p, t, 0]), (msg[p, t, 1], dt, bud[p, t, 1])):
                    worst = max(worst, float(abs(mp.mpf(float(got)) - exact) / mp.mpf(float(bd))))
    assert worst < 2.0 ** -20, worst


def test_oracle_raw_and_scaled_decodes_agree():
    """The raw and the scaled encoding of one message decode to the same posterior (the
    raw table is the scaled one times pi_B, rounded to fp32: 4 U of its operands)."""
    T = C.decode_table()
    sc, rw = C.decode_oracle(T, T.scaled, True), C.decode_oracle(T, T.raw, False)
    n = 0
    for p, l in enumerate(T.labels):
        if l["kind"] in ("equal", "unequal", "gain"):
            t = l["t"]
            assert sc["branch"][p][t] == rw["branch"][p][t] in ("nat", "var")
            np.testing.assert_allclose(rw["out"][p, t], sc["out"][p, t], rtol=2e-5, atol=2e-3)
            n += 1
    assert n == 7 * 4 * 3 * 5


# ------------------------------------------------------------------ CPU: host mirror
@pytest.mark.parametrize("scaled", [False, True])
def test_host_messages_within_budget(scaled):
    check_messages("cpu", scaled)


@pytest.mark.parametrize("mode", MODES)
def test_host_decode_within_budget(mode):
    check_decode("cpu", mode)


@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_host_prefix_delta_within_budget(wire):
    check_prefix_delta("cpu", wire)


def test_prefix_delta_rejects_a_short_seed_table():
    """The kernel indexes vst by tier + 1 (31 tiers): a shorter table must not reach it."""
    P = 2
    s0, attrs, delta = torch.zeros(P, 16), torch.zeros(P, 4), torch.empty(P, 16)
    prefix = torch.zeros(P, 14, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="vst must have 31 entries"):
        native().prefix_delta(s0, prefix, attrs, _vst("cpu")[:30].contiguous(), US, delta)
    native().prefix_delta(s0, prefix, attrs, _vst("cpu"), US, delta)  # the whole table passes


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_host_record_correction_within_budget(K):
    check_records("cpu", K)


@pytest.mark.parametrize("scaled", [False, True])
def test_host_round_trip_and_telescope(scaled):
    check_round_trip("cpu", scaled)
    check_telescope("cpu", scaled)


@pytest.mark.parametrize("mode", MODES)
def test_host_zero_message_keeps_the_row(mode):
    check_zero_message("cpu", mode)


@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_host_nonfinite_sum_raises(wire):
    check_nonfinite_raises("cpu", wire)


def test_host_clone_of_start_gives_the_aliased_messages():
    gtab = C.grid_table()
    first = C.Table(gtab.start, gtab.start, gtab.after, gtab.attrs, gtab.labels)
    for scaled in (False, True):
        assert torch.equal(_bits(run_messages("cpu", first, scaled, "alias")), _bits(run_messages("cpu", first, scaled, "clone")))


@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_host_packed_operands_strided_and_contiguous(wire):
    """The host path of the compressed operands: the fp32 mirror + torch's conversion, the
    same bits through strided views of [P, 8]-word operand rows."""
    tab, _ = C.tiled_grid()
    touch = _tile(C.grid_messages(True)[2])
    want = run_messages("cpu", tab, True)[:, :14].to(C.WIRE[wire]).contiguous().view(torch.int16)
    for strided in (False, True):
        msg, cnt = run_messages("cpu", tab, True, packed=wire, strided=strided)
        assert torch.equal(msg, want), strided
        assert np.array_equal(cnt.numpy()[:, 0].astype(np.int64), touch[:, 0] | (touch[:, 1] << 16)), strided
    T = C.decode_table()
    a, b = run_decode("cpu", T, wire), run_decode("cpu", T, wire, strided=True)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])) and a[2] == b[2]


BLOCK_CASES = [(N, blk, w) for N in (1, 2, 15) for blk in (1, 31, 257) for w in ("fp16", "bf16")]


@pytest.mark.parametrize("N,blk,wire", BLOCK_CASES)
def test_host_block_reduce_matches_oracle(N, blk, wire):
    recv = C.block_reduce_case(N, blk, wire)
    tot, pref = C.oracle_block_reduce(recv, N, wire)
    if N >= 2:  # the cases hold ties of both parities: sums that round up and that round down
        acc = sum(C.wire_value(np.ascontiguousarray(recv.reshape(N, blk, 8)[q, :, :7]).view(np.uint16), wire).astype(np.float64)
                  for q in range(N))
        back = C.wire_value(np.ascontiguousarray(tot[:, :7]).view(np.uint16), wire).astype(np.float64)
        assert (back > acc).any() and (back < acc).any()
    assert not pref.reshape(N, blk, 7)[0].any()
    if N == 15:
        assert (tot[:, 7] == 0x0FFFFFFF).all()
    th, ph = block_reduce_rows(torch.from_numpy(recv), N, C.WIRE[wire], True)
    assert np.array_equal(th.numpy(), tot) and np.array_equal(ph.numpy(), pref)
    assert block_reduce_rows(torch.from_numpy(recv), N, C.WIRE[wire], False)[1] is None


# ------------------------------------------------------------------ CPU: the fp32 transcription and its mutations
def transcription_ratios(mut=None):
    """Worst |error| / budget of the numpy-fp32 transcription per output (inf: a value the
    oracle pins exactly -- a NULL, a zero, a touch count -- differs)."""
    out = {}
    gtab = C.grid_table()
    seeds = [C.seed_of(a) for a in gtab.attrs]
    for scaled in (False, True):
        msg, bud, touch = C.grid_messages(scaled)
        got = np.zeros_like(msg)
        for p in range(gtab.P):
            c0 = C.tr(gtab.start[p], 0)
            for t in range(C.TRACKS):
                got[p, t] = C.t_message(t, C.tr(gtab.start[p], t), c0, C.tr(gtab.prior[p], t), C.tr(gtab.after[p], t),
                                        seeds[p], scaled, mut)[:2]
        out["msg %s" % ("scaled" if scaled else "raw")] = float(C.ratios(got, msg, bud).max())
        if scaled:
            exp, pb, gotd = np.zeros_like(msg), np.zeros_like(msg), np.zeros_like(msg)
            vals = msg.astype(np.float32)
            for p in range(gtab.P):
                c0 = C.tr(gtab.start[p], 0)
                for t in range(C.TRACKS):
                    a = (t, C.tr(gtab.start[p], t), c0, seeds[p], float(vals[p, t, 0]), float(vals[p, t, 1]))
                    r = C.oracle_prefix_delta(*a)
                    exp[p, t], pb[p, t] = r[:2], r[2:]
                    gotd[p, t] = C.t_prefix_delta(*a, mut)
            out["delta table"] = float(C.ratios(gotd, exp, pb).max())
    T = C.decode_table()
    lo, hi = T.touch()
    for scaled in (False, True):
        vals = T.scaled if scaled else T.raw
        orc = C.decode_oracle(T, vals, scaled)
        got = np.array(T.start, dtype=np.float64)
        clamps = 0
        for p in range(T.P):
            sd, c0 = C.seed_of(T.attrs[p]), C.tr(T.start[p], 0)
            for t in range(C.TRACKS):
                m = int(C.t_touch_count(int(lo[p]), int(hi[p]), t, mut))
                o, cl = C.t_decode(t, C.tr(T.start[p], t), c0, sd, vals[p, t, 0], vals[p, t, 1], m, scaled, mut)
                clamps += cl
                got[p, t] = (np.nan, np.nan) if o is None else o
        r = C.ratios(got[:, :7], orc["out"][:, :7], orc["B"])
        out["decode %s" % ("scaled" if scaled else "raw")] = float(r.max()) if clamps == orc["clamps"] else np.inf
    K = 3
    rec, rows, delta = C.record_case(K)
    exp, bud = C.record_oracle(K)
    got = rows.astype(np.float64)
    S = 2 * K
    for i in range(rows.shape[0]):
        if rows.view(np.int32)[i, 5 * S + 1] & 0xFF:
            continue
        meta = int(rec[i, S])
        t, n0, n1 = 1 + (meta & 0xFF), (meta >> 8) & 0xFF, (meta >> 16) & 0xFF
        tm = t - 1 if mut == "record_track" else t
        for j in range(S):
            p = int(rec[i, j])
            if ((j < n0) if j < K else (j - K < n1)) and 0 <= p < delta.shape[0]:
                got[i, j], got[i, S + j] = C.t_correct(rows[i, j], rows[i, S + j], delta[p, 0], delta[p, 1])
                got[i, 3 * S + j], got[i, 4 * S + j] = C.t_correct(rows[i, 3 * S + j], rows[i, 4 * S + j],
                                                                   delta[p, 2 * tm], delta[p, 2 * tm + 1])
    out["records"] = float(C.ratios(got, exp, bud).max())
    return out


def test_transcription_within_budget():
    r = transcription_ratios()
    print("fp32 transcription worst |error| / budget:", {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("mut", C.MUTATIONS)
def test_budget_catches_mutation(mut):
    """Each wrong term a test against the shared header cannot see breaks a budget."""
    r = transcription_ratios(mut)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    print("mutation %s fails: %s" % (mut, {k: ("%.3g" % v) for k, v in bad.items()}))
    assert bad, (mut, r)


# ------------------------------------------------------------------ the device
@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True])
def test_device_messages_within_budget(gpu_device, scaled):
    """Measured on MI355X: docs/ARCHITECTURE.md "Merge error budget"."""
    check_messages(gpu_device, scaled)
    gtab = C.grid_table()
    first = C.Table(gtab.start, gtab.start, gtab.after, gtab.attrs, gtab.labels)
    a, b = run_messages(gpu_device, first, scaled, "alias"), run_messages(gpu_device, first, scaled, "clone")
    assert torch.equal(_bits(a), _bits(b)), "a prior that is a copy of the start != the aliased call"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_device_decode_within_budget(gpu_device, mode):
    check_decode(gpu_device, mode)
    check_zero_message(gpu_device, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_device_packed_kernels_pinned_to_fp32_path(gpu_device, wire):
    """The compressed kernels at the new edges == the fp32 kernels + torch's conversion,
    bit for bit, through contiguous operands and through strided views of [P, 8]-word
    operand rows; a prior passed as its own buffer == the aliased call."""
    dev, dt = gpu_device, C.WIRE[wire]
    tab, _ = C.tiled_grid()
    _, _, touch = (_tile(x) for x in C.grid_messages(True))
    buf = run_messages(dev, tab, True)
    want = buf[:, :14].to(dt).contiguous().view(torch.int16)
    for strided in (False, True):
        msg, cnt = run_messages(dev, tab, True, packed=wire, strided=strided)
        assert torch.equal(msg, want), strided
        assert np.array_equal(cnt.numpy()[:, 0].astype(np.int64), touch[:, 0] | (touch[:, 1] << 16)), strided
    gtab = C.grid_table()
    first = C.Table(gtab.start, gtab.start, gtab.after, gtab.attrs, gtab.labels)
    a, b = run_messages(dev, first, True, "alias", packed=wire), run_messages(dev, first, True, "clone", packed=wire)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the decode: wire operands == the fp32 kernel on their values
    T = C.decode_table()
    half = torch.from_numpy(T.scaled.reshape(T.P, 14)).to(dt)
    lo, hi = T.touch()
    joined = torch.cat([half.float(), torch.from_numpy(np.stack([lo, hi], 1).astype(np.float32))], dim=1)
    ref = run_decode(dev, T, "scaled", msg=joined)
    for strided in (False, True):
        got = run_decode(dev, T, wire, strided=strided)
        assert torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(_bits(got[1]), _bits(ref[1])), strided
        assert got[2] == ref[2]


@pytest.mark.gpu
@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_device_prefix_delta_within_budget(gpu_device, wire):
    _, delta, prefix = check_prefix_delta(gpu_device, wire)
    # the decode's fused delta table == the stand-alone kernel
    tab, _ = C.tiled_grid()
    T = _GridDecode(tab)
    fused = run_decode(gpu_device, T, wire, msg=torch.zeros((T.P, 14), dtype=C.WIRE[wire]), prefix=prefix)[3]
    assert torch.equal(_bits(fused), _bits(delta))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_device_record_correction_within_budget(gpu_device, K):
    check_records(gpu_device, K)


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True])
def test_device_round_trip_and_telescope(gpu_device, scaled):
    check_round_trip(gpu_device, scaled)
    check_telescope(gpu_device, scaled)


@pytest.mark.gpu
@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_device_nonfinite_sum_raises_and_matches_host(gpu_device, wire):
    check_nonfinite_raises(gpu_device, wire)
    T = C.decode_table()
    host, dev = run_decode("cpu", T, wire), run_decode(gpu_device, T, wire)
    nf = torch.tensor([l["kind"] == "nonfinite" for l in T.labels])
    assert host[2] == dev[2]
    assert torch.equal(_bits(host[0])[nf], _bits(dev[0])[nf]) and torch.equal(_bits(host[1])[nf], _bits(dev[1])[nf])


@pytest.mark.gpu
@pytest.mark.parametrize("N,blk,wire", BLOCK_CASES)
def test_device_block_reduce_matches_oracle(gpu_device, N, blk, wire):
    recv = C.block_reduce_case(N, blk, wire)
    tot, pref = C.oracle_block_reduce(recv, N, wire)
    rd = torch.from_numpy(recv).to(gpu_device)
    t1 = torch.full((blk + 1, 8), -3, dtype=torch.int32, device=gpu_device)
    p1 = torch.full((N * blk + 1, 7), -3, dtype=torch.int32, device=gpu_device)
    t2 = torch.full((blk, 8), -3, dtype=torch.int32, device=gpu_device)
    native().sweep_block_reduce(rd, N, wire == "bf16", t1[:blk], p1[:N * blk])
    native().sweep_block_reduce(rd, N, wire == "bf16", t2)
    torch.cuda.synchronize()
    assert np.array_equal(t1[:blk].cpu().numpy(), tot) and np.array_equal(t2.cpu().numpy(), tot)
    assert np.array_equal(p1[:N * blk].cpu().numpy(), pref)
    assert bool((t1[blk] == -3).all()) and bool((p1[N * blk] == -3).all())
