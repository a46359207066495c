"""The planner matrix on the GPU (tests/planned_matrix.py): every case through
msha_digest_batch_device_planned with the look-back checked (MSHA_CHECK_LOOKBACK=1), into
a prefilled, guard-banded digest buffer; after each call the digests (hashlib, each
distinct (off, len) once), then the plan read back with msha_planned_read_plan and held
against the model (check_plan), then msha_device_status. The direct planner's cases
(k_plan_*, msha_digest_batch on a pinned arena) have no read-back: digests and stats."""
import numpy as np
import pytest

import planned_matrix as M
from mirbft_amd import Engine

pytestmark = pytest.mark.gpu

NOMINAL = M.cases()
GUARD_ROWS = 64
KNOBS = ("MSHA_PLAN_HEAD", "MSHA_PLAN_HEAD_PCT", "MSHA_HEAD_CHAIN2", "MSHA_HEAD_CHAIN8", "MSHA_EARLY_HEAD",
         "MSHA_LANE_WS", "MSHA_PLAN_LANE_CYCLES", "MSHA_PLAN_WAVE_CYCLES", "MSHA_POISON_FOLD_TABLE",
         "MSHA_TRACE_PLAN")


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    """The planned call's knobs as a case sets them and no other way; every look-back checked."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MSHA_CHECK_LOOKBACK", "1")


def _u64(a, shifted):
    """a on the GPU, 16-byte aligned or (shifted) one element into its buffer: 8 mod 16."""
    import torch
    t = torch.empty(a.size + 2, dtype=torch.int64, device="cuda:0")
    v = t[1:1 + a.size] if shifted else t[:a.size]
    v.copy_(torch.from_numpy(a.view(np.int64)))
    assert v.data_ptr() % 16 == (8 if shifted else 0) and v.is_contiguous()
    return v


class Call:
    """One planned call of a batch: its tensors (kept alive), the guard-banded output."""

    def __init__(self, eng, b, fold, unaligned=(False, False), stream=None):
        import torch
        self.b, self.fold = b, fold
        self.arena = torch.from_numpy(b.arena()).to("cuda:0")
        self.off, self.len = _u64(b.off, unaligned[0]), _u64(b.len, unaligned[1])
        self.full = torch.full(((b.n + 2 * GUARD_ROWS) * 32,), M.PREFILL, dtype=torch.uint8, device="cuda:0")
        self.out = self.full[GUARD_ROWS * 32:(GUARD_ROWS + b.n) * 32].view(b.n, 32)
        eng.digest_batch_device_planned(self.arena, self.off, self.len, self.out, stream=stream, fold=fold)

    def digests_ok(self):
        full = self.full.cpu().numpy().reshape(-1, 32)
        assert (full[:GUARD_ROWS] == M.PREFILL).all() and (full[-GUARD_ROWS:] == M.PREFILL).all(), \
            "a row beside the digests was written"
        got, want = full[GUARD_ROWS:-GUARD_ROWS], M.digests(self.b.arena(), self.b.off, self.b.len)
        wrong = np.flatnonzero((got != want).any(axis=1))
        assert wrong.size == 0, "%d digests differ, first at message %d (%s)" % (
            wrong.size, wrong[0], "unwritten" if (got[wrong[0]] == M.PREFILL).all() else "wrong")


@pytest.fixture(scope="module")
def actual(engine):
    """The cases for THIS device: its CU count, and long_cap as a read-back gives it."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    import os
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    try:
        p = M.probe_case(cus)
        Call(engine, p.make(), p.fold)
        plan, _, _ = engine.planned_read_plan()
        engine.device_status()
    finally:
        os.environ.update(saved)
    assert plan["n"] == cus * M.kCoopMsgsPerWg + 1 and plan["long_cap"] > 1, plan
    cs = M.cases(cus, plan["long_cap"])
    assert len(cs) == len(NOMINAL)
    return cs


def _run(engine, monkeypatch, case, b, unaligned):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    engine.set_kernel_policy(case.policy)
    try:
        call = Call(engine, b, case.fold, unaligned)
        plan, order, longs = engine.planned_read_plan()     # (the host's wait for the call)
        call.digests_ok()
        bad = M.check_plan(b.off, b.len, case.fold, plan, order, longs, case.expect)
        assert not bad, (case.name, bad, plan)
        engine.device_status()
    finally:
        engine.set_kernel_policy("auto")
    return plan, order, longs


def test_read_back_before_any_planned_call():
    with Engine(1) as e:
        plan, order, longs = e.planned_read_plan()
        assert plan["n"] == 0 and not any(plan.values()) and order.size == 0 and longs.size == 0


@pytest.mark.parametrize("idx", range(len(NOMINAL)), ids=[c.name for c in NOMINAL])
def test_case(engine, monkeypatch, actual, idx):
    case = actual[idx]
    b = case.make()
    plan, order, _ = _run(engine, monkeypatch, case, b, case.unaligned)
    if any(case.unaligned):
        # the aligned run: the same counters and, position by position, the same classes
        # (which claimant of a key is the lane may differ)
        plan0, order0, _ = _run(engine, monkeypatch, case, b, (False, False))
        assert plan == plan0
        lanes = plan["lanes"]
        assert np.array_equal(M.klass(b.len[order[:lanes].astype(np.int64)]),
                              M.klass(b.len[order0[:lanes].astype(np.int64)]))


def test_sequence_on_one_context():
    """M.sequence(): a larger folded call, a small one under the same keys (a new epoch:
    the larger call's slots read as empty; the order's words past n are stale), an unfolded
    one and, with no host wait after it, a folded one on another stream."""
    import torch
    streams = {0: None, 1: torch.cuda.Stream(), 2: torch.cuda.Stream()}
    with Engine(1) as e:
        pending = []
        for step in M.sequence():
            b = step.make()
            call = Call(e, b, step.fold, stream=streams[step.stream])
            pending.append(call)
            if not step.wait:
                continue
            plan, order, longs = e.planned_read_plan()        # (waits for the device)
            for c in pending:
                c.digests_ok()
            pending = []
            bad = M.check_plan(b.off, b.len, step.fold, plan, order, longs)
            assert not bad, (b.n, bad, plan)
            e.device_status()
        assert not pending and e.stats()["planned_device_calls"] == 4


@pytest.mark.parametrize("name,make,shards", M.direct_cases(), ids=[c[0] for c in M.direct_cases()])
def test_direct_planner(monkeypatch, name, make, shards):
    """The direct planner (plan.hip k_plan_*): digests and stats only, there is no read-back."""
    for k, v in M.DIRECT_ENV.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MSHA_VIRTUAL_SHARDS", str(shards))
    b = make()
    host = b.arena()
    want = M.digests(host, b.off, b.len)
    with Engine(1) as e:
        arena = e.pinned_empty(host.size)
        arena[:] = host
        out = np.full((b.n, 32), M.PREFILL, np.uint8)
        st0 = e.stats()
        got = e.digest_batch(arena, b.off, b.len, out=out)
        st = e.stats()
        sh = e.shard_stats()
        wrong = np.flatnonzero((got != want).any(axis=1))
        assert wrong.size == 0, "%d digests differ, first at message %d" % (wrong.size, wrong[0])
        assert st["direct_calls"] == st0["direct_calls"] + 1 and st["small_calls"] == st0["small_calls"]
        assert len(sh) == shards and sum(s["messages"] for s in sh) == b.n
        distinct = np.unique(M.keys(b.off, b.len)).size
        lanes = sum(s["lanes"] for s in sh)
        assert distinct <= lanes <= b.n and (shards > 1 or lanes == distinct), (lanes, distinct, b.n)
