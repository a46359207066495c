"""The planner matrix on the GPU (tests/parts_plan_matrix.py; mirbft_amd/csrc/parts_plan.hip):
every populated wave of k_parts_scan, the big classes of the device's class_key, every
path of hist_add, the grid edges of init, mark, measure, scatter and fill, a sequence of
calls of different shapes on one context, and the wave length sum at forced
thresholds. Every call is checked three ways: the digests equal hashlib's
(expected_digests), the lane order read back from the device is the plan the header
promises (check_plan against plan_model: a permutation of the named lists, classes
never increasing, the lane count), and the device error word is clean.
tests/test_parts_plan_matrix_cpu.py proves what the builders reach and that
check_plan rejects each kind of wrong plan."""
import numpy as np
import pytest

import parts_plan_matrix as PM

gpu = pytest.mark.gpu


def _dev(a: np.ndarray):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.size == 0:
        return torch.empty(0, dtype=torch.from_numpy(a).dtype, device="cuda:0")
    return torch.from_numpy(a).to("cuda:0")


def _bad_rows(got, want):
    return [int(i) for i in np.nonzero((got != want).any(axis=1))[0]]


def _check_call(engine, case, action_list=None, timed=None, want=None):
    """One call on uploaded copies of the case's arrays, checked in full -> (out rows,
    the model, the order). `timed`: a monkeypatch; the call then runs under
    MSHA_PARTS_TIMING=1 and last_lanes and last_blocks must be the model's."""
    import torch
    al = case.action_list if action_list is None else action_list
    n = case.begin.size - 1 if al is None else al.size
    model = PM.plan_model(case.part_len, case.begin, al)
    if want is None:
        want = PM.expected_digests(case.lists, al)
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    if timed is not None:
        timed.setenv("MSHA_PARTS_TIMING", "1")
    try:
        engine.hash_actions_device_planned(_dev(case.arena), _dev(case.part_off), _dev(case.part_len),
                                           _dev(case.begin), out, action_list=None if al is None else _dev(al))
        stats = engine.parts_plan_stats()
    finally:
        if timed is not None:
            timed.delenv("MSHA_PARTS_TIMING")
    engine.device_status()
    got = out.cpu().numpy()
    bad = _bad_rows(got, want)
    assert bad == [], (len(bad), bad[:8])
    order = engine.parts_plan_order()
    PM.check_plan(order, model, lanes=stats["last_lanes"] if timed is not None else None)
    if timed is not None:
        assert stats["last_blocks"] == model.block_sum
    engine.device_status()
    return got, model, order


@gpu
def test_scan_waves_and_big_classes(engine, monkeypatch):
    """A list at both end keys of every populated scan wave (the cross-wave base over
    13 waves), at every key position of a scan thread, and 4095 .. 16384 blocks: the
    device's class_key puts 2^14 before 2^13 before 2^12 before 4095, with all of
    2^k .. 2^(k+1) - 1 one class. Direct, then through an action list that names the
    lists last to first, the 8,192-block one 50 times and five one-block lists never."""
    case = PM.scan_waves_batch()
    per_list = PM.expected_digests(case.lists)
    for al in (None, PM.reversed_action_list(case)):
        want = per_list if al is None else per_list[al.astype(np.int64)]
        _, model, order = _check_call(engine, case, action_list=al, timed=monkeypatch, want=want)
        along = [model.blocks[int(l)] for l in order]
        assert along[0] == 16384
        assert set(along[1:3]) == {8192, 16383}
        assert set(along[3:6]) == {4096, 4097, 8191}
        assert along[6] == 4095
        assert along[7:] == sorted(along[7:], reverse=True)        # exact classes from there on
        assert len(order) == len(case.lists) - (5 if al is not None else 0)


@gpu
def test_histogram_patterns(engine, monkeypatch):
    """hist_add's cases, a wave each (measure's keys, scatter's positions): one key
    in all 64 lanes, a leader that is not lane 0, only lane 63, an empty wave between
    named ones, one odd lane among 63 at 0, 31 and 63, 64 distinct keys, a bucket three
    workgroups share with 64, 1 and 37 lanes, and a wave the grid cuts."""
    case, patterns = PM.hist_batch()
    assert set(patterns) == PM.HIST_PATTERNS
    _, model, order = _check_call(engine, case, timed=monkeypatch)
    assert len(order) == model.lanes == len(set(case.action_list.tolist()))


@gpu
@pytest.mark.parametrize("n_lists", PM.LIST_EDGES)
def test_list_count_edges(engine, n_lists):
    """n_lists at the wave and workgroup edges of measure and scatter, and on both
    sides of 16 + kKeys, where k_parts_init's grid goes from the counters to the lists."""
    case = PM.tiny_batch(n_lists)
    _, model, order = _check_call(engine, case)
    assert len(order) == n_lists


@gpu
@pytest.mark.parametrize("n_lists,n_actions", PM.ACTION_EDGES, ids=["%d-%d" % p for p in PM.ACTION_EDGES])
def test_action_count_edges(engine, n_lists, n_actions):
    """n_actions at the workgroup edges of mark and fill and at 70,001; every list
    named at least once where n_actions allows."""
    case = PM.tiny_batch(n_lists, n_actions)
    got, model, order = _check_call(engine, case)
    assert len(order) == min(n_lists, n_actions)
    if n_actions == 70001:
        al = case.action_list.astype(np.int64)
        ids, at = np.unique(al, return_index=True)              # the first action naming each list
        assert ids.tolist() == list(range(n_lists))
        first = at.astype(np.int64)
        same = (got == got[first[al]]).all(axis=1)
        assert same.all(), np.nonzero(~same)[0][:8].tolist()


@gpu
def test_a_sequence_of_calls_on_one_context(engine, monkeypatch):
    """Calls of different sizes and shapes on the session's context, the plan of each
    checked in full: nothing of a call (used flags, counters, keys, the order, the
    digest table) may reach the next. (a) 4,501 lists direct; (b) 70 lists, 100,000
    actions; (c) (a)'s arrays, ten lists named -- the workspace grows here, for the
    table; (d) ten others: ten lanes, not twenty; (e) 300 lists direct; (f) (a) again."""
    a = PM.mixed_batch(4501, seed=0x5E01)
    b = PM.mixed_batch(70, seed=0x5E02, n_actions=100000)
    e = PM.mixed_batch(300, seed=0x5E03, max_blocks=40)
    rng = np.random.default_rng(0x5E04)
    pick = rng.permutation(4501)[:20].astype(np.uint32)
    s1, s2 = pick[:10], pick[10:]
    assert not set(s1.tolist()) & set(s2.tolist())
    want_a = PM.expected_digests(a.lists)
    _check_call(engine, a, timed=monkeypatch, want=want_a)
    _check_call(engine, b, timed=monkeypatch)
    _, m, order = _check_call(engine, a, action_list=np.concatenate([s1, s1[:3]]), timed=monkeypatch)
    assert sorted(order.tolist()) == sorted(s1.tolist())
    _, m, order = _check_call(engine, a, action_list=s2, timed=monkeypatch)
    assert m.lanes == 10 and sorted(order.tolist()) == sorted(s2.tolist())
    _check_call(engine, e, timed=monkeypatch)
    _check_call(engine, a, timed=monkeypatch, want=want_a)


@gpu
@pytest.mark.parametrize("threshold", PM.WAVE_SUM_THRESHOLDS)
def test_forced_wave_sum_threshold(engine, actions_golden, monkeypatch, threshold):
    """MSHA_PARTS_PLAN_WAVE_SUM forced: at 1 every non-empty list of a wave is summed
    by the wave, one after the other; at 64 the part counts lie on both sides of it
    and of one and two strides; at 100,000 the 1,505-part EpochChange is summed by its
    own lane. last_blocks is the sum's readout, and a wrong sum is a class out of order."""
    ec = next(parts for name, kind, parts, _ in actions_golden if kind == "epoch_change" and len(parts) > 1000)
    assert len(ec) == 1505
    case = PM.wave_sum_batch(ec)
    monkeypatch.setenv("MSHA_PARTS_PLAN_WAVE_SUM", str(threshold))
    _, model, order = _check_call(engine, case, timed=monkeypatch)
    assert model.blocks[PM.EPOCH_CHANGE_AT] == max(model.blocks) and int(order[0]) == PM.EPOCH_CHANGE_AT
    assert model.blocks[PM.LAST_PART_AT[0]] == 2 and model.blocks[PM.LAST_PART_AT[1]] == 3
