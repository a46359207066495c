"""msha_hash_actions_device_routed on the GPU (mirbft_amd/csrc/parts_plan.hip
k_route_measure, parts_route.cpp): the planned parts call with its long lists found on
the GPU, flattened and hashed by the eight-lane chain. Thresholds are forced small
through the options, so every case is a few hundred lists. Every case checks every
digest against hashlib, the device status, the route itself (tests/parts_route_matrix.py
check_route on the routed ids and the lane order) and the launch counters of both stat
structs."""
import os

import numpy as np
import pytest

import parts_route_matrix as M
from mirbft_amd import MshaError
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

CAPTURE_MESSAGE = "make one call of this size outside the capture first"


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


def _launch(engine, case, stream=None, tensors=None, out=None, al=None):
    """One routed call; tensors, out and al: what is on the device already (a capture uploads nothing)."""
    import torch
    n = case.begin.size - 1 if case.action_list is None else case.action_list.size
    if out is None:
        out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    t = tensors or [_dev(x) for x in (case.arena, case.part_off, case.part_len, case.begin)]
    if al is None and case.action_list is not None:
        al = _dev(case.action_list)
    engine.hash_actions_device_routed(*t, out, action_list=al, stream=stream, long_blocks=case.long_blocks,
                                      max_long=case.max_long, long_bytes=case.long_bytes)
    return out


def _check_route(engine, case):
    ids, nbytes = engine.parts_route_lists()
    order = engine.parts_route_order()
    model = M.model_of(case)
    assert M.check_route(ids, nbytes, order, model) == []
    return ids, model


def _run(engine, case, status=None):
    """One call with everything asserted; status: the texts device_status() must raise
    with (None: clean). Returns the routed ids and the model."""
    s0, r0 = engine.stats(), engine.parts_route_stats()
    q0, c0, p0 = engine.parts_plan_stats(), engine.concat_stats(), engine.parts_stats()
    # held until device_status() has waited for the call: it only enqueues, on a stream torch's
    # allocator does not know, so inputs freed earlier could be handed out again under its kernels
    t = [_dev(x) for x in (case.arena, case.part_off, case.part_len, case.begin)]
    al = None if case.action_list is None else _dev(case.action_list)
    out = _launch(engine, case, tensors=t, al=al)
    if status is None:
        engine.device_status()
    else:
        with pytest.raises(MshaError) as ei:
            engine.device_status()
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG
        for text in status:
            assert text in str(ei.value)
        assert "msha_concat_lists_device" not in str(ei.value)        # never bit 16
        engine.device_status()                                       # reported once, then clean
    got = out.cpu().numpy()
    assert _bad_rows(got, M.expected_digests(case)) == []
    ids, model = _check_route(engine, case)
    s1, r1 = engine.stats(), engine.parts_route_stats()
    with_list = case.action_list is not None
    n_actions = case.action_list.size if with_list else model.n_lists
    assert r1["calls"] - r0["calls"] == 1 and r1["actions"] - r0["actions"] == n_actions
    assert r1["lists"] - r0["lists"] == model.n_lists
    assert r1["launches_plan"] - r0["launches_plan"] == (5 if with_list else 4)
    assert r1["launches_copy"] - r0["launches_copy"] == 1 and r1["launches_chain"] - r0["launches_chain"] == 1
    assert r1["launches_hash"] - r0["launches_hash"] == 1
    assert r1["launches_fill"] - r0["launches_fill"] == (1 if with_list else 0)
    if os.environ.get("MSHA_PARTS_TIMING") != "1":
        assert [r1[k] for k in ("last_lanes", "last_blocks", "last_routed", "last_routed_bytes", "last_kernel_ms")] \
            == [0, 0, 0, 0, 0.0]
    moved = {k: s1[k] - s0[k] for k in s1 if s1[k] != s0[k]}
    assert moved == {"launches_coop": 1, "launches_chain8": 1}
    assert (engine.parts_plan_stats(), engine.concat_stats(), engine.parts_stats()) == (q0, c0, p0)
    return ids, model


@gpu
def test_threshold_edge_named_once_often_and_never(engine):
    """long_blocks = 4 over lists of 2..5 blocks whose lengths sit 55, 56 and 64 bytes
    past a block multiple: exactly the named ones of 4 and 5 blocks are routed, whether
    one action names them or 300; the unnamed copies, whose parts lie outside the arena,
    are neither routed nor read."""
    case, (once, often, never) = M.threshold_edge()
    ids, model = _run(engine, case)
    want = {l for l in once + often if model.blocks[l] >= 4}
    assert set(ids.tolist()) == want == model.long and len(want) == 10


@gpu
@pytest.mark.parametrize("wave_sum", [None, "1"], ids=["default_T", "T1"])
def test_both_summing_paths(engine, monkeypatch, wave_sum):
    """A long list summed by its lane (3 parts, 2,000 bytes at an odd offset) and one
    summed by its wave (300 parts, empty ones among them), both routed; the same with
    every list summed by its wave."""
    if wave_sum:
        monkeypatch.setenv("MSHA_PARTS_PLAN_WAVE_SUM", wave_sum)
    case, (three, many) = M.summing_paths()
    ids, _ = _run(engine, case)
    assert sorted(ids.tolist()) == [three, many]


@gpu
def test_seventy_long_lists_in_a_row(engine):
    """70 long lists of 33 parts each: a wave sums 64 of them one after the other and
    every one claims its slot and room."""
    ids, _ = _run(engine, M.one_wave_of_long())
    assert sorted(ids.tolist()) == list(range(3, 73))


@gpu
def test_caps_never_fail_a_call(engine):
    """Five equal long lists: two slots; room for exactly three, then one byte less;
    one slot. The digests are right every time and the counts are the formula's."""
    r16 = M.round16(M.CAP_LEN)
    for max_long, long_bytes, want in ((2, 0, 2), (0, 3 * r16 + M.SLACK, 3), (0, 3 * r16 + M.SLACK - 1, 2),
                                       (1, 0, 1), (0, 0, 5), (4, 2 * r16 + M.SLACK + 15, 2)):
        ids, model = _run(engine, M.caps(max_long, long_bytes))
        assert len(ids) == want == model.count, (max_long, long_bytes)


@gpu
@pytest.mark.parametrize("with_list", [False, True], ids=["direct", "action_list"])
@pytest.mark.parametrize("n_lists", [64, 65, 257])
def test_no_long_list_and_every_list_long(engine, n_lists, with_list):
    ids, _ = _run(engine, M.uniform(n_lists, False, with_list))
    assert ids.size == 0
    ids, _ = _run(engine, M.uniform(n_lists, True, with_list))
    assert sorted(ids.tolist()) == list(range(n_lists))
    assert engine.parts_route_order().size == 0


@gpu
def test_empty_lists_routed_at_long_blocks_one(engine):
    """long_blocks = 1 makes the empty lists long too: they take a slot and no room, the
    copy has nothing to write for them and the chain hashes the empty message."""
    ids, model = _run(engine, M.empty_long())
    assert sorted(ids.tolist()) == [0, 1, 2, 4, 5, 6, 7] and engine.parts_route_lists()[1] == 352
    assert engine.parts_route_order().size == 0


@gpu
def test_device_errors_are_the_planned_entrys(engine):
    """An action_list id out of range: bit 8 and zeros. A decreasing part range on a
    list whose parts would make it long: bit 4, zeros for both actions naming it, and it
    is not routed. Both in one call, then each alone."""
    case = M.decreasing_long()
    ids, _ = _run(engine, case, status=("action_part_begin decreases", "action_list out of range"))
    assert sorted(ids.tolist()) == [1, 3, 4]
    al = case.action_list.copy()
    al[al == 5] = 0
    _run(engine, case._replace(action_list=al), status=("action_part_begin decreases",))
    al = case.action_list.copy()
    al[al == 2] = 0
    _run(engine, case._replace(action_list=al), status=("action_list out of range",))


@gpu
def test_host_checks_each_with_its_text(engine):
    import torch
    case = M.caps()
    lib, ctx = engine._lib, engine._ctx
    d = [_dev(x) for x in (case.arena, case.part_off, case.part_len, case.begin)]
    al = _dev(case.action_list)
    n_lists, n = case.begin.size - 1, case.action_list.size
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    args = [t.data_ptr() for t in d]
    f = lib.msha_hash_actions_device_routed
    r0 = engine.parts_route_stats()

    def refused(text, *a):
        assert f(ctx, *a) == L.MSHA_ERR_INVALID_ARG
        assert text in lib.msha_last_error(ctx), lib.msha_last_error(ctx)

    def opts(*v):
        import ctypes
        return ctypes.byref(L.MshaRouteOpts(*v))

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    refused(b"is above 16 x compute units", *args, n_lists, al.data_ptr(), n, opts(0, 16 * cus + 1, 0), out.data_ptr(), None)
    refused(b"it must be 0 or at least 80", *args, n_lists, al.data_ptr(), n, opts(0, 0, 79), out.data_ptr(), None)
    refused(b"is above 2^48", *args, n_lists, al.data_ptr(), n, opts(0, 0, (1 << 48) + 1), out.data_ptr(), None)
    refused(b"must equal n_lists", *args, n_lists, None, n_lists - 1, None, out.data_ptr(), None)
    refused(b"must be below 2^32 - 1", *args, 0xFFFFFFFF, al.data_ptr(), n, None, out.data_ptr(), None)
    refused(b"null pointer argument", args[0], None, args[2], args[3], n_lists, al.data_ptr(), n, None,
            out.data_ptr(), None)
    refused(b"null pointer argument", *args, n_lists, al.data_ptr(), n, None, None, None)
    refused(b"d_arena must be 16-byte aligned", args[0] + 1, *args[1:], n_lists, al.data_ptr(), n, None,
            out.data_ptr(), None)
    # no actions: MSHA_OK and nothing is launched; the bounds of the options accepted at their edges
    assert f(ctx, *args, n_lists, al.data_ptr(), 0, None, out.data_ptr(), None) == L.MSHA_OK
    assert f(ctx, *args, n_lists, al.data_ptr(), 0, opts(0, 16 * cus + 1, 79), None, None) == L.MSHA_OK   # opts unused
    assert engine.parts_route_stats() == r0 and not out.any()
    assert f(ctx, *args, n_lists, al.data_ptr(), n, opts(1, 16 * cus, 80), out.data_ptr(), None) == L.MSHA_OK
    engine.device_status()
    assert _bad_rows(out.cpu().numpy(), M.expected_digests(case)) == []
    assert engine.parts_route_lists()[0].size == 0                 # 80 bytes hold no list of 1,000


@gpu
def test_calls_of_different_shapes_share_one_context(engine):
    """Six routed calls of different shapes and options, a planned call, a routed call
    again: no slot, counter or order of one call shows in the next, and the planned
    entry's workspace is its own."""
    import torch
    cases = [M.one_wave_of_long(), M.uniform(65, False, True), M.caps(2, 0), M.threshold_edge()[0],
             M.uniform(257, True, False), M.summing_paths()[0]]
    for case in cases:
        _run(engine, case)
    case = cases[0]
    out = torch.zeros((case.begin.size - 1, 32), dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device_planned(*[_dev(x) for x in (case.arena, case.part_off, case.part_len, case.begin)],
                                       out)
    engine.device_status()
    assert _bad_rows(out.cpu().numpy(), M.expected_digests(case)) == []
    assert sorted(engine.parts_plan_order().tolist()) == list(range(case.begin.size - 1))
    ids, _ = engine.parts_route_lists()                            # the routed state is still the sixth call's
    assert sorted(ids.tolist()) == sorted(M.model_of(cases[5]).long)
    _run(engine, M.caps(1, 0))


@gpu
def test_workspace_grows_between_calls_on_two_streams():
    """A small call, one that must grow the workspace, the small one again, alternating
    between two caller streams with no host wait between them. A fresh context, so the
    first call allocates for 5 lists and a 4 KiB buffer (about 26 KB with its spare) and
    the second needs 300 lists and 64 KiB: the old buffer is freed under a call that may
    still be running, and the third call runs in the larger one at other offsets."""
    import torch
    from mirbft_amd import Engine
    small = M.uniform(5, True, False)._replace(max_long=4, long_bytes=4 << 10)
    large = M.uniform(300, True, False)._replace(max_long=4, long_bytes=64 << 10)
    assert small.long_blocks == large.long_blocks == 2
    calls = [small, large, small]
    t = [[_dev(x) for x in (c.arena, c.part_off, c.part_len, c.begin)] for c in calls]
    outs = [torch.zeros((c.begin.size - 1, 32), dtype=torch.uint8, device="cuda:0") for c in calls]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with Engine(1) as eng:
        torch.cuda.synchronize()
        for k, case in enumerate(calls):
            _launch(eng, case, stream=streams[k % 2], tensors=t[k], out=outs[k])
        torch.cuda.synchronize()
        eng.device_status()
        for k, case in enumerate(calls):
            assert _bad_rows(outs[k].cpu().numpy(), M.expected_digests(case)) == [], k
        ids, _ = _check_route(eng, small)                          # the last call's route: four slots, one lane
        assert len(ids) == 4 and eng.parts_route_order().size == 1
        assert eng.parts_route_stats()["calls"] == 3


@gpu
def test_capturable_into_a_graph(engine):
    """After one call of its size the routed call captures into a HIP graph; each replay
    hashes what the arena holds by then, long lists included."""
    import hashlib
    import torch
    case, (three, many) = M.summing_paths()
    t = [_dev(x) for x in (case.arena, case.part_off, case.part_len, case.begin)]
    n = case.begin.size - 1
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    _launch(engine, case, tensors=t, out=out)                      # the warm call
    engine.device_status()
    out.zero_()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            _launch(engine, case, stream=s, tensors=t, out=out)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert not out.any()
    off, ln, begin = case.part_off, case.part_len, case.begin
    for seed in (1, 2):
        fresh = np.random.default_rng(seed).integers(0, 256, case.arena.size, dtype=np.uint8)
        t[0].copy_(_dev(fresh))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        engine.device_status()
        host = fresh.tobytes()
        want = [hashlib.sha256(b"".join(host[int(off[j]):int(off[j] + ln[j])]
                                        for j in range(int(begin[i]), int(begin[i + 1])))).digest() for i in range(n)]
        want = np.frombuffer(b"".join(want), dtype=np.uint8).reshape(-1, 32)
        assert _bad_rows(out.cpu().numpy(), want) == [], seed
        assert sorted(engine.parts_route_lists()[0].tolist()) == [three, many]


@gpu
def test_capture_on_a_fresh_context_fails_cleanly():
    import torch
    from mirbft_amd import Engine
    case = M.caps()
    t = [_dev(x) for x in (case.arena, case.part_off, case.part_len, case.begin)]
    al = _dev(case.action_list)
    out = torch.zeros((case.action_list.size, 32), dtype=torch.uint8, device="cuda:0")
    with Engine(1) as eng:
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(MshaError) as ei:
                    _launch(eng, case, stream=s, tensors=t, out=out, al=al)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG and CAPTURE_MESSAGE in str(ei.value)
        assert "msha_hash_actions_device_routed" in str(ei.value)
        assert not out.any()
        _launch(eng, case, tensors=t, out=out, al=al)
        eng.device_status()
        assert _bad_rows(out.cpu().numpy(), M.expected_digests(case)) == []


@gpu
def test_equals_the_planned_entry_on_a_mixed_batch(engine):
    """4,096 actions over one-part, 20-part and five long lists, default options: the
    five are routed and every digest equals hash_actions_device_planned's (and hashlib's)."""
    import torch
    case, longs = M.mixed_batch()
    ids, _ = _run(engine, case)
    assert sorted(ids.tolist()) == sorted(longs)
    # the inputs of both calls stay alive, and nothing is allocated, until both have finished:
    # the calls only enqueue, on a stream torch's allocator does not know
    t = [_dev(x) for x in (case.arena, case.part_off, case.part_len, case.begin)]
    al = _dev(case.action_list)
    routed = torch.zeros((case.action_list.size, 32), dtype=torch.uint8, device="cuda:0")
    planned = torch.zeros_like(routed)
    torch.cuda.synchronize()
    _launch(engine, case, tensors=t, out=routed, al=al)
    engine.hash_actions_device_planned(*t, planned, action_list=al)
    engine.device_status()
    assert torch.equal(routed, planned)
    assert _bad_rows(routed.cpu().numpy(), M.expected_digests(case)) == []
