#!/usr/bin/env python3
"""What the device stream sets (msha_dstreams_*) cost: against the host stream sets on the
recorder's shape, and kernel against kernel over tools/parts_bench.py's part lists.

    python3 tools/dstream_bench.py recorder [--reps 7] [--out profiles/streams_device/recorder.jsonl]
    python3 tools/dstream_bench.py kernel   [--reps 7] [--out profiles/streams_device/kernel.jsonl]
    python3 tools/dstream_bench.py jobs     [--reps 7] [--out profiles/streams_device/jobs.jsonl]
    python3 tools/dstream_bench.py long     [--reps 7] [--out profiles/streams_device/long.jsonl]
    python3 tools/dstream_bench.py jobs_long [--reps 7] [--out profiles/streams_device/jobs_long.jsonl]

recorder  `--streams` (65,536) streams each appending `--digests` (20) 32-byte digests that
          sit in HBM as rows of a digest table (NodeState.Apply's shape, recorder.go:348).
          Both sets start with 32 bytes buffered in every stream (the state after a Snap).
          (a) device set: write_device + sum_device, one synchronisation at the end;
          (b) host set, the route without this feature: a D2H copy of the table, then
              StreamSet.write_packed + StreamSet.sum.
          Wall clock per repetition (the device idle before and after), (a) and (b)
          alternating in one process after a warm repetition of each.
kernel    k_dstream_write against k_digest_parts over the same part lists, lanes in list
          order for both (cases ec, c2, c2_odd as tools/parts_bench.py builds them), by
          the `last_kernel_ms` each call reports under MSHA_PARTS_TIMING=1 (set here).
          A write compresses the whole blocks only (no padding block), so each kernel's
          ns per lane-block is over the blocks it compressed; the ratio of the launch
          times is printed too.
jobs      the recorder's shape as NodeState.Apply produces it: the `--streams` x `--digests`
          digests arrive in commit order, job d * streams + s, the worst interleaving for a
          grouping by stream. Three routes to the same streams, each a write + sum_device
          with one synchronisation at the end, alternating after a warm repetition of each:
          (a) write_device with the grouped CSR given (the floor: the caller already did
              the grouping);
          (b) what a Python caller can do without this entry: torch.sort(stable=True) on
              the ids, searchsorted for the CSR, two gathers, then write_device;
          (c) write_jobs_device.
          (c) - (a) is the grouping's cost, (c) against (b) the gain over torch's sort.
          The same again for one small call (64 streams x 20 digests): the launch-bound
          end. Every stream's digest of every route is checked against hashlib outside
          the timed window.
long      write_routed_device against write_device, each a write + sum_device with one
          synchronisation at the end, alternating in one process after a warm repetition of
          each, the grouped CSR given, over streams x digests of 32 bytes: 4 x 8,192,
          64 x 2,048, 256 x 512 (few long streams: NodeState.ActiveHash's shape) and
          65,536 x 20 (no long row: what the routed call's extra launches cost). A gain or
          a loss is named only where the medians differ by more than the two spreads
          combined. Then the `long_blocks` sweep (8 .. 256) on 64 x 2,048 and on a mixed
          shape (65,536 x 20 with 32 streams of 2,048 among them). Every stream's digest of
          every route is checked against hashlib outside the timed window.
jobs_long `long`'s four shapes given as jobs in commit-major order (job d * streams + s), the
          call shape of NodeState.ActiveHash for a device-resident caller. Three arms, each a
          reset, the write, sum_device and one synchronisation, timed by wall clock,
          alternating in one process after a warm repetition of each:
          (a) write_jobs_device: every stream a lane, however long;
          (b) write_jobs_routed_device, all defaults;
          (c) write_routed_device on the grouped CSR given: the floor that grouping cannot
              beat.
          A sample of every repetition's digests is checked against hashlib outside the
          window. A difference is named only where it exceeds the two arms' spreads combined.
Every figure is the median of `--reps` (>= 5) timed repetitions after warm ones, with
(max - min) / median beside it. A sample of what was timed is checked against hashlib.
A measurement, not a threshold. Needs the GPU; there is no fallback.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(xs):
    med = statistics.median(xs)
    return {"median": round(med, 5), "min": round(min(xs), 5), "max": round(max(xs), 5),
            "spread": round((max(xs) - min(xs)) / med, 4), "all": [round(x, 5) for x in xs]}


def _up(x, dev):
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).to(dev)


def recorder(a, build):
    import torch
    from mirbft_amd import DeviceStreamSet, Engine, StreamSet
    dev = torch.device("cuda:0")
    n, k = a.streams, a.digests
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    table = torch.randint(0, 256, (n * k * 32 + 64,), dtype=torch.uint8, device=dev, generator=g)
    part_off = torch.arange(n * k, dtype=torch.int64, device=dev) * 32
    part_len = torch.full((n * k,), 32, dtype=torch.int64, device=dev)
    begin = torch.arange(n + 1, dtype=torch.int64, device=dev) * k
    one = torch.arange(n + 1, dtype=torch.int64, device=dev)           # the seeding write: digest row s to stream s
    out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    ids = np.repeat(np.arange(n, dtype=np.uint64), k)
    h_off = 32 * np.arange(n * k, dtype=np.uint64)
    h_len = np.full(n * k, 32, dtype=np.uint64)
    torch.cuda.synchronize()
    t_dev, t_host, t_d2h, writes = [], [], [], 0
    with Engine(1) as eng, DeviceStreamSet(eng, n) as ds, StreamSet(eng, n) as hs:
        ds.write_device(table, part_off, part_len, one)
        host_table = table.cpu().numpy()
        hs.write_packed(host_table, np.arange(n, dtype=np.uint64), h_off[:n], h_len[:n])
        for rep in range(a.reps + 1):                                  # the first of each is the warm one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds.write_device(table, part_off, part_len, begin)
            ds.sum_device(out)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            host_table = table.cpu().numpy()
            t2 = time.perf_counter()
            hs.write_packed(host_table, ids, h_off, h_len)
            host_sums = hs.sum()
            t3 = time.perf_counter()
            writes += 1
            if rep:
                t_dev.append((t1 - t0) * 1e3)
                t_d2h.append((t2 - t1) * 1e3)
                t_host.append((t3 - t1) * 1e3)
        eng.device_status()
        dev_sums = out.cpu().numpy()
        st = ds.stats()
        for s in (0, 1, n // 2, n - 1):                                # both against hashlib
            rows = host_table[: n * k * 32].reshape(n, k * 32)
            seed = host_table[32 * s: 32 * s + 32].tobytes()           # the seeding write: part s
            want = hashlib.sha256(seed + rows[s].tobytes() * writes).digest()
            assert dev_sums[s].tobytes() == want, ("device set", s)
            assert host_sums[s].tobytes() == want, ("host set", s)
    a_, b_ = _stat(t_dev), _stat(t_host)
    gap = b_["median"] - a_["median"]
    spreads = (a_["max"] - a_["min"]) + (b_["max"] - b_["min"])
    return [{"measure": "recorder", "streams": n, "digests_per_stream": k, "bytes": n * k * 32, "reps": a.reps,
             "device_ms": a_, "host_ms": b_, "host_d2h_ms": _stat(t_d2h),
             "host_over_device": round(b_["median"] / a_["median"], 3),
             "gap_ms": round(gap, 4), "spreads_combined_ms": round(spreads, 4),
             "device_faster_by_more_than_the_spreads": bool(gap > spreads),
             "device_launches": st["launches"], "build": build["id"]}]


def _jobs_shape(eng, n, k, reps, build, label):
    import torch
    from mirbft_amd import DeviceStreamSet
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    table = torch.randint(0, 256, (n * k * 32 + 64,), dtype=torch.uint8, device=dev, generator=g)
    # commit-major: job j = d * n + s is digest d of stream s, at table row j
    job_stream = torch.arange(n, dtype=torch.int32, device=dev).repeat(k)
    job_off = torch.arange(n * k, dtype=torch.int64, device=dev) * 32
    job_len = torch.full((n * k,), 32, dtype=torch.int64, device=dev)
    # (a)'s input, prepared outside the window: the same jobs grouped by stream
    perm = torch.arange(n * k, dtype=torch.int64, device=dev).view(k, n).t().contiguous().view(-1)
    g_off, g_len = job_off[perm].contiguous(), job_len[perm].contiguous()
    begin = torch.arange(n + 1, dtype=torch.int64, device=dev) * k
    out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    host = table.cpu().numpy()[: n * k * 32].reshape(k, n, 32)
    want = np.frombuffer(b"".join(hashlib.sha256(host[:, s].tobytes()).digest() for s in range(n)),
                         dtype=np.uint8).reshape(n, 32)
    torch.cuda.synchronize()

    def route_a(ds):
        ds.write_device(table, g_off, g_len, begin)

    def route_b(ds):
        keys, order = torch.sort(job_stream, stable=True)
        b = torch.searchsorted(keys, torch.arange(n + 1, dtype=torch.int32, device=dev)).to(torch.int64)
        torch.cuda.current_stream().synchronize()      # torch's stream, then the context's: what a caller must do
        ds.write_device(table, job_off[order].contiguous(), job_len[order].contiguous(), b)

    def route_c(ds):
        ds.write_jobs_device(table, job_stream, job_off, job_len)

    times = {"a": [], "b": [], "c": []}
    passes = launches = 0
    with DeviceStreamSet(eng, n) as ds:
        for rep in range(reps + 1):                    # the first of each is the warm one
            for name, route in (("a", route_a), ("b", route_b), ("c", route_c)):
                ds.reset_device()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                route(ds)
                ds.sum_device(out)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                # every digest, outside the window
                assert np.array_equal(out.cpu().numpy(), want), (label, name, rep)
                if rep:
                    times[name].append((t1 - t0) * 1e3)
        eng.device_status()
        js = ds.jobs_stats()
        passes, launches = js["last_passes"], (js["launches_sort"] + js["launches_rows"] + js["launches_write"]) // js["calls"]
    a_, b_, c_ = (_stat(times[x]) for x in "abc")
    spread = lambda s: s["max"] - s["min"]             # noqa: E731
    return {"measure": "jobs", "shape": label, "streams": n, "digests_per_stream": k, "jobs": n * k, "reps": reps,
            "csr_given_ms": a_, "torch_sort_ms": b_, "write_jobs_ms": c_,
            "grouping_cost_ms": round(c_["median"] - a_["median"], 4),
            "jobs_minus_torch_ms": round(c_["median"] - b_["median"], 4),
            "jobs_over_torch": round(c_["median"] / b_["median"], 3),
            "spreads_jobs_torch_ms": round(spread(b_) + spread(c_), 4),
            "jobs_slower_than_torch_by_more_than_the_spreads": bool(c_["median"] - b_["median"] > spread(b_) + spread(c_)),
            "jobs_faster_than_torch_by_more_than_the_spreads": bool(b_["median"] - c_["median"] > spread(b_) + spread(c_)),
            "passes": passes, "launches_per_jobs_call": launches, "build": build["id"]}


def jobs(a, build):
    from mirbft_amd import Engine
    with Engine(1) as eng:
        return [_jobs_shape(eng, a.streams, a.digests, a.reps, build, "recorder"),
                _jobs_shape(eng, 64, 20, a.reps, build, "small")]


def _long_shape(eng, n, k, reps, build, label, long_blocks=(0,), big=None):
    """n streams x k digests; big = (count, digests): that many streams take `digests` instead."""
    import torch
    from mirbft_amd import DeviceStreamSet
    dev = torch.device("cuda:0")
    per = np.full(n, k, dtype=np.int64)
    if big:
        per[np.linspace(0, n - 1, big[0]).astype(np.int64)] = big[1]
    begin_h = np.concatenate([[0], np.cumsum(per)])
    total = int(begin_h[-1])
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    table = torch.randint(0, 256, (total * 32 + 64,), dtype=torch.uint8, device=dev, generator=g)
    part_off = torch.arange(total, dtype=torch.int64, device=dev) * 32
    part_len = torch.full((total,), 32, dtype=torch.int64, device=dev)
    begin = torch.from_numpy(begin_h).to(dev)
    out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    host = table.cpu().numpy()
    check = sorted(set([0, 1, n // 2, n - 1] + (np.linspace(0, n - 1, big[0]).astype(int).tolist() if big else [])))
    want = {s: hashlib.sha256(host[32 * begin_h[s]: 32 * begin_h[s + 1]].tobytes()).digest() for s in check}
    torch.cuda.synchronize()
    lines = []
    with DeviceStreamSet(eng, n) as ds:
        for lb in long_blocks:
            routes = (("lanes", lambda: ds.write_device(table, part_off, part_len, begin)),
                      ("routed", lambda: ds.write_routed_device(table, part_off, part_len, begin, long_blocks=lb)))
            times = {"lanes": [], "routed": []}
            for rep in range(reps + 1):                # the first of each is the warm one
                for name, route in routes:
                    ds.reset_device()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    route()
                    ds.sum_device(out)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    got = out.cpu().numpy()
                    for s_, w in want.items():
                        assert got[s_].tobytes() == w, (label, name, lb, rep, s_)
                    if rep:
                        times[name].append((t1 - t0) * 1e3)
            eng.device_status()
            routed_rows, routed_bytes = ds.routed_rows()
            a_, b_ = _stat(times["lanes"]), _stat(times["routed"])
            spreads = (a_["max"] - a_["min"]) + (b_["max"] - b_["min"])
            gap = a_["median"] - b_["median"]
            lines.append({"measure": "long", "shape": label, "streams": n, "digests_per_stream": k,
                          "big": list(big) if big else None, "bytes": total * 32, "reps": reps,
                          "long_blocks": lb or "default", "routed_rows": int(routed_rows.size),
                          "routed_bytes": int(routed_bytes), "write_device_ms": a_, "write_routed_ms": b_,
                          "lanes_over_routed": round(a_["median"] / b_["median"], 3), "gap_ms": round(gap, 4),
                          "spreads_combined_ms": round(spreads, 4),
                          "routed_faster_by_more_than_the_spreads": bool(gap > spreads),
                          "routed_slower_by_more_than_the_spreads": bool(-gap > spreads), "build": build["id"]})
    return lines


def long_rows(a, build):
    from mirbft_amd import Engine
    sweep = (8, 16, 32, 64, 128, 256)
    with Engine(1) as eng:
        lines = []
        for label, n, k in (("a", 4, 8192), ("b", 64, 2048), ("c", 256, 512), ("d", 1 << 16, 20)):
            lines += _long_shape(eng, n, k, a.reps, build, label)
        lines += _long_shape(eng, 64, 2048, a.reps, build, "b_sweep", sweep)
        lines += _long_shape(eng, 1 << 16, 20, a.reps, build, "mixed_sweep", sweep, big=(32, 2048))
        return lines


def _jobs_long_shape(eng, n, k, reps, build, label):
    import torch
    from mirbft_amd import DeviceStreamSet
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(13)
    table = torch.randint(0, 256, (n * k * 32 + 64,), dtype=torch.uint8, device=dev, generator=g)
    # commit-major: job j = d * n + s is digest d of stream s, at table row j
    job_stream = torch.arange(n, dtype=torch.int32, device=dev).repeat(k)
    job_off = torch.arange(n * k, dtype=torch.int64, device=dev) * 32
    job_len = torch.full((n * k,), 32, dtype=torch.int64, device=dev)
    # (c)'s input, prepared outside the window: the same jobs grouped by stream
    perm = torch.arange(n * k, dtype=torch.int64, device=dev).view(k, n).t().contiguous().view(-1)
    g_off, g_len = job_off[perm].contiguous(), job_len[perm].contiguous()
    begin = torch.arange(n + 1, dtype=torch.int64, device=dev) * k
    out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    host = table.cpu().numpy()[: n * k * 32].reshape(k, n, 32)
    check = sorted({0, 1, n // 2, n - 1})
    want = {s: hashlib.sha256(host[:, s].tobytes()).digest() for s in check}
    torch.cuda.synchronize()
    with DeviceStreamSet(eng, n) as ds:
        arms = (("jobs", lambda: ds.write_jobs_device(table, job_stream, job_off, job_len)),
                ("jobs_routed", lambda: ds.write_jobs_routed_device(table, job_stream, job_off, job_len)),
                ("routed_csr", lambda: ds.write_routed_device(table, g_off, g_len, begin)))
        times = {name: [] for name, _ in arms}
        for rep in range(reps + 1):                    # the first of each is the warm one
            for name, arm in arms:
                ds.reset_device()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arm()
                ds.sum_device(out)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                got = out.cpu().numpy()
                for s_, w in want.items():
                    assert got[s_].tobytes() == w, (label, name, rep, s_)
                if rep:
                    times[name].append((t1 - t0) * 1e3)
        eng.device_status()
        routed = int(ds.jobs_route_read()[2].size)
        st = ds.jobs_route_stats()
        launches = sum(v for f, v in st.items() if f.startswith("launches_")) // st["calls"]
    a_, b_, c_ = (_stat(times[x]) for x in ("jobs", "jobs_routed", "routed_csr"))
    spread = lambda s: s["max"] - s["min"]             # noqa: E731
    gain, over = a_["median"] - b_["median"], b_["median"] - c_["median"]
    return {"measure": "jobs_long", "shape": label, "streams": n, "digests_per_stream": k, "jobs": n * k,
            "bytes": n * k * 32, "reps": reps, "routed_streams": routed, "passes": st["last_passes"],
            "launches_per_jobs_routed_call": launches,
            "write_jobs_ms": a_, "write_jobs_routed_ms": b_, "write_routed_csr_ms": c_,
            "jobs_over_jobs_routed": round(a_["median"] / b_["median"], 3),
            "jobs_minus_jobs_routed_ms": round(gain, 4), "spreads_jobs_jobs_routed_ms": round(spread(a_) + spread(b_), 4),
            "jobs_routed_faster_than_jobs_by_more_than_the_spreads": bool(gain > spread(a_) + spread(b_)),
            "jobs_routed_slower_than_jobs_by_more_than_the_spreads": bool(-gain > spread(a_) + spread(b_)),
            "jobs_routed_minus_csr_ms": round(over, 4), "spreads_jobs_routed_csr_ms": round(spread(b_) + spread(c_), 4),
            "jobs_routed_above_the_floor_by_more_than_the_spreads": bool(over > spread(b_) + spread(c_)),
            "build": build["id"]}


def jobs_long(a, build):
    from mirbft_amd import Engine
    with Engine(1) as eng:
        return [_jobs_long_shape(eng, n, k, a.reps, build, label)
                for label, n, k in (("a", 4, 8192), ("b", 64, 2048), ("c", 256, 512), ("d", 1 << 16, 20))]


def _blocks(length):
    length = length.astype(np.uint64)
    return (length >> np.uint64(6)) + np.where((length & np.uint64(63)) < 56, 1, 2).astype(np.uint64)


def kernel(a, build):
    import torch
    from mirbft_amd import DeviceStreamSet, Engine
    from mirbft_amd.workloads import epoch_change_parts_pool, scatter_parts
    dev = torch.device("cuda:0")
    cases = {}
    pool = epoch_change_parts_pool(max_set=a.ec_max_set)
    p_arena, p_off, p_len, p_begin = scatter_parts(pool)
    n_pool, n_parts, c = len(pool), int(p_off.size), a.ec_copies
    m_len = np.array([sum(len(p) for p in m) for m in pool], dtype=np.uint64)
    step = torch.arange(c, dtype=torch.int64, device=dev).repeat_interleave(n_pool) * n_parts
    cases["ec"] = dict(arena=_up(p_arena, dev), off=_up(p_off, dev).repeat(c), len=_up(p_len, dev).repeat(c),
                       begin=torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                        _up(p_begin[1:], dev).repeat(c) + step]),
                       lens=np.tile(m_len, c), digests=[hashlib.sha256(b"".join(m)).digest() for m in pool])
    n, msg, stride = a.lanes, 512, 528
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    c2_arena = torch.randint(0, 256, (n * stride + 64,), dtype=torch.uint8, device=dev, generator=g)
    c2_off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    c2_len = torch.full((n,), msg, dtype=torch.int64, device=dev)
    c2_begin = torch.arange(n + 1, dtype=torch.int64, device=dev)
    for name, shift in (("c2", 0), ("c2_odd", 1)):
        cases[name] = dict(arena=c2_arena, off=c2_off + shift, len=c2_len, begin=c2_begin,
                           lens=np.full(n, msg, dtype=np.uint64), digests=None, shift=shift)
    lines = []
    torch.cuda.synchronize()
    with Engine(1) as eng:
        for name, cs in cases.items():
            lanes = cs["lens"].size
            out_p = torch.zeros((lanes, 32), dtype=torch.uint8, device=dev)
            out_s = torch.zeros((lanes, 32), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            t_parts, t_write, per_parts, per_write = [], [], [], []
            parts_blocks = int(_blocks(cs["lens"]).sum())
            with DeviceStreamSet(eng, lanes) as ds:
                t_start, rep, written = time.perf_counter(), 0, 0
                while rep < a.reps:                    # warm repetitions first (at least one), untimed
                    warming = written == 0 or (rep == 0 and (time.perf_counter() - t_start) * 1e3 < a.min_warmup_ms)
                    eng.hash_actions_device(cs["arena"], cs["off"], cs["len"], cs["begin"], out_p)
                    ms_p = eng.parts_stats()["last_kernel_ms"]
                    ds.write_device(cs["arena"], cs["off"], cs["len"], cs["begin"])
                    ms_w = ds.stats()["last_kernel_ms"]
                    # whole blocks this write compressed: the streams held `written` copies before it
                    wb = int((((written + 1) * cs["lens"]) >> np.uint64(6)).sum() - ((written * cs["lens"]) >> np.uint64(6)).sum())
                    written += 1
                    if not warming:
                        rep += 1
                        t_parts.append(ms_p)
                        t_write.append(ms_w)
                        per_parts.append(ms_p * 1e6 / parts_blocks)
                        per_write.append(ms_w * 1e6 / wb)
                assert min(t_parts) > 0 and min(t_write) > 0, "MSHA_PARTS_TIMING=1 did not take effect"
                ds.reset_device()
                ds.write_device(cs["arena"], cs["off"], cs["len"], cs["begin"])
                ds.sum_device(out_s)
                eng.device_status()
            for i in [0, 1, 63, 64, lanes // 2, lanes - 1]:            # what was timed computed the right thing
                if cs["digests"]:
                    want = cs["digests"][i % n_pool]
                else:
                    want = hashlib.sha256(c2_arena[i * stride + cs["shift"]: i * stride + cs["shift"] + msg]
                                          .cpu().numpy().tobytes()).digest()
                assert out_p[i].cpu().numpy().tobytes() == want, (name, "parts", i)
                assert out_s[i].cpu().numpy().tobytes() == want, (name, "stream", i)
            sp, sw = _stat(per_parts), _stat(per_write)
            lines.append({"measure": "kernel", "case": name, "lanes": lanes, "reps": a.reps,
                          "warm_reps": written - a.reps, "digest_parts_blocks": parts_blocks,
                          "digest_parts_ms": _stat(t_parts), "dstream_write_ms": _stat(t_write),
                          "digest_parts_ns_per_lane_block": sp, "dstream_write_ns_per_lane_block": sw,
                          "write_over_parts_per_lane_block": round(sw["median"] / sp["median"], 4),
                          "write_over_parts_ms": round(statistics.median(t_write) / statistics.median(t_parts), 4),
                          "build": build["id"]})
    return lines


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("measure", choices=["recorder", "kernel", "jobs", "long", "jobs_long"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--streams", type=int, default=1 << 16)
    ap.add_argument("--digests", type=int, default=20)
    ap.add_argument("--lanes", type=int, default=1 << 20, help="rows of the c2 cases")
    ap.add_argument("--ec-copies", type=int, default=656, help="copies of the 100-payload pool (656: 65,600 lanes)")
    ap.add_argument("--ec-max-set", type=int, default=1000)
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default="", help="the JSON lines are written to this file too (replacing it)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    if a.measure == "kernel":
        os.environ["MSHA_PARTS_TIMING"] = "1"      # read by the library at each call
    elif os.environ.get("MSHA_PARTS_TIMING") == "1":
        ap.error("%s measures enqueue-only calls: unset MSHA_PARTS_TIMING" % a.measure)
    from mirbft_amd import _lib
    build = _lib.require_tree_build("dstream_bench")
    lines = {"recorder": recorder, "kernel": kernel, "jobs": jobs, "long": long_rows, "jobs_long": jobs_long}[a.measure](a, build)
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
