#!/usr/bin/env python3
"""What the byte-granular gather of msha_hash_actions_device costs against the lane
kernel over the same bytes pre-concatenated, kernel-resident.

    python3 tools/parts_bench.py [--reps 9] [--out profiles/parts/parts_bench.jsonl]

Cases, each a pair (parts: hash_actions_device; lane: digest_batch_device, the
yardstick, over the same messages concatenated at 16-byte aligned starts):
  ec        the c5 EpochChange pool (workloads.epoch_change_parts_pool: 100 payloads as
            epochChangeHashData yields them, |P|, |Q| up to 1000) scattered
            (workloads.scatter_parts: the 8-byte big-endian fields in one region, digests
            and checkpoint values in another), `--ec-copies` copies of it so the launch
            has a wave a SIMD; both kernels run the lanes in descending block order
  c2        `--lanes` actions of one 512-byte part at 16-byte aligned offsets
  c2_odd    the same parts one byte further (offsets = 1 mod 16)
All pairs alternate in one process; each is timed with HIP events (warm-up repetitions
for 300 ms so the clock settles, then `reps` timed ones; a repetition is `inner`
launches back to back between one pair of events). Prints one JSON line a kernel and
case (ns per lane-block of every repetition, the median, (max - min) / median) and
one ratio line a case. A sample of the digests of what was timed is checked against
hashlib. A measurement, not a threshold. Needs the GPU; there is no fallback.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _blocks(length: np.ndarray) -> np.ndarray:
    length = length.astype(np.uint64)
    return (length >> np.uint64(6)) + np.where((length & np.uint64(63)) < 56, 1, 2).astype(np.uint64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lanes", type=int, default=1 << 20, help="actions of the c2 cases")
    ap.add_argument("--ec-copies", type=int, default=656, help="copies of the 100-payload pool (656: 65,600 lanes)")
    ap.add_argument("--ec-max-set", type=int, default=1000)
    ap.add_argument("--inner", type=int, default=4, help="launches between one pair of events")
    ap.add_argument("--min-warmup-ms", type=float, default=300.0,
                    help="warm-up repetitions go on until this much time has passed (the clock settles)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "parts", "parts_bench.jsonl"),
                    help="the JSON lines are written to this file too (replacing it; '' for none)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    import torch
    from mirbft_amd import Engine, _lib
    from mirbft_amd.engine import order_by_blocks
    from mirbft_amd.workloads import epoch_change_parts_pool, scatter_parts
    build = _lib.require_tree_build("parts_bench")
    dev = torch.device("cuda:0")

    def up(x):
        x = np.ascontiguousarray(x)
        if x.dtype == np.uint64:
            x = x.view(np.int64)
        if x.dtype == np.uint32:
            x = x.view(np.int32)
        return torch.from_numpy(x.copy()).to(dev)

    cases = {}      # name -> dict(parts=fn, lane=fn, lanes, blocks (lane-blocks a launch), check=fn)

    # -- ec: the pool in parts form, scattered; and concatenated for the lane kernel
    pool = epoch_change_parts_pool(max_set=a.ec_max_set)
    p_arena, p_off, p_len, p_begin = scatter_parts(pool)
    n_pool, n_parts = len(pool), int(p_off.size)
    joined = [b"".join(m) for m in pool]
    m_len = np.array([len(m) for m in joined], dtype=np.uint64)
    m_off = np.zeros(n_pool, dtype=np.uint64)
    m_off[1:] = np.cumsum((m_len + np.uint64(15)) & ~np.uint64(15))[:-1]
    m_arena = np.zeros(int(m_off[-1] + m_len[-1]) + 64, dtype=np.uint8)
    for m, o in zip(joined, m_off):
        m_arena[int(o):int(o) + len(m)] = np.frombuffer(m, dtype=np.uint8)
    c = a.ec_copies
    n_ec = n_pool * c
    ec_arena, ec_marena = up(p_arena), up(m_arena)
    ec_off, ec_len = up(p_off).repeat(c), up(p_len).repeat(c)          # copy k's parts name the same bytes
    step = torch.arange(c, dtype=torch.int64, device=dev).repeat_interleave(n_pool) * n_parts
    ec_begin = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), up(p_begin[1:]).repeat(c) + step])
    ec_moff, ec_mlen = up(m_off).repeat(c), up(m_len).repeat(c)
    ec_order = up(order_by_blocks(np.tile(m_len, c)))
    ec_out_p = torch.zeros((n_ec, 32), dtype=torch.uint8, device=dev)
    ec_out_l = torch.zeros((n_ec, 32), dtype=torch.uint8, device=dev)
    ec_digests = [hashlib.sha256(m).digest() for m in joined]

    # -- c2: one 512-byte part an action, aligned and odd starts (stride 528 leaves room for both)
    n, msg, stride = a.lanes, 512, 528
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    c2_arena = torch.randint(0, 256, (n * stride + 64,), dtype=torch.uint8, device=dev, generator=g)
    c2_off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    c2_off_odd = c2_off + 1
    c2_len = torch.full((n,), msg, dtype=torch.int64, device=dev)
    c2_begin = torch.arange(n + 1, dtype=torch.int64, device=dev)
    c2_out = {k: torch.zeros((n, 32), dtype=torch.uint8, device=dev) for k in ("parts", "odd", "lane")}

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with Engine(1) as eng:
        cases["ec"] = {
            "parts": lambda: eng.hash_actions_device(ec_arena, ec_off, ec_len, ec_begin, ec_out_p, stream=stream,
                                                     order=ec_order),
            "lane": lambda: eng.digest_batch_device(ec_marena, ec_moff, ec_mlen, ec_out_l, stream=stream,
                                                    order=ec_order),
            "lanes": n_ec, "blocks": int(_blocks(m_len).sum()) * c,
            "shape": {"copies": c, "pool": n_pool, "parts_per_copy": n_parts, "bytes_per_copy": int(m_len.sum())}}
        lane_c2 = lambda: eng.digest_batch_device(c2_arena, c2_off, c2_len, c2_out["lane"], stream=stream)  # noqa: E731
        cases["c2"] = {
            "parts": lambda: eng.hash_actions_device(c2_arena, c2_off, c2_len, c2_begin, c2_out["parts"],
                                                     stream=stream),
            "lane": lane_c2, "lanes": n, "blocks": 9 * n, "shape": {"part_bytes": msg, "start_mod_16": 0}}
        cases["c2_odd"] = {
            "parts": lambda: eng.hash_actions_device(c2_arena, c2_off_odd, c2_len, c2_begin, c2_out["odd"],
                                                     stream=stream),
            "lane": lane_c2, "lanes": n, "blocks": 9 * n, "shape": {"part_bytes": msg, "start_mod_16": 1}}

        times = {(k, w): [] for k in cases for w in ("parts", "lane")}
        t_start, rep, warm = time.perf_counter(), 0, 0
        while rep < a.reps:                    # warm-up repetitions first (at least one), untimed
            warming = warm == 0 or (time.perf_counter() - t_start) * 1e3 < a.min_warmup_ms
            if warming and rep == 0:
                warm += 1
            else:
                rep += 1
            for (k, w), ts in times.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.inner):
                    cases[k][w]()
                e1.record(stream)
                e1.synchronize()
                if rep:
                    ts.append(e0.elapsed_time(e1) / a.inner)
        eng.device_status()

    # what was timed computed the right thing (a sample, against hashlib)
    for i in [0, 1, 99, 100, n_ec // 2, n_ec - 1]:
        assert bytes(ec_out_p[i].cpu().numpy()) == ec_digests[i % n_pool], ("ec parts", i)
        assert bytes(ec_out_l[i].cpu().numpy()) == ec_digests[i % n_pool], ("ec lane", i)
    for i in [0, 1, 63, 64, n // 2, n - 1]:
        host = c2_arena[i * stride:i * stride + msg + 1].cpu().numpy().tobytes()
        assert bytes(c2_out["parts"][i].cpu().numpy()) == hashlib.sha256(host[:msg]).digest(), ("c2 parts", i)
        assert bytes(c2_out["lane"][i].cpu().numpy()) == hashlib.sha256(host[:msg]).digest(), ("c2 lane", i)
        assert bytes(c2_out["odd"][i].cpu().numpy()) == hashlib.sha256(host[1:]).digest(), ("c2 odd", i)

    lines = []
    for k, case in cases.items():
        med = {}
        for w in ("parts", "lane"):
            per = [t * 1e6 / case["blocks"] for t in times[(k, w)]]
            med[w] = statistics.median(per)
            lines.append({"case": k, "kernel": w, "lanes": case["lanes"], "lane_blocks": case["blocks"],
                          "shape": case["shape"], "reps": a.reps, "inner": a.inner, "warmup_reps": warm,
                          "kernel_ms": [round(t, 4) for t in times[(k, w)]],
                          "ns_per_lane_block": [round(p, 5) for p in per],
                          "median_ns_per_lane_block": round(med[w], 5),
                          "spread": round((max(per) - min(per)) / med[w], 4), "build": build["id"]})
        lines.append({"case": k, "parts_over_lane": round(med["parts"] / med["lane"], 4)})
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
