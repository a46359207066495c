#!/usr/bin/env python3
"""Rate of the stream sets' absorb kernel against the lane kernel, kernel-resident.

    python3 tools/stream_bench.py [--reps 7] [--lanes 1048576] [--out profiles/streams/bench.jsonl]
    python3 tools/stream_bench.py --chain [--reps 7] [--out profiles/streams_device/long.jsonl]

Two cases over the same device arena of `lanes` x 512 bytes, alternated in one
process, each timed with HIP events (warm-up repetitions for 300 ms, then `reps` timed ones; a
repetition is `inner` launches back to back between one pair of events, so the host's
enqueue time hides behind the kernel before it and is paid once a repetition):
  absorb  msha_absorb_device, 8 whole blocks a lane
  lane    msha_digest_batch_device, 512-byte messages: 9 blocks a lane (8 + padding);
          the yardstick, untouched by the stream sets
--chain: msha_absorb_chain_device (eight lanes a stream) against msha_absorb_device (one)
at 4, 64, 1,024 and 4,096 lanes of 1,024 blocks each, one launch between a pair of events,
in ns per block of the launch (launch time / (lanes x blocks)); the states of both are
compared. It shows where eight lanes a stream stop paying. A case line each, no verdict.
Prints one JSON line a case (ns per lane-block of every repetition, the median and
(max - min) / median) and a verdict line: absorb's per-block median should be no
worse than the lane kernel's by more than the larger of the two spreads. The
digests / states of one repetition are checked against hashlib on a sample. Needs
the GPU; there is no fallback.
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

IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def chain_cases(a, build):
    import torch
    from mirbft_amd import Engine
    dev = torch.device("cuda:0")
    blocks = 1024
    stream = torch.cuda.Stream(dev)
    lines = []
    with Engine(1) as eng:
        for n in (4, 64, 1024, 4096):
            g = torch.Generator(device=dev)
            g.manual_seed(6)
            arena = torch.randint(0, 256, (n * blocks * 64 + 64,), dtype=torch.uint8, device=dev, generator=g)
            off = torch.arange(n, dtype=torch.int64, device=dev) * (blocks * 64)
            nblocks = torch.full((n,), blocks, dtype=torch.int64, device=dev)
            iv = torch.from_numpy(np.tile(np.array(IV, dtype=np.uint32), (n, 1)).view(np.int32)).to(dev)
            states = {"chain": iv.clone(), "lane": iv.clone()}
            fns = {"chain": eng.absorb_chain_device, "lane": eng.absorb_device}
            times = {"chain": [], "lane": []}
            torch.cuda.synchronize()
            t_start, rep, warm = time.perf_counter(), 0, 0
            while rep < a.reps:                    # warm-up repetitions first (at least one), untimed
                warming = warm == 0 or (time.perf_counter() - t_start) * 1e3 < a.min_warmup_ms
                if warming and rep == 0:
                    warm += 1
                else:
                    rep += 1
                for name in ("chain", "lane"):
                    with torch.cuda.stream(stream):
                        states[name].copy_(iv)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fns[name](states[name], arena, off, nblocks, stream=stream)
                    e1.record(stream)
                    e1.synchronize()
                    if rep:
                        times[name].append(e0.elapsed_time(e1))
            eng.device_status()
            assert torch.equal(states["chain"], states["lane"]), n
            row = {"case": "chain", "lanes": n, "blocks_per_lane": blocks, "reps": a.reps, "warmup_reps": warm,
                   "build": build["id"]}
            for name in ("chain", "lane"):
                per = [t * 1e6 / (n * blocks) for t in times[name]]
                med = statistics.median(per)
                row[name + "_ms"] = [round(t, 4) for t in times[name]]
                row[name + "_median_ns_per_block"] = round(med, 4)
                row[name + "_spread"] = round((max(per) - min(per)) / med, 4)
            row["lane_over_chain"] = round(row["lane_median_ns_per_block"] / row["chain_median_ns_per_block"], 3)
            lines.append(row)
    return lines


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain", action="store_true", help="the eight-lane absorb chain against the lane absorb")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--inner", type=int, default=8, help="launches between one pair of events")
    ap.add_argument("--min-warmup-ms", type=float, default=300.0,
                    help="warm-up repetitions go on until this much time has passed (the clock settles)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    import torch
    from mirbft_amd import Engine, _lib
    build = _lib.require_tree_build("stream_bench")
    if a.chain:
        lines = chain_cases(a, build)
        for ln in lines:
            print(json.dumps(ln))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")
        return 0
    dev = torch.device("cuda:0")
    n, msg = a.lanes, 512
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    arena = torch.randint(0, 256, (n * msg + 64,), dtype=torch.uint8, device=dev, generator=g)
    off = torch.arange(n, dtype=torch.int64, device=dev) * msg
    length = torch.full((n,), msg, dtype=torch.int64, device=dev)
    nblocks = torch.full((n,), msg // 64, dtype=torch.int64, device=dev)
    iv = torch.from_numpy(np.tile(np.array(IV, dtype=np.uint32), (n, 1)).view(np.int32)).to(dev)
    state = iv.clone()
    out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    # a stream of this run's own: the library's calls, the state's re-initialisation and
    # the events all go to it, in order (the null stream does not order the context's)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    with Engine(1) as eng:
        def absorb():
            eng.absorb_device(state, arena, off, nblocks, stream=stream)

        def lane():
            eng.digest_batch_device(arena, off, length, out, stream=stream)

        cases = {"absorb": (absorb, msg // 64), "lane": (lane, msg // 64 + 1)}
        times = {k: [] for k in cases}
        t_start, rep, warm = time.perf_counter(), 0, 0
        while rep < a.reps:                    # warm-up repetitions first (at least one), untimed
            warming = warm == 0 or (time.perf_counter() - t_start) * 1e3 < a.min_warmup_ms
            if warming and rep == 0:
                warm += 1
            else:
                rep += 1
            for name, (fn, _) in cases.items():
                if name == "absorb":
                    with torch.cuda.stream(stream):
                        state.copy_(iv)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.inner):       # (absorb goes on from the state before: same work)
                    fn()
                e1.record(stream)
                e1.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1) / a.inner)
        warmup_reps = warm
        with torch.cuda.stream(stream):        # one absorb from the initial value, for the check
            state.copy_(iv)
        absorb()
        eng.device_status()
        # what was timed computed the right thing: finish the absorbed states (no bytes
        # left, prefix 512) and compare both with hashlib on a sample
        fin = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        off_end, none_left = off + msg, torch.zeros_like(length)
        torch.cuda.synchronize()
        eng.finish_device(state, length, arena, off_end, none_left, fin, stream=stream)
        eng.device_status()
    sample = [0, 1, 63, 64, n // 2, n - 1]
    host = arena.cpu().numpy().tobytes()
    for i in sample:
        exp = hashlib.sha256(host[i * msg:(i + 1) * msg]).digest()
        assert bytes(out[i].cpu().numpy()) == exp, ("lane", i)
        assert bytes(fin[i].cpu().numpy()) == exp, ("absorb + finish", i)

    lines, summary = [], {}
    for name, (_, blocks) in cases.items():
        per = [t * 1e6 / (n * blocks) for t in times[name]]
        med = statistics.median(per)
        summary[name] = (med, (max(per) - min(per)) / med)
        lines.append({"case": name, "lanes": n, "blocks_per_lane": blocks, "reps": a.reps, "inner": a.inner, "warmup_reps": warmup_reps,
                      "kernel_ms": [round(t, 4) for t in times[name]],
                      "ns_per_lane_block": [round(p, 5) for p in per], "median_ns_per_lane_block": round(med, 5),
                      "spread": round(summary[name][1], 4), "build": build["id"]})
    (ma, sa), (ml, sl) = summary["absorb"], summary["lane"]
    tol = max(sa, sl)
    lines.append({"case": "verdict", "absorb_over_lane": round(ma / ml, 4), "allowed": round(1 + tol, 4),
                  "absorb_no_worse_than_lane": bool(ma <= ml * (1 + tol))})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
