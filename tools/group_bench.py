#!/usr/bin/env python3
"""What msha_group_digests_device costs, against the two ways a caller has without it.

    python3 tools/group_bench.py [--reps 9] [--sizes N ...] [--out profiles/group/group_bench.jsonl]

For n = 2^20 and 2^24 digests in four group shapes -- all distinct, n / 16 groups of 16 (a
quorum tally), 100 groups (the storm) and one group -- these entries alternate in one
process (warm-up repetitions for 300 ms so the clock settles, then `reps` timed ones, entry
after entry within each repetition):
  kernels   (a) the call's six kernels by HIP events: msha_group_stats.last_kernel_ms under
            MSHA_PARTS_TIMING=1, group_cap 1024
  upto1..5  the first k kernels alone (MSHA_GROUP_STOP_AFTER=k), the same way: init; +
            insert; + resolve; + scan; + rank. A kernel's share is the difference of two
            medians (the `share` lines)
  call      (b) the call as a caller sees it: enqueue, wait for the stream, read the
            40-byte result (host clock)
  torch     (c) torch.unique(rows, dim=0, return_inverse=True, return_counts=True), wait
            included (host clock)
  download  (d) today's way: the 32 n bytes copied into pinned memory, then the map built
            on the host, np.unique over the rows with index, inverse and counts (host
            clock; `d2h` is the copy's share). `--host-reps` repetitions where n is above
            2^22: one build takes seconds there
Prints one JSON line an entry (ms of every repetition, the median, (max - min) / median),
one line a ratio (median over median, with both spreads) and the clock msha_clock_probe
finds before and after each size. Every entry's answer is compared with how the rows were
drawn, once, outside the timed window. A measurement, not a threshold. Needs the GPU; no
fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP_CAP = 1024
KERNELS = ("init", "insert", "resolve", "scan", "rank", "fill")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group", "group_bench.jsonl"),
                    help="the JSON lines are written to this file too ('' for none)")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    import torch
    from mirbft_amd import Engine, _lib
    build = _lib.require_tree_build("group_bench")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def summary(ms):
        med = statistics.median(ms)
        return {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4),
                "spread": round((max(ms) - min(ms)) / med, 3) if med else 0.0}

    emit({"bench": "group_bench", "build": build["id"], "reps": a.reps, "group_cap": GROUP_CAP,
          "device": torch.cuda.get_device_name(0)})
    side = torch.cuda.Stream()
    with Engine(1) as eng:
        for n in a.sizes:
            clk = eng.clock_probe()
            emit({"n": n, "clock": "before", "ghz_median": round(clk["ghz_median"], 3),
                  "ghz_min": round(clk["ghz_min"], 3), "ghz_max": round(clk["ghz_max"], 3)})
            gen = torch.Generator(device=dev)
            gen.manual_seed(0x62B ^ n)
            first, group, members = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
            group_first, group_count = (torch.empty(GROUP_CAP, dtype=torch.int32, device=dev) for _ in range(2))
            result = torch.empty(5, dtype=torch.int64, device=dev)
            pinned = torch.empty((n, 32), dtype=torch.uint8, pin_memory=True)
            host_reps = a.reps if n <= 1 << 22 else a.host_reps
            slot = torch.arange(n, device=dev)
            for shape, g in (("distinct", n), ("quorum16", n // 16), ("storm100", 100), ("one", 1)):
                # which value a slot holds: n / g slots a value (to within one), in a random order
                assign = (torch.randperm(n, device=dev, generator=gen) % g) if g > 1 else torch.zeros(
                    n, dtype=torch.int64, device=dev)
                pool = torch.randint(0, 256, (g, 32), dtype=torch.uint8, device=dev, generator=gen)
                rows = pool[assign].contiguous()
                del pool
                # what the call has to say, from how the rows were drawn (random 32-byte values: distinct)
                leader = torch.full((g,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, assign, slot, "amin")
                want_first = leader[assign].to(torch.int32)
                number = torch.empty(g, dtype=torch.int64, device=dev)
                number[torch.argsort(leader)] = torch.arange(g, device=dev)
                want_group = number[assign].to(torch.int32)
                sizes = torch.bincount(assign, minlength=g)
                want_members = sizes[assign].to(torch.int32)
                want_max = int(sizes.max())
                torch.cuda.synchronize()

                def call(stop=None, timing=True):
                    if timing:
                        os.environ["MSHA_PARTS_TIMING"] = "1"
                    if stop:
                        os.environ["MSHA_GROUP_STOP_AFTER"] = str(stop)
                    try:
                        eng.group_digests_device(rows.view(-1), first, group, result, members=members,
                                                 group_first=group_first, group_count=group_count, stream=side)
                    finally:
                        os.environ.pop("MSHA_PARTS_TIMING", None)
                        os.environ.pop("MSHA_GROUP_STOP_AFTER", None)
                    return eng.group_stats()["last_kernel_ms"]

                def e_call():
                    t0 = time.perf_counter()
                    eng.group_digests_device(rows.view(-1), first, group, result, members=members,
                                             group_first=group_first, group_count=group_count, stream=side)
                    side.synchronize()
                    r = result.cpu().tolist()
                    return (time.perf_counter() - t0) * 1e3, r

                def e_torch():
                    t0 = time.perf_counter()
                    u = torch.unique(rows, dim=0, return_inverse=True, return_counts=True)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3, u

                d2h = []

                def e_download():
                    t0 = time.perf_counter()
                    pinned.copy_(rows, non_blocking=True)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    keys = pinned.numpy().view(np.dtype((np.void, 32))).reshape(-1)
                    u = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
                    t2 = time.perf_counter()
                    d2h.append((t1 - t0) * 1e3)
                    return (t2 - t0) * 1e3, u

                # every answer against how the rows were drawn, once
                _, r = e_call()
                by_number = sizes[torch.argsort(leader)]
                want_max_group = int((by_number == want_max).nonzero()[0])
                assert r == [n, g, min(g, GROUP_CAP), want_max, want_max_group], r
                assert torch.equal(first, want_first) and torch.equal(group, want_group)
                assert torch.equal(members, want_members)
                listed = r[2]
                assert torch.equal(group_first[:listed].long(), torch.sort(leader).values[:listed])
                u = e_torch()[1]
                assert u[0].shape[0] == g and torch.equal(u[2][u[1].view(-1)], sizes[assign])
                del u
                hu = e_download()[1]
                assert hu[0].size == g and np.array_equal(hu[1][hu[2].reshape(-1)], want_first.cpu().numpy())
                del hu

                entries = {"kernels": lambda: call()}
                for k in range(1, len(KERNELS)):
                    entries["upto%d" % k] = (lambda k: lambda: call(stop=k))(k)
                entries["call"] = lambda: e_call()[0]
                entries["torch"] = lambda: e_torch()[0]
                entries["download"] = lambda: e_download()[0]
                t_end = time.perf_counter() + a.min_warmup_ms / 1e3
                while time.perf_counter() < t_end:
                    for name in ("kernels", "call"):
                        entries[name]()
                entries["torch"]()
                del d2h[:]
                ms = {name: [] for name in entries}
                for rep in range(a.reps):
                    for name, f in entries.items():
                        if name == "download" and rep >= host_reps:
                            continue
                        ms[name].append(f())
                ms["d2h"] = list(d2h)
                s = {name: summary(v) for name, v in ms.items()}
                for name, v in s.items():
                    emit(dict({"n": n, "shape": shape, "groups": g, "entry": name, "reps": len(ms[name])}, **v))
                upto = [0.0] + [s["upto%d" % k]["median_ms"] for k in range(1, len(KERNELS))] + [s["kernels"]["median_ms"]]
                emit({"n": n, "shape": shape, "share": {KERNELS[k]: round(upto[k + 1] - upto[k], 4)
                                                        for k in range(len(KERNELS))},
                      "of_ms": s["kernels"]["median_ms"]})
                for num, den in (("kernels", "torch"), ("kernels", "download"), ("call", "torch"), ("call", "download")):
                    emit({"n": n, "shape": shape, "ratio": "%s / %s" % (num, den),
                          "value": round(s[num]["median_ms"] / s[den]["median_ms"], 4),
                          "spreads": [s[num]["spread"], s[den]["spread"]]})
                del rows, assign, leader, want_first, want_group, want_members, number, sizes
                torch.cuda.empty_cache()
            clk = eng.clock_probe()
            emit({"n": n, "clock": "after", "ghz_median": round(clk["ghz_median"], 3),
                  "ghz_min": round(clk["ghz_min"], 3), "ghz_max": round(clk["ghz_max"], 3)})
            del first, group, members, pinned, slot
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
