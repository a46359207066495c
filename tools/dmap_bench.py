#!/usr/bin/env python3
"""What a device digest map gains a caller over what it had for the same stream of arrivals.

    python3 tools/dmap_bench.py [--reps 9] [--out profiles/dmap/dmap_bench.jsonl]

Three arrival streams, each a list of calls whose digests already lie in HBM:
  quorum    64 calls of 16,384 acks over 4,096 keys (256 votes a key; threshold 171, two thirds of them)
  distinct  one call of 2^20 digests over 2^20 distinct keys (the insert's worst case, and
            a single call on an empty map: group plus four launches, expected to lose)
  hot       64 calls of 16,384 acks of one key
For each stream these entries alternate in one process (warm-up repetitions for 300 ms so
the clock settles, then `reps` timed ones, entry after entry within each repetition); every
time is that of the WHOLE stream, on the host clock, ending in a wait:
  map       the map: clear, then per call add_device, wait for the stream, read the 64-byte
            result
  regroup   (a) without a map, in HBM: per call msha_group_digests_device over EVERYTHING
            seen so far (the calls are slices of one array, so nothing is copied), wait,
            read the 40-byte result
  download  (b) without a map, on the host: per call the call's 32 n bytes copied into pinned
            memory and counted into a Python dict keyed by the 32 bytes (`d2h` is the
            copies' share). `--host-reps` repetitions: one takes a second
And one more call of the stream's shape on the map as the stream left it (for `distinct`:
on an empty map), by HIP events (msha_dmap_stats.last_kernel_ms under MSHA_PARTS_TIMING=1):
  kernels   its seven kernels
  upto1..5  the first k kernels alone (MSHA_DMAP_STOP_AFTER=k). A kernel's share is the
            difference of two medians (the `share` lines); commit and fill are one share,
            since the library never runs commit without fill
Prints one JSON line an entry (ms of every repetition, the median, (max - min) / median),
one line a ratio (median over median, with both spreads) and the clock msha_clock_probe
finds before and after each stream. The map's final counts are compared with how the calls
were drawn, once, outside the timed window. A measurement, not a threshold. Needs the GPU;
no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARES = ("group_init", "group_insert", "group_resolve", "find", "scan", "commit_fill")
CROSSED_CAP = 1024


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--streams", nargs="+", default=["quorum", "distinct", "hot"])
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmap", "dmap_bench.jsonl"),
                    help="the JSON lines are written to this file too ('' for none)")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    import torch
    from mirbft_amd import Engine, GPUHasher, _lib
    build = _lib.require_tree_build("dmap_bench")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def summary(ms):
        med = statistics.median(ms)
        return {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4),
                "spread": round((max(ms) - min(ms)) / med, 3) if med else 0.0}

    shapes = {"quorum": (64, 1 << 14, 4096, 171), "distinct": (1, 1 << 20, 1 << 20, 1), "hot": (64, 1 << 14, 1, 2731)}
    emit({"bench": "dmap_bench", "build": build["id"], "reps": a.reps, "host_reps": a.host_reps,
          "crossed_cap": CROSSED_CAP, "device": torch.cuda.get_device_name(0)})
    side = torch.cuda.Stream()
    with Engine(1) as eng:
        hasher = GPUHasher(engine=eng)
        for name in a.streams:
            calls, per, keys, threshold = shapes[name]
            n = calls * per
            clk = eng.clock_probe()
            emit({"stream": name, "clock": "before", "ghz_median": round(clk["ghz_median"], 3),
                  "ghz_min": round(clk["ghz_min"], 3), "ghz_max": round(clk["ghz_max"], 3)})
            gen = torch.Generator(device=dev)
            gen.manual_seed(0xD3A9 ^ n ^ keys)
            pool = torch.randint(0, 256, (keys, 32), dtype=torch.uint8, device=dev, generator=gen)
            assign = (torch.randperm(n, device=dev, generator=gen) % keys) if keys > 1 else torch.zeros(
                n, dtype=torch.int64, device=dev)
            rows = pool[assign].contiguous()                      # [n, 32]: call c is rows[c * per : (c + 1) * per]
            flat = rows.view(-1)
            dmap = hasher.new_device_digest_map(keys)
            ids, before, after = (torch.empty(per, dtype=torch.int32, device=dev) for _ in range(3))
            crossed = torch.empty(CROSSED_CAP, dtype=torch.int32, device=dev)
            result = torch.empty(8, dtype=torch.int64, device=dev)
            g_first, g_group = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
            g_result = torch.empty(5, dtype=torch.int64, device=dev)
            pinned = torch.empty((per, 32), dtype=torch.uint8, pin_memory=True)
            torch.cuda.synchronize()

            def add(c):
                dmap.add_device(flat[32 * per * c:32 * per * (c + 1)], ids, result, threshold=threshold, before=before,
                                after=after, crossed_slots=crossed, stream=side)

            def e_map():
                t0 = time.perf_counter()
                dmap.clear_device(stream=side)
                crossings = 0
                for c in range(calls):
                    add(c)
                    side.synchronize()
                    crossings += result.cpu().tolist()[4]
                return (time.perf_counter() - t0) * 1e3, crossings

            def e_regroup():
                t0 = time.perf_counter()
                groups = 0
                for c in range(calls):
                    seen = per * (c + 1)
                    eng.group_digests_device(flat[:32 * seen], g_first[:seen], g_group[:seen], g_result, stream=side)
                    side.synchronize()
                    groups = g_result.cpu().tolist()[1]
                return (time.perf_counter() - t0) * 1e3, groups

            d2h = []

            def e_download():
                t0 = time.perf_counter()
                copies = 0.0
                tally = {}
                for c in range(calls):
                    t1 = time.perf_counter()
                    pinned.copy_(rows[per * c:per * (c + 1)], non_blocking=True)
                    torch.cuda.synchronize()
                    copies += time.perf_counter() - t1
                    raw = pinned.numpy().tobytes()
                    for i in range(0, len(raw), 32):
                        k = raw[i:i + 32]
                        tally[k] = tally.get(k, 0) + 1
                d2h.append(copies * 1e3)
                return (time.perf_counter() - t0) * 1e3, tally

            def one_more(stop=None):
                """One more call of the stream's shape, by HIP events. `distinct`: on an
                empty map, so what the whole call put in is cleared away first."""
                if name == "distinct":
                    dmap.clear_device(stream=side)
                os.environ["MSHA_PARTS_TIMING"] = "1"
                if stop:
                    os.environ["MSHA_DMAP_STOP_AFTER"] = str(stop)
                try:
                    add(calls - 1)
                finally:
                    os.environ.pop("MSHA_PARTS_TIMING", None)
                    os.environ.pop("MSHA_DMAP_STOP_AFTER", None)
                return dmap.stats()["last_kernel_ms"]

            # the answers against how the calls were drawn, once
            sizes = torch.bincount(assign, minlength=keys)
            _, crossings = e_map()
            assert dmap.size() == keys and crossings == int((sizes >= threshold).sum()), (dmap.size(), crossings)
            f_ids, f_count = (torch.empty(keys, dtype=torch.int32, device=dev) for _ in range(2))
            dmap.find_device(pool.view(-1), f_ids, count=f_count, stream=side)
            side.synchronize()
            assert torch.equal(f_count.long(), sizes) and torch.equal(torch.sort(f_ids.long()).values,
                                                                      torch.arange(keys, device=dev))
            assert e_regroup()[1] == keys
            tally = e_download()[1]
            assert len(tally) == keys and sorted(tally.values()) == sorted(sizes.cpu().tolist())
            del tally

            entries = {"map": lambda: e_map()[0], "regroup": lambda: e_regroup()[0], "download": lambda: e_download()[0]}
            t_end = time.perf_counter() + a.min_warmup_ms / 1e3
            while time.perf_counter() < t_end:
                entries["map"]()
                entries["regroup"]()
            del d2h[:]
            ms = {k: [] for k in entries}
            for rep in range(a.reps):
                for k, f in entries.items():
                    if k == "download" and rep >= a.host_reps:
                        continue
                    ms[k].append(f())
            ms["d2h"] = list(d2h)
            # one more call on the map as the last e_map() left it
            probes = {"kernels": lambda: one_more()}
            for k in range(1, len(SHARES)):
                probes["upto%d" % k] = (lambda k: lambda: one_more(stop=k))(k)
            for f in probes.values():
                f()
            for k in probes:
                ms[k] = []
            for rep in range(a.reps):
                for k, f in probes.items():
                    ms[k].append(f())
            if name == "distinct":
                dmap.clear_device(stream=side)
            s = {k: summary(v) for k, v in ms.items()}
            for k, v in s.items():
                emit(dict({"stream": name, "calls": calls, "per_call": per, "keys": keys, "entry": k,
                           "reps": len(ms[k])}, **v))
            upto = [0.0] + [s["upto%d" % k]["median_ms"] for k in range(1, len(SHARES))] + [s["kernels"]["median_ms"]]
            emit({"stream": name, "share": {SHARES[k]: round(upto[k + 1] - upto[k], 4) for k in range(len(SHARES))},
                  "of_ms": s["kernels"]["median_ms"]})
            for num, den in (("map", "regroup"), ("map", "download")):
                emit({"stream": name, "ratio": "%s / %s" % (num, den),
                      "value": round(s[num]["median_ms"] / s[den]["median_ms"], 4),
                      "spreads": [s[num]["spread"], s[den]["spread"]]})
            clk = eng.clock_probe()
            emit({"stream": name, "clock": "after", "ghz_median": round(clk["ghz_median"], 3),
                  "ghz_min": round(clk["ghz_min"], 3), "ghz_max": round(clk["ghz_max"], 3)})
            dmap.close()
            del pool, assign, rows, flat, ids, before, after, g_first, g_group, pinned, sizes
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
