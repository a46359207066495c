#!/usr/bin/env python3
"""What msha_verify_digests_device costs, against the two ways a caller has without it.

    python3 tools/verify_bench.py [--reps 9] [--out profiles/verify/verify_bench.jsonl]

For n = 2^20 and 2^24 digests with 0, 1 and 1 % of them differing, these entries alternate
in one process (warm-up repetitions for 300 ms so the clock settles, then `reps` timed
ones, entry after entry within each repetition):
  kernels   (a) the call's two kernels by HIP events: msha_verify_stats.last_kernel_ms
            under MSHA_PARTS_TIMING=1, list_cap 1024
  compare   k_verify_compare alone (MSHA_VERIFY_ONLY=1), the same way
  scan      k_verify_scan alone (MSHA_VERIFY_ONLY=2) over the mask the compare left
  call      the call as a caller sees it: enqueue, wait for the stream, read the 40-byte
            result (host clock)
  download  (b) today's way: the 32 n bytes copied into pinned memory, then numpy
            (got != expected).any(1) and flatnonzero on the host (host clock; `d2h` is the
            copy's share)
  torch     (c) (got != expected).any(1).nonzero() on the device, wait included (host clock)
Prints one JSON line an entry (ms of every repetition, the median, (max - min) / median),
one line a ratio (median over median, with both spreads) and the clock msha_clock_probe
finds before and after each size. Every entry's answer is compared with the flips that
were made, once, outside the timed window. A measurement, not a threshold. Needs the GPU;
no fallback.
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

LIST_CAP = 1024


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify", "verify_bench.jsonl"),
                    help="the JSON lines are written to this file too (replacing it; '' for none)")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    import torch
    from mirbft_amd import Engine, _lib
    build = _lib.require_tree_build("verify_bench")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def summary(ms):
        med = statistics.median(ms)
        return {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4),
                "spread": round((max(ms) - min(ms)) / med, 3) if med else 0.0}

    emit({"bench": "verify_bench", "build": build["id"], "reps": a.reps, "list_cap": LIST_CAP,
          "device": torch.cuda.get_device_name(0)})
    side = torch.cuda.Stream()
    with Engine(1) as eng:
        for n in a.sizes:
            clk = eng.clock_probe()
            emit({"n": n, "clock": "before", "ghz_median": round(clk["ghz_median"], 3),
                  "ghz_min": round(clk["ghz_min"], 3), "ghz_max": round(clk["ghz_max"], 3)})
            rng = np.random.default_rng(0xBE7C ^ n)
            got = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev)
            mask = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
            result = torch.empty(5, dtype=torch.int64, device=dev)
            bad_list = torch.empty(LIST_CAP, dtype=torch.int32, device=dev)
            pinned = torch.empty((n, 32), dtype=torch.uint8, pin_memory=True)
            for pattern, count in (("none", 0), ("one", 1), ("1pct", n // 100)):
                slots = np.sort(rng.choice(n, count, replace=False)) if count else np.zeros(0, dtype=np.int64)
                expected = got.clone()
                if count:
                    where = torch.from_numpy(slots).to(dev)
                    col = torch.from_numpy(rng.integers(0, 32, count)).to(dev)
                    expected[where, col] = expected[where, col] ^ 0x40
                exp_host = expected.cpu().numpy()
                torch.cuda.synchronize()

                def call(only=None, timing=True):
                    if timing:
                        os.environ["MSHA_PARTS_TIMING"] = "1"
                    if only:
                        os.environ["MSHA_VERIFY_ONLY"] = str(only)
                    try:
                        eng.verify_digests_device(got.view(-1), expected.view(-1), mask, result, bad_list=bad_list,
                                                  stream=side)
                    finally:
                        os.environ.pop("MSHA_PARTS_TIMING", None)
                        os.environ.pop("MSHA_VERIFY_ONLY", None)
                    return eng.verify_stats()["last_kernel_ms"]

                def e_call():
                    t0 = time.perf_counter()
                    eng.verify_digests_device(got.view(-1), expected.view(-1), mask, result, bad_list=bad_list,
                                              stream=side)
                    side.synchronize()
                    r = result.cpu().tolist()
                    return (time.perf_counter() - t0) * 1e3, r[1]

                d2h = []

                def e_download():
                    t0 = time.perf_counter()
                    pinned.copy_(got, non_blocking=True)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    bad = np.flatnonzero((pinned.numpy() != exp_host).any(axis=1))
                    t2 = time.perf_counter()
                    d2h.append((t1 - t0) * 1e3)
                    return (t2 - t0) * 1e3, bad

                def e_torch():
                    t0 = time.perf_counter()
                    bad = (got != expected).any(1).nonzero()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3, bad

                # every answer against the flips, once
                call(timing=False)
                side.synchronize()
                r = result.cpu().tolist()
                assert r[:2] == [n, count] and r[3] == min(count, LIST_CAP), r
                assert bad_list[:r[3]].cpu().tolist() == slots[:r[3]].tolist()
                assert np.array_equal(e_download()[1], slots)
                assert np.array_equal(e_torch()[1].view(-1).cpu().numpy(), slots)
                assert e_call()[1] == count

                entries = {"kernels": lambda: call(), "compare": lambda: call(only=1), "scan": lambda: call(only=2),
                           "call": lambda: e_call()[0], "download": lambda: e_download()[0],
                           "torch": lambda: e_torch()[0]}
                t_end = time.perf_counter() + a.min_warmup_ms / 1e3
                while time.perf_counter() < t_end:
                    for name in ("kernels", "call", "torch"):
                        entries[name]()
                entries["download"]()
                del d2h[:]
                ms = {name: [] for name in entries}
                for _ in range(a.reps):
                    for name, f in entries.items():
                        if name == "scan":
                            call(only=1, timing=False)      # the mask the scan walks is this pattern's
                        ms[name].append(f())
                ms["d2h"] = list(d2h)
                s = {name: summary(v) for name, v in ms.items()}
                for name, v in s.items():
                    emit(dict({"n": n, "pattern": pattern, "bad": count, "entry": name}, **v))
                for num, den in (("kernels", "download"), ("kernels", "torch"), ("call", "download"),
                                 ("call", "torch"), ("scan", "kernels")):
                    emit({"n": n, "pattern": pattern, "ratio": "%s / %s" % (num, den),
                          "value": round(s[num]["median_ms"] / s[den]["median_ms"], 4),
                          "spreads": [s[num]["spread"], s[den]["spread"]]})
                del expected
            clk = eng.clock_probe()
            emit({"n": n, "clock": "after", "ghz_median": round(clk["ghz_median"], 3),
                  "ghz_min": round(clk["ghz_min"], 3), "ghz_max": round(clk["ghz_max"], 3)})
            del got, mask, pinned
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
