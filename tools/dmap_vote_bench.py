#!/usr/bin/env python3
"""What counting each voter once costs a device digest map, and what it saves a caller.

    python3 tools/dmap_vote_bench.py [--reps 9] [--out profiles/dmap_vote/dmap_vote_bench.jsonl]

The arrival streams of tools/dmap_bench.py (quorum: 64 calls of 16,384 acks over 4,096 keys;
distinct: one call of 2^20 digests over 2^20 keys; hot: 64 calls of 16,384 acks of one key),
each with a voter a slot drawn from 4, 16 and 128 nodes, a tenth of the slots then made an
exact repeat of another slot's (key, voter). The digests and voters already lie in HBM.
For each stream and node count these entries alternate in one process (warm-up repetitions
for 300 ms, then `reps` timed ones, entry after entry within each repetition); every time is
that of the WHOLE stream, on the host clock, ending in a wait:
  vote      a vote map: clear, then per call vote_device, wait, read the 88-byte result
  add       (1) a plain map over the same slots: clear, per call add_device, wait, read the
            64-byte result. That code counts slots; the difference is what deduplication costs
  download  (2) what a caller has without a vote map: per call the digests and voters copied
            into pinned memory and entered into a Python dict of sets (`d2h`: the copies'
            share). `--host-reps` repetitions
And one more call of the stream's shape on the maps as the stream left them (`distinct`: on
empty maps), by HIP events (last_kernel_ms under MSHA_PARTS_TIMING=1):
  vote_kernels   the vote's ten kernels        add_kernels   the add's seven
  upto1..8       the vote's first k kernels alone (MSHA_DMAP_VOTE_STOP_AFTER=k); a kernel's
                 share is the difference of two medians, commit and fill one share
Prints one JSON line an entry (ms of every repetition, the median, (max - min) / median),
the shares, the ratios, the repeats the vote map reported and the clock msha_clock_probe finds
before and after. The vote map's final counts are compared with the host's dict of sets,
once, outside the timed window. A measurement, not a threshold. Needs the GPU; no fallback.
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

SHARES = ("group_init", "group_insert", "group_resolve", "find", "pair", "count", "totals", "scan", "commit_fill")
CROSSED_CAP = 1024


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--streams", nargs="+", default=["quorum", "distinct", "hot"])
    ap.add_argument("--nodes", nargs="+", type=int, default=[4, 16, 128])
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmap_vote", "dmap_vote_bench.jsonl"),
                    help="the JSON lines are written to this file too ('' for none)")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    import torch
    from mirbft_amd import Engine, GPUHasher, _lib
    build = _lib.require_tree_build("dmap_vote_bench")
    dev = torch.device("cuda:0")
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def summary(ms):
        med = statistics.median(ms)
        return {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4),
                "spread": round((max(ms) - min(ms)) / med, 3) if med else 0.0}

    shapes = {"quorum": (64, 1 << 14, 4096), "distinct": (1, 1 << 20, 1 << 20), "hot": (64, 1 << 14, 1)}
    emit({"bench": "dmap_vote_bench", "build": build["id"], "reps": a.reps, "host_reps": a.host_reps,
          "crossed_cap": CROSSED_CAP, "device": torch.cuda.get_device_name(0)})
    side = torch.cuda.Stream()
    with Engine(1) as eng:
        hasher = GPUHasher(engine=eng)
        for name in a.streams:
            calls, per, keys = shapes[name]
            n = calls * per
            for nodes in a.nodes:
                tag = {"stream": name, "nodes": nodes}
                clk = eng.clock_probe()
                emit(dict(tag, clock="before", ghz_median=round(clk["ghz_median"], 3), ghz_min=round(clk["ghz_min"], 3),
                          ghz_max=round(clk["ghz_max"], 3)))
                threshold = 2 * nodes // 3 + 1
                gen = torch.Generator(device=dev)
                gen.manual_seed(0x707E ^ n ^ keys ^ nodes)
                pool = torch.randint(0, 256, (keys, 32), dtype=torch.uint8, device=dev, generator=gen)
                assign = (torch.randperm(n, device=dev, generator=gen) % keys) if keys > 1 else torch.zeros(
                    n, dtype=torch.int64, device=dev)
                voter = torch.randint(0, nodes, (n,), dtype=torch.int64, device=dev, generator=gen)
                # a tenth of the slots repeat another slot's (key, voter) exactly
                again = torch.randperm(n, device=dev, generator=gen)[:n // 10]
                src = torch.randint(0, n, (again.numel(),), dtype=torch.int64, device=dev, generator=gen)
                assign[again], voter[again] = assign[src], voter[src]
                rows = pool[assign].contiguous()                  # [n, 32]: call c is rows[c * per : (c + 1) * per]
                flat = rows.view(-1)
                voter32 = voter.to(torch.int32).contiguous()
                vmap = hasher.new_device_vote_map(keys, nodes)
                pmap = hasher.new_device_digest_map(keys)
                ids, counted, before, after = (torch.empty(per, dtype=torch.int32, device=dev) for _ in range(4))
                crossed = torch.empty(CROSSED_CAP, dtype=torch.int32, device=dev)
                v_result = torch.empty(11, dtype=torch.int64, device=dev)
                p_result = torch.empty(8, dtype=torch.int64, device=dev)
                pinned = torch.empty((per, 32), dtype=torch.uint8, pin_memory=True)
                pinned_v = torch.empty(per, dtype=torch.int32, pin_memory=True)
                torch.cuda.synchronize()

                def vote(c):
                    vmap.vote_device(flat[32 * per * c:32 * per * (c + 1)], voter32[per * c:per * (c + 1)], ids, v_result,
                                     threshold=threshold, counted=counted, before=before, after=after, crossed_slots=crossed,
                                     stream=side)

                def add(c):
                    pmap.add_device(flat[32 * per * c:32 * per * (c + 1)], ids, p_result, threshold=threshold, before=before,
                                    after=after, crossed_slots=crossed, stream=side)

                def e_vote():
                    t0 = time.perf_counter()
                    vmap.clear_device(stream=side)
                    repeats = 0
                    for c in range(calls):
                        vote(c)
                        side.synchronize()
                        repeats += v_result.cpu().tolist()[9]
                    return (time.perf_counter() - t0) * 1e3, repeats

                def e_add():
                    t0 = time.perf_counter()
                    pmap.clear_device(stream=side)
                    crossings = 0
                    for c in range(calls):
                        add(c)
                        side.synchronize()
                        crossings += p_result.cpu().tolist()[4]
                    return (time.perf_counter() - t0) * 1e3, crossings

                d2h = []

                def e_download():
                    t0 = time.perf_counter()
                    copies = 0.0
                    tally = {}
                    for c in range(calls):
                        t1 = time.perf_counter()
                        pinned.copy_(rows[per * c:per * (c + 1)], non_blocking=True)
                        pinned_v.copy_(voter32[per * c:per * (c + 1)], non_blocking=True)
                        torch.cuda.synchronize()
                        copies += time.perf_counter() - t1
                        raw = pinned.numpy().tobytes()
                        senders = pinned_v.tolist()
                        for i, v in enumerate(senders):
                            k = raw[32 * i:32 * i + 32]
                            s = tally.get(k)
                            if s is None:
                                tally[k] = {v}
                            else:
                                s.add(v)
                    d2h.append(copies * 1e3)
                    return (time.perf_counter() - t0) * 1e3, tally

                def one_more(which, stop=None):
                    """One more call of the stream's shape, by HIP events. `distinct`: on an
                    empty map, so what the whole call put in is cleared away first."""
                    m = vmap if which == "vote" else pmap
                    if name == "distinct":
                        m.clear_device(stream=side)
                    os.environ["MSHA_PARTS_TIMING"] = "1"
                    if stop:
                        os.environ["MSHA_DMAP_VOTE_STOP_AFTER"] = str(stop)
                    try:
                        (vote if which == "vote" else add)(calls - 1)
                    finally:
                        os.environ.pop("MSHA_PARTS_TIMING", None)
                        os.environ.pop("MSHA_DMAP_VOTE_STOP_AFTER", None)
                    return (m.vote_stats() if which == "vote" else m.stats())["last_kernel_ms"]

                # the answers against the host's dict of sets, once
                _, repeats = e_vote()
                tally = e_download()[1]
                distinct_pairs = sum(len(s) for s in tally.values())
                held = len(tally)                                 # at most `keys`: a repeat may have replaced a key's only slot
                assert vmap.size() == held and repeats == n - distinct_pairs, (vmap.size(), held, repeats)
                count = vmap.read()[2]
                assert sorted(count.tolist()) == sorted(len(s) for s in tally.values())
                masks = vmap.read_voters()
                assert np.array_equal(np.unpackbits(masks.view(np.uint8), axis=1).sum(axis=1), count)
                e_add()
                assert pmap.size() == held
                del tally, masks
                emit(dict(tag, slots=n, keys_held=held, distinct_pairs=distinct_pairs, repeats=repeats, repeat_fraction=round(repeats / n, 4),
                          threshold=threshold))

                entries = {"vote": lambda: e_vote()[0], "add": lambda: e_add()[0], "download": lambda: e_download()[0]}
                t_end = time.perf_counter() + a.min_warmup_ms / 1e3
                while time.perf_counter() < t_end:
                    entries["vote"]()
                    entries["add"]()
                del d2h[:]
                ms = {k: [] for k in entries}
                for rep in range(a.reps):
                    for k, f in entries.items():
                        if k == "download" and rep >= a.host_reps:
                            continue
                        ms[k].append(f())
                ms["d2h"] = list(d2h)
                # one more call on the maps as the last e_vote() and e_add() left them
                probes = {"vote_kernels": lambda: one_more("vote"), "add_kernels": lambda: one_more("add")}
                for k in range(1, len(SHARES)):
                    probes["upto%d" % k] = (lambda k: lambda: one_more("vote", stop=k))(k)
                for f in probes.values():
                    f()
                for k in probes:
                    ms[k] = []
                for rep in range(a.reps):
                    for k, f in probes.items():
                        ms[k].append(f())
                s = {k: summary(v) for k, v in ms.items()}
                for k, v in s.items():
                    emit(dict(tag, calls=calls, per_call=per, keys=keys, entry=k, reps=len(ms[k]), **v))
                upto = [0.0] + [s["upto%d" % k]["median_ms"] for k in range(1, len(SHARES))] + [s["vote_kernels"]["median_ms"]]
                emit(dict(tag, share={SHARES[k]: round(upto[k + 1] - upto[k], 4) for k in range(len(SHARES))},
                          of_ms=s["vote_kernels"]["median_ms"]))
                for num, den in (("vote", "add"), ("vote", "download"), ("vote_kernels", "add_kernels")):
                    emit(dict(tag, ratio="%s / %s" % (num, den), value=round(s[num]["median_ms"] / s[den]["median_ms"], 4),
                              spreads=[s[num]["spread"], s[den]["spread"]]))
                clk = eng.clock_probe()
                emit(dict(tag, clock="after", ghz_median=round(clk["ghz_median"], 3), ghz_min=round(clk["ghz_min"], 3),
                          ghz_max=round(clk["ghz_max"], 3)))
                vmap.close()
                pmap.close()
                del pool, assign, voter, voter32, rows, flat, ids, counted, before, after, pinned, pinned_v
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
