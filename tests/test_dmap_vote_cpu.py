"""The rules of the vote maps (mirbft_amd/csrc/dmap_vote.hpp) under AddressSanitizer +
UBSan, as a stand-alone program with its own main (tests/cpp/dmap_vote_check.cpp) over the
sequences the GPU test runs (tests/dmap_vote_matrix.py; all but the one that is too long
for a sanitizer run), both inserts in three slot orders, its results compared with the
dict-of-sets oracle; the sequences proven to cover what they claim; and the oracle's
comparison shown to reject wrong results. Host code only: nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import dmap_matrix as M
import dmap_vote_matrix as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _by_name():
    seqs = V.all_sequences()
    names = [s.name for s in seqs]
    assert len(set(names)) == len(names)
    return {s.name: s for s in seqs}


def _bits(mask_row):
    return sorted(32 * w + b for w, word in enumerate(mask_row) for b in range(32) if int(word) >> b & 1)


def test_sequences_cover_what_they_claim():
    S = _by_name()
    T = V.TILE
    assert V.launches() == 10 and M.launches() == 7 and V.sizes() == [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    # one call on an empty map
    for n in V.sizes():
        p = V.patterns(n)
        assert set(p) == {"distinct", "equal", "random"}
        val, voter = p["distinct"]
        assert len(set(zip(val.tolist(), voter.tolist()))) == n                      # every pair once
        assert np.unique(p["equal"][0]).size == 1 and np.unique(p["equal"][1]).size == 1
        assert p["random"][0].max() < max(1, n // 4) and p["random"][1].max() < 4
        for name in p:
            s = S["one_%d_%s" % (n, name)]
            first, found = V.run_oracle(s)
            assert first["result"][:4] == (n, s.max_keys, s.max_keys, 0) and s.steps[0].threshold == 2
            assert (found["voted"] == 1).all()
        r = V.run_oracle(S["one_%d_equal" % n])[0]
        assert r["counted"].tolist() == [1] + [0] * (n - 1) and r["result"][8:] == (1, n - 1, 0)
        r = V.run_oracle(S["one_%d_distinct" % n])[0]
        assert (r["counted"] == 1).all() and r["result"][8:] == (n, 0, 0) and int(r["after"].max()) == min(n, 4)
    big = S["big_exact_fit"]
    assert big.big and big.max_keys == big.steps[0].n == 65537 and -(-65537 // T) > 256      # a second scan chunk
    # mask word edges
    assert V.MASK_EDGES == (1, 31, 32, 33, 64, 65, 1024)
    for mv in V.MASK_EDGES:
        s = S["mask_edges_%d" % mv]
        a, b, c, f = V.run_oracle(s)
        good = sorted({v for v in V.EDGE_VOTERS + (mv - 1,) if v < mv})
        assert s.max_voters == mv and _bits(a["state"][3][0]) == good and a["state"][3].shape[1] == V.words(mv)
        assert a["result"][10] == sum(v >= mv for v in V.EDGE_VOTERS + (mv - 1,))
        assert all(_bits(row) == good for row in c["state"][3]) and c["result"][1] == 4
        assert c["result"][9] > 0 and (f["voted"] == (np.tile(np.array(V.EDGE_VOTERS + (mv - 1,)), 4) < mv)).all()
    two = V.run_oracle(S["mask_edges_65"])[0]["state"][3][0]
    assert int(two[0]) == 1 | 1 << 31 and int(two[1]) == 1 | 1 << 31 and int(two[2]) == 1    # one word twice, and three words
    # the smallest slot wins, wherever the two lie, in either order
    for name, (a, b) in V.DUPLICATES.items():
        assert {"wave": a // 64 == b // 64, "waves": a // 64 != b // 64 and a // T == b // T, "tiles": a // T != b // T,
                "leader_third": len({5 // T, a // T, b // T}) == 3}[name]
        r = V.run_oracle(S["dup_" + name])[0]
        assert r["counted"][a] == 1 and r["counted"][b] == 0 and r["result"][8:] == (599, 1, 0)
        r = V.run_oracle(S["dup_" + name + "_reversed"])[0]
        assert r["counted"][599 - b] == 1 and r["counted"][599 - a] == 0 and 599 - b < 599 - a
    # across calls
    a, b, c = V.run_oracle(S["repeat_later"])
    assert b["counted"].tolist() == [0, 1, 0] and c["counted"].tolist() == [0, 1] and c["after"].tolist() == [2, 3]
    votes, plain = V.run_oracle(S["third_voter"]), M.run_oracle(V.third_voter_plain())
    for x, y in zip(S["third_voter"].steps, V.third_voter_plain().steps):
        assert np.array_equal(x.val, y.val) and x.threshold == y.threshold == 3          # the same slots
    assert [r["result"][4] for r in votes] == [0, 0, 1] and [r["result"][4] for r in plain] == [0, 1, 0]
    assert votes[2]["crossed"][0] == 0 and votes[2]["before"][0] == 2 and votes[2]["after"][0] == 3
    r = V.run_oracle(S["crossing"])
    assert r[0]["result"][4:6] == (2, 2) and r[0]["crossed"][:2].tolist() == [0, 3]          # once a key, at its leader
    assert r[1]["result"][4:6] == (1, 1) and r[1]["crossed"][0] == 0
    assert r[2]["result"][4] == 0 and S["crossing"].steps[2].threshold == 0
    assert S["crossing"].steps[3].crossed_cap == 0 and r[3]["result"][4:6] == (1, 0) and r[3]["result"][8:] == (1, 1, 0)
    assert r[4]["result"][4:6] == (0, 0) and r[4]["result"][8:] == (0, 1, 0)
    r = V.run_oracle(S["crossing_cap"])
    assert r[0]["result"][4:6] == (5, 2) and r[0]["crossed"].tolist() == [0, 3]
    assert r[1]["result"][4:6] == (5, 5) and r[1]["crossed"].tolist() == [0, 3, 6, 9, 12]
    # voters out of range
    for mv in (5, 33):
        a, b, f = V.run_oracle(S["bad_voters_%d" % mv])
        assert a["result"] == (2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 2) and a["state"][2].tolist() == [0, 0]
        assert not a["state"][3].any() and b["counted"].tolist() == [1, 0, 1, 0, 0] and b["result"][8:] == (2, 0, 3)
        assert b["state"][2].tolist() == [1, 0, 1] and _bits(b["state"][3][0]) == [mv - 1] and f["voted"].tolist() == [1, 0, 1, 0]
    # full: all or nothing, the per-slot facts still reported
    r = V.run_oracle(S["full"])
    assert r[0]["result"][:4] == (4, 3, 3, 0)
    assert r[1]["result"] == (5, 3, 2, 1, 0, 0, 0, 0, 3, 2, 0) and (r[1]["ids"] == V.NO_ID).all()
    assert r[1]["counted"].tolist() == [1, 1, 1, 0, 0] and r[1]["before"].tolist() == [0, 1, 0, 1, 2]
    assert r[1]["after"].tolist() == [1, 2, 1, 2, 2]
    assert all(np.array_equal(x, y) for x, y in zip(r[0]["state"], r[1]["state"]))
    assert r[3]["ids"].tolist() == [3, 1] and r[3]["result"][:4] == (2, 4, 1, 0)             # fits exactly
    assert r[4]["result"][:4] == (1, 4, 1, 1) and r[5]["result"][:4] == (3, 4, 0, 0) and r[5]["result"][8:] == (1, 2, 0)
    # the chains
    cap = V.capacity(V.PAIR_N)
    assert [S["pair_chain_%d" % h].pair_home for h in (0, cap - 1)] == [0, cap - 1] and cap == 256
    a, b = V.run_oracle(S["pair_chain_0"])
    assert a["result"][8:] == (35, 35, 0) and (a["state"][2] == 5).all() and b["result"][8] == 0
    for h in (0, 63):
        s = S["map_chain_home_%d" % h]
        assert s.home == h and s.max_keys == 8 and V.capacity(8) == 64
        assert [r["result"][1] for r in V.run_oracle(s) if r["kind"] == V.VOTE] == [3, 5, 8]
    # clear and reuse, find_votes
    r = V.run_oracle(S["clear_reuse"])
    assert (r[2]["ids"] == V.NO_ID).all() and not r[2]["voted"].any() and r[1]["state"][3].shape[0] == 0
    assert r[3]["ids"].tolist() == [0, 1, 2, 0] and r[3]["counted"].tolist() == [1, 1, 1, 0] and r[6]["ids"].tolist() == [0]
    assert (4, 1) in zip(S["clear_reuse"].steps[0].val.tolist(), S["clear_reuse"].steps[0].voter.tolist())   # counted again
    r = V.run_oracle(S["find_votes"])
    assert r[2]["ids"].tolist() == [0, 0, V.NO_ID, 1, 1] and r[2]["voted"].tolist() == [1, 0, 0, 0, 1]
    assert r[2]["count"].tolist() == [2, 2, 0, 1, 1] and r[3]["count"] is None and r[3]["voted"].tolist() == [1, 0]
    assert all(not st.counts for st in S["no_counts"].steps)


def test_problems_reject_wrong_results():
    S = _by_name()
    want = V.run_oracle(S["dup_tiles"])[0]
    assert V.problems(want, want) == []
    a, b = V.DUPLICATES["tiles"]
    larger = dict(want, counted=want["counted"].copy())
    larger["counted"][[a, b]] = [0, 1]                                     # the vote counted at the larger slot
    assert any("counted differs at %d" % a in p for p in V.problems(want, larger))
    later = V.run_oracle(S["repeat_later"])[1]
    both = dict(later, counted=np.ones(3, np.uint32), after=later["after"] + np.array([1, 0, 1], np.uint32))
    found = V.problems(later, both)                                        # a repeat counted
    assert any("counted differs at 0" in p for p in found) and any("after differs at 0" in p for p in found)
    scope, digests, count, masks = later["state"]
    m2 = masks.copy()
    m2[0, 0] &= ~np.uint32(2)                                              # a mask bit missing
    found = V.problems(later, dict(later, state=(scope, digests, count, m2)))
    assert "state masks differs" in found and "state count is not popcount(mask)" in found
    c2 = count.copy()
    c2[1] += 1                                                             # a count that is not popcount(mask)
    found = V.problems(later, dict(later, state=(scope, digests, c2, masks)))
    assert "state count differs" in found and "state count is not popcount(mask)" in found
    assert any("eleven result words" in p for p in V.problems(later, dict(later, result=later["result"][:10] + (7,))))
    # a map changed after full: a mask bit, a count, one more entry
    refused = V.run_oracle(S["full"])[1]
    scope, digests, count, masks = refused["state"]
    m2 = masks.copy()
    m2[1, 0] |= np.uint32(2)                                               # the refused call's vote left in
    assert "state masks differs" in V.problems(refused, dict(refused, state=(scope, digests, count, m2)))
    grown = (np.append(scope, 0).astype(np.uint32), np.vstack([digests, digests[:1]]), np.append(count, 1).astype(np.uint32),
             np.vstack([masks, masks[:1]]))
    assert any("3 entries expected, got 4" in p for p in V.problems(refused, dict(refused, state=grown)))
    found = V.run_oracle(S["find_votes"])[2]
    assert any("voted differs at 1" in p for p in V.problems(found, dict(found, voted=np.array([1, 1, 0, 0, 1], np.uint32))))
    quiet = V.run_oracle(S["no_counts"])[0]
    assert quiet["counted"] is None and V.problems(quiet, dict(quiet, counted=np.zeros(1, np.uint32))) == []


def test_vote_rules_under_asan_ubsan(tmp_path):
    seqs = [s for s in V.all_sequences() if not s.big]
    assert len(seqs) == len(V.all_sequences()) - 1
    path, results = str(tmp_path / "sequences.bin"), str(tmp_path / "results.bin")
    V.write_sequences(path, seqs)
    exe = tmp_path / "dmap_vote_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "dmap_vote_check.cpp")], check=True)
    r = subprocess.run([str(exe), path, results], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    steps = sum(len(s.steps) for s in seqs)
    assert "units and layout checked" in r.stdout and "dmap_vote ok: %d sequences, %d steps" % (len(seqs), steps) in r.stdout
    got = V.read_results(results, seqs)
    for s, g in zip(seqs, got):
        for k, (want, have) in enumerate(zip(V.run_oracle(s), g)):
            assert V.problems(want, have) == [], (s.name, k)
