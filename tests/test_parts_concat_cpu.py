"""The placement logic of k_concat_copy (mirbft_amd/csrc/parts_concat.hpp) under
AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/parts_concat_check.cpp), over the batches the GPU test launches
(tests/parts_concat_matrix.py); the builders proven to cover what they claim; and the
model shown to reject wrong results. Host code only: nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import parts_concat_matrix as M
import parts_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(begin):
    return [int(b) - int(a) for a, b in zip(begin, begin[1:])]


def test_step_edges_cover_what_they_claim():
    S = M.step_parts()
    arena, off, ln, begin = M.step_edges()
    counts = _counts(begin)
    assert set(counts) == {S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 63, 64, 65, S + 3, 0}
    assert {int(x) for x in ln[ln > 0]} == set(range(1, 18))            # lengths cycle 1..17
    assert M.step_boundary_phases(ln, begin) == set(range(16))          # every phase at a step boundary
    assert {int(o) % 2 for o, l in zip(off, ln) if l} == {1}            # odd source offsets
    empties = [s for s in range(len(counts)) if counts[s] and not ln[int(begin[s]): int(begin[s + 1])].any()]
    assert len(empties) == 1 and counts[empties[0]] == S + 3            # one list of empty parts only
    assert arena.size >= int((off + ln).max()) + M.SLACK


def test_threshold_edges_cover_what_they_claim():
    T, S, IMG = M.large_part(), M.step_parts(), M.image_bytes()
    arena, off, ln, begin = M.threshold_edges()
    big = {(int(ln[j]), int(off[j]) % 16) for s in range(9) for j in [int(begin[s]) + 1]}
    assert big == {(n, p) for n in (T - 1, T, T + 1) for p in (0, 1, 15)}
    for s in range(9):                                                  # a one-byte part on each side
        assert _counts(begin)[s] == 3 and ln[int(begin[s])] == 1 == ln[int(begin[s]) + 2]
    sums = [int(ln[int(begin[s]): int(begin[s + 1])].sum()) for s in (9, 10, 11)]
    assert sums == [IMG - 1, IMG, IMG + 1] and all(_counts(begin)[s] == S for s in (9, 10, 11))
    assert int(ln[int(begin[9]): int(begin[12])].max()) < T             # steps of small parts only
    assert 70001 in ln[int(begin[12]): int(begin[13])].tolist()
    assert arena.size >= int((off + ln).max()) + M.SLACK


def test_scan_edges_cover_what_they_claim():
    W = M.scan_width()
    counts = M.scan_edge_counts()
    assert {1, 63, 64, 65, 70001} <= set(counts)
    assert any(c % W == W - 1 for c in counts) and any(c % W == 1 and c > W for c in counts)
    arena, off, ln, begin = M.one_part_lists(70001)
    assert {int(x) for x in ln} == set(range(41)) and _counts(begin) == [1] * 70001
    assert arena.size >= int((off + ln).max()) + M.SLACK


def _small():
    rng = np.random.default_rng(3)
    lists = [[rng.bytes(5), rng.bytes(20)], [], [rng.bytes(16)], [rng.bytes(1), b"", rng.bytes(40)]]
    return M._lists_to_arrays(rng, lists, lambda j: (5 * j + 3) % 16), lists


def test_model_follows_the_header():
    (arena, off, ln, begin), lists = _small()
    need = M.concat_need(ln, begin)
    assert need == 32 + 0 + 16 + 48 + M.SLACK
    dst, mask, mo, ml, flagged = M.concat_model(arena, off, ln, begin, None, need)
    assert not flagged and mo.tolist() == [0, 32, 32, 48] and ml.tolist() == [25, 0, 16, 41]
    assert dst[:25].tobytes() == b"".join(lists[0]) and not dst[25:32].any()
    assert dst[48:89].tobytes() == b"".join(lists[3]) and not dst[89:96].any()
    assert mask[:96].all() and not mask[96:].any() and (dst[96:] == M.SENTINEL).all()
    # one byte less: the last message is refused and nothing of it is written
    dst, mask, mo, ml, flagged = M.concat_model(arena, off, ln, begin, None, need - 1)
    assert flagged and mo.tolist() == [0, 32, 32, 0] and ml.tolist() == [25, 0, 16, 0]
    assert not mask[48:].any() and (dst[48:] == M.SENTINEL).all()
    # select: a repeat is a second copy; an id out of range and a decreasing list are refused, length 0 in the sum
    bad = begin.copy()
    bad[2] = 0                                                          # list 1 decreases, list 2 = parts [0, 3)
    sel = np.array([3, 4, 1, 3], dtype=np.uint32)
    dst, mask, mo, ml, flagged = M.concat_model(arena, off, ln, bad, sel, 4096)
    assert flagged and mo.tolist() == [0, 0, 0, 48] and ml.tolist() == [41, 0, 0, 41]
    assert dst[:41].tobytes() == dst[48:89].tobytes() == b"".join(lists[3])
    # nothing fits an empty d_dst, not even an empty message
    dst, mask, mo, ml, flagged = M.concat_model(arena, off, ln, begin, None, 0)
    assert flagged and dst.size == 0 and not mo.any() and not ml.any()


def test_model_rejects_wrong_results():
    (arena, off, ln, begin), _ = _small()
    need = M.concat_need(ln, begin)
    model = M.concat_model(arena, off, ln, begin, None, need)
    dst, _, mo, ml, _ = model
    assert M.problems(model, dst.copy(), mo.copy(), ml.copy()) == []
    d = dst.copy()
    d[24] ^= 0xFF                                                       # a dropped (wrong) byte
    assert any("message bytes wrong" in p for p in M.problems(model, d, mo, ml))
    d = dst.copy()
    d[30] = 7                                                           # a pad byte that is not zero
    assert any("message bytes wrong" in p for p in M.problems(model, d, mo, ml))
    d = dst.copy()
    d[96] = 0                                                           # a byte written past the last pad
    assert any("outside the messages" in p for p in M.problems(model, d, mo, ml))
    o = mo.copy()
    o[2] += np.uint64(16)                                               # a wrong offset
    assert any("msg_off[2]" in p for p in M.problems(model, dst, o, ml))
    refused = M.concat_model(arena, off, ln, begin, None, need - 1)
    keep = refused[3].copy()
    keep[3] = 41                                                        # a refused message that keeps its length
    assert any("msg_len[3]" in p for p in M.problems(refused, refused[0], refused[2], keep))


def test_placement_under_asan_ubsan(tmp_path):
    arena, off, ln, begin, _, _ = parts_matrix.boundary_matrix()
    batches = [(arena, off, ln, begin), M.step_edges(), M.threshold_edges(), M.one_part_lists(300)]
    files = M.write_batches(str(tmp_path / "matrix.bin"), batches)
    exe = tmp_path / "parts_concat_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "parts_concat_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    for b in batches:
        assert "matrix: %d lists, %d parts" % (b[3].size - 1, b[1].size) in r.stdout
    assert "parts_concat ok" in r.stdout
