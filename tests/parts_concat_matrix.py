"""Batches and the model for msha_concat_lists_device (include/mirsha.h "Part lists
flattened on the GPU"; mirbft_amd/csrc/parts_concat.hip), shared by
tests/test_parts_concat_cpu.py (the sanitized host program and the model's own checks)
and tests/test_gpu_parts_concat.py.

concat_model() is written from the header's paragraph alone: messages, layout, bytes
written, fit, the three refusals. The builders make the smallest batches at which each
piece of k_concat_copy can go wrong; S, T and the image size are read from
parts_concat.hpp so the edges move with the code.
"""
import os
import re

import numpy as np

import parts_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 64
SENTINEL = 0xA5


def _constant(name: str) -> int:
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "parts_concat.hpp")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


def step_parts() -> int:
    """S: parts a step of k_concat_copy takes."""
    return _constant("kStepParts")


def large_part() -> int:
    """T: parts of T bytes or more are copied by the whole workgroup."""
    return _constant("kLargePart")


def image_bytes() -> int:
    return _constant("kImageBytes")


def scan_width() -> int:
    """Messages one iteration of k_concat_scan takes."""
    return _constant("kScanThreads") * _constant("kScanPer")


def round16(x: int) -> int:
    return (x + 15) & ~15


# -- the model -------------------------------------------------------------------------
def concat_model(arena, off, ln, begin, select, dst_bytes):
    """-> (dst_image, written_mask, msg_off, msg_len, flagged): what the call leaves in a
    d_dst of dst_bytes bytes that held SENTINEL everywhere, which of its bytes it wrote,
    the two output arrays, and whether bit 16 of the device error word is raised."""
    n_lists = begin.size - 1
    sel = np.arange(n_lists, dtype=np.uint64) if select is None else select
    dst = np.full(dst_bytes, SENTINEL, dtype=np.uint8)
    mask = np.zeros(dst_bytes, dtype=bool)
    msg_off = np.zeros(len(sel), dtype=np.uint64)
    msg_len = np.zeros(len(sel), dtype=np.uint64)
    run, flagged = 0, False
    for k, s in enumerate(int(x) for x in sel):
        if s >= n_lists:
            flagged = True
            continue
        b0, b1 = int(begin[s]), int(begin[s + 1])
        if b1 < b0 or b1 - b0 >= 1 << 32:
            flagged = True
            continue
        if b1 - b0 == 1:
            data = arena[int(off[b0]): int(off[b0]) + int(ln[b0])]
        elif b1 > b0:
            data = np.concatenate([arena[int(off[j]): int(off[j]) + int(ln[j])] for j in range(b0, b1)])
        else:
            data = arena[:0]
        size = int(data.size)
        if run + round16(size) + SLACK <= dst_bytes:
            dst[run: run + size] = data
            dst[run + size: run + round16(size)] = 0
            mask[run: run + round16(size)] = True
            msg_off[k], msg_len[k] = run, size
        else:
            flagged = True
        run += round16(size)          # a message that does not fit still counts: none after it fits
    return dst, mask, msg_off, msg_len, flagged


def concat_need(ln, begin, select=None) -> int:
    """The smallest dst_bytes at which every message of a valid list fits."""
    n_lists = begin.size - 1
    sel = range(n_lists) if select is None else [int(s) for s in select]
    csum = np.concatenate([[0], np.cumsum(ln.astype(np.int64))])
    valid = [s for s in sel if s < n_lists and int(begin[s]) <= int(begin[s + 1])]
    return sum(round16(int(csum[int(begin[s + 1])] - csum[int(begin[s])])) for s in valid) + SLACK


def problems(model, dst, msg_off, msg_len):
    """What a result (dst: all dst_bytes bytes, SENTINEL-filled before the call) has
    wrong against concat_model()'s tuple; [] when it is exact."""
    want, mask, w_off, w_len, _ = model
    out = []
    if not np.array_equal(msg_off, w_off):
        k = int(np.nonzero(msg_off != w_off)[0][0])
        out.append("msg_off[%d] = %d, expected %d" % (k, int(msg_off[k]), int(w_off[k])))
    if not np.array_equal(msg_len, w_len):
        k = int(np.nonzero(msg_len != w_len)[0][0])
        out.append("msg_len[%d] = %d, expected %d" % (k, int(msg_len[k]), int(w_len[k])))
    if dst.size != want.size:
        return out + ["dst has %d bytes, expected %d" % (dst.size, want.size)]
    wrong = np.nonzero((dst != want) & mask)[0]
    if wrong.size:
        out.append("%d message bytes wrong, first at %d: %#x, expected %#x"
                   % (wrong.size, int(wrong[0]), int(dst[wrong[0]]), int(want[wrong[0]])))
    stray = np.nonzero((dst != SENTINEL) & ~mask)[0]
    if stray.size:
        out.append("%d bytes written outside the messages, first at %d" % (stray.size, int(stray[0])))
    return out


# -- builders --------------------------------------------------------------------------
def _lists_to_arrays(rng, lists, residue_of):
    """lists: [[bytes, ...], ...] -> (arena, off, ln, begin); part j starts at residue
    residue_of(j) mod 16, filler between the parts, SLACK after the last."""
    ar = parts_matrix.Arena(rng)
    begin = [0]
    j = 0
    for parts in lists:
        for p in parts:
            ar.put(p, residue_of(j))
            j += 1
        begin.append(len(ar.off))
    arena, off, ln = ar.arrays(SLACK)
    return arena, off, ln, np.array(begin, dtype=np.uint64)


def step_edge_counts():
    S = step_parts()
    return [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 63, 64, 65]


def step_edges(seed: int = 0x5E):
    """Lists of S-1 .. 2S+1 and 63, 64, 65 parts whose lengths cycle 1..17 from every
    one of the 17 starting points, parts at odd source offsets; one list of empty parts
    only (S + 3 of them) and one of zero parts. -> (arena, off, ln, begin)."""
    rng = np.random.default_rng(seed)
    lists = []
    for i, n in enumerate(step_edge_counts() + [2 * step_parts() + 1] * 16):
        lists.append([rng.bytes((i + j) % 17 + 1) for j in range(n)])
    lists.append([b""] * (step_parts() + 3))
    lists.append([])
    return _lists_to_arrays(rng, lists, lambda j: (2 * j + 1) % 16)


def step_boundary_phases(ln, begin):
    """The running destination phase (bytes placed mod 16) at every step boundary inside a list."""
    S, seen = step_parts(), set()
    for s in range(begin.size - 1):
        b0, b1 = int(begin[s]), int(begin[s + 1])
        for cut in range(b0 + S, b1, S):
            seen.add(int(ln[b0:cut].sum()) % 16)
    return seen


def threshold_edges(seed: int = 0x7E):
    """A part of T-1, T and T+1 bytes at source phases 0, 1 and 15, each between two
    one-byte parts (nine lists); a step of S parts summing to the image size - 1, the
    size and + 1; one 70,001-byte part. -> (arena, off, ln, begin, source phases of the big parts)."""
    rng = np.random.default_rng(seed)
    T, S, IMG = large_part(), step_parts(), image_bytes()
    lists, residues = [], []
    for size in (T - 1, T, T + 1):
        for phase in (0, 1, 15):
            lists.append([rng.bytes(1), rng.bytes(size), rng.bytes(1)])
            residues += [7, phase, 9]
    for total in (IMG - 1, IMG, IMG + 1):
        each = total // S
        assert 0 < each < T
        sizes = [each] * (S - 1) + [total - each * (S - 1)]
        assert sizes[-1] < T and sum(sizes) == total
        lists.append([rng.bytes(n) for n in sizes])
        residues += [(3 * j + 1) % 16 for j in range(S)]
    lists.append([rng.bytes(3), rng.bytes(70001), rng.bytes(2)])
    residues += [5, 11, 0]
    arena, off, ln, begin = _lists_to_arrays(rng, lists, lambda j: residues[j])
    return arena, off, ln, begin


def scan_edge_counts():
    W = scan_width()
    return [1, 63, 64, 65, W - 1, W + 1, 2 * W - 1, 2 * W + 1, 70001]


def one_part_lists(n: int, seed: int = 0x5C):
    """n one-part lists of 0..40 bytes, packed back to back (hence unaligned)."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, 41, n).astype(np.uint64)
    ln[: min(n, 41)] = np.arange(min(n, 41), dtype=np.uint64)       # every length at least once when n allows
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64) + np.uint64(3)
    arena = rng.integers(0, 256, int(ln.sum()) + 3 + SLACK, dtype=np.uint8)
    return arena, off, ln, np.arange(n + 1, dtype=np.uint64)


def write_batches(path, batches):
    """One file per batch for tests/cpp/parts_concat_check.cpp, in parts_matrix.write_batch()'s format."""
    out = []
    for i, (arena, off, ln, begin) in enumerate(batches):
        p = "%s.%d" % (path, i)
        parts_matrix.write_batch(p, arena, off, ln, begin)
        out.append(p)
    return out
