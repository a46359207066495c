"""The exported stream state and the id lists both kinds of stream set share
(mirbft_amd/csrc/stream_state.hpp) under AddressSanitizer + UBSan, as a stand-alone
program with its own main (tests/cpp/stream_state_check.cpp). The expected bytes are
built here with struct.pack, from crypto/sha256's MarshalBinary layout, and nothing of
the header's. Host code only: nothing is loaded into Python."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = b"sha\x03"


def _blob(state, buf, length, magic=MAGIC):
    return magic + struct.pack(">8I", *state) + buf.ljust(64, b"\0") + struct.pack(">Q", length)


def _ids(tag, id_, k, n=None):
    head = (struct.pack("<Q", n) if n is not None else b"") + struct.pack("<BQ", id_ is not None, k)
    return tag + head + (struct.pack("<%dQ" % k, *id_) if id_ is not None else b"")


def _last_wins(id_, k, want):
    return _ids(b"L", id_, k) + struct.pack("<Q%dQ" % len(want), len(want), *want)


def test_stream_state_under_asan_ubsan(tmp_path):
    rng = np.random.default_rng(23)
    rec, count = [], {"E": 0, "D": 0, "M": 0, "L": 0, "V": 0}

    def add(tag, body):
        rec.append(body)
        count[tag] += 1

    # encode, and decode(encode(x)) == x: every buffer edge, both words of the length, the largest length
    lengths = [0, 1, 55, 56, 63, 64, 64 * 7 + 55,
               (1 << 32) - 1, 1 << 32, (1 << 32) + 56, (5 << 32) + 63, (1 << 63) + 1, (1 << 64) - 64, (1 << 64) - 1]
    assert {x % 64 for x in lengths} >= {0, 1, 55, 56, 63} and lengths[-1] % 64 == 63
    for length in lengths:
        state = [int(x) for x in rng.integers(0, 1 << 32, size=8, dtype=np.uint64)]
        buf = rng.bytes(length % 64)
        blob = _blob(state, buf, length)
        assert len(blob) == 108
        add("E", b"E" + struct.pack("<8IQ", *state, length) + buf + blob)
    add("E", b"E" + struct.pack("<8IQ", *([0xFFFFFFFF] * 8), 63) + b"\xff" * 63 + _blob([0xFFFFFFFF] * 8, b"\xff" * 63, 63))

    # an input blob's bytes past length % 64 are dropped
    for length in (0, 1, 55, 63, (1 << 32) + 7):
        state = list(range(1, 9))
        buf = rng.bytes(length % 64)
        dirty = _blob(state, buf + b"\xee" * (64 - length % 64), length)
        assert dirty != _blob(state, buf, length)
        add("D", b"D" + dirty + _blob(state, buf, length))

    # the magic, and a wrong byte at each of its four places
    good = _blob(range(8), b"abc", 3)
    add("M", b"M" + good + b"\1")
    for at in range(4):
        for wrong in (MAGIC[at] ^ 1, MAGIC[at] ^ 0x80, 0):
            bad = bytearray(good)
            bad[at] = wrong
            assert bad[at] != good[at]
            add("M", b"M" + bytes(bad) + b"\0")
    add("M", b"M" + b"sha\x02" + good[4:] + b"\0")             # the magic of another hash

    # of the entries that name one stream the last wins; what takes effect, in call order
    add("L", _last_wins(None, 5, [0, 1, 2, 3, 4]))            # id NULL: all
    add("L", _last_wins([4, 0, 9, 2], 4, [0, 1, 2, 3]))       # no repeats
    add("L", _last_wins([3, 1, 3, 3, 1], 5, [3, 4]))
    add("L", _last_wins([7, 7, 7], 3, [2]))
    add("L", _last_wins([1, 2, 1, 2, (1 << 64) - 1], 5, [2, 3, 4]))
    add("L", _last_wins([], 0, []))                           # k == 0, with and without ids
    add("L", _last_wins(None, 0, []))

    for n, id_, k, ok in [(4, None, 4, 1), (4, None, 3, 0), (4, None, 0, 0), (4, [0, 3, 3], 3, 1), (4, [0, 4], 2, 0),
                          (4, [], 0, 1), (1, [(1 << 64) - 1], 1, 0)]:
        add("V", _ids(b"V", id_, k, n) + struct.pack("<B", ok))

    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(rec))
    exe = tmp_path / "stream_state_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "stream_state_check.cpp")], check=True)
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert ("stream_state ok: %d encode, %d dirty, %d magic, %d last_wins, %d ids_valid"
            % (count["E"], count["D"], count["M"], count["L"], count["V"])) in r.stdout
