"""The stream kernel matrix on the GPU (tests/stream_matrix.py): the resume kernels
of stream_kernels.hip -- k_stream_absorb and k_stream_finish in every load mode --
and the host half of the stream sets (streams.cpp) where tests/test_gpu_streams.py
does not reach:

  a. the device forms at the natural kPrefetch (421 lanes): every finish cell (r
     class x nfull class x prefix and state x wave kind) and every absorb cell, each
     absorbed state checked word for word;
  b. the device forms at the natural kPair (768 CUs + 37 lanes), a third of the
     lanes resumed from an absorbed state with a non-zero prefix;
  c. MSHA_LOAD_MODE = 0..3, each in a fresh child process: the matrix of (a) and a
     stream-set pass, the set's last_load_mode proving the mode that ran;
  d. byte counts of 2^29 and more (bit lengths past 32 bits, and past 64), reached
     through import_state;
  e. sum, reset, export_state and import_state in four pieces of 64 lanes;
  f. an id repeated in one import: the last entry wins.

Every comparison is bit-exact. Expected digests: stream_matrix.resume_digest /
midstate (FIPS 180-4 carried there), hashlib where it can express the message.
"""
import json
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import stream_matrix as SM
from mirbft_amd import StreamSet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE_STAGING = 4096        # the minimum staging: 64 lanes a piece
N_SET = 229                 # 3 pieces of 64 lanes + one of 37

# Set when a child process ended by a signal or its time limit: nothing of this
# module goes to the GPU after that.
_child_fault = []


@pytest.fixture(autouse=True)
def _no_gpu_work_after_a_fault():
    if _child_fault:
        pytest.fail("not run: an earlier child process %s" % _child_fault[0])


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _natural_mode(n):
    """The load mode an unforced launch of n lanes runs: stream_mode() restated. The
    library reads MSHA_LOAD_MODE once per process, so it must not be set here."""
    assert "MSHA_LOAD_MODE" not in os.environ, "MSHA_LOAD_MODE is set: this process cannot run a natural load mode"
    return SM.stream_mode(n, _cus())


# -- a. device forms at natural kPrefetch ------------------------------------------------
def test_421_lanes_run_prefetch(engine):
    """What the device forms cannot report, a stream set of the same lane count can:
    421 lanes launch as kPrefetch (pick_mode's kPipe range, run as kPrefetch)."""
    assert _natural_mode(SM.N_SMALL) == 1
    launches, bad = SM.run_set_pass(engine, SM.N_SMALL, 12)
    assert not bad, bad
    assert [x["op"] for x in launches if x["op"].startswith("sum")] == ["sum %d" % r for r in range(4)]
    assert any(x["op"].startswith("write") for x in launches)
    assert {x["mode"] for x in launches} == {1}, launches


@pytest.mark.parametrize("pattern,kind", SM.finish_cases(), ids=["%s-%s" % c for c in SM.finish_cases()])
def test_finish_matrix_prefetch(engine, pattern, kind):
    mode = _natural_mode(SM.N_SMALL)
    assert mode == 1
    bad = SM.run_finish_case(engine, pattern, kind, SM.N_SMALL, mode)
    assert not bad, bad


@pytest.mark.parametrize("pattern", SM.ABSORB_PATTERNS)
def test_absorb_matrix_prefetch(engine, pattern):
    mode = _natural_mode(SM.N_SMALL)
    assert mode == 1
    bad = SM.run_absorb_case(engine, pattern, SM.N_SMALL, mode)
    assert not bad, bad


# -- b. device forms at natural kPair ----------------------------------------------------
def test_finish_matrix_pair(engine):
    """768 CUs + 37 lanes (tests/test_gpu_streams.py shows a stream set of this size
    reporting kPair): absorb_device over the resumed third, then finish_device over
    all lanes, tail lengths cycling 0..383 in ragged and whole-wave form."""
    cus = _cus()
    n = SM.pair_n(cus)
    assert _natural_mode(n) == 2, "on %d CUs n = %d is outside the kPair range" % (cus, n)
    assert SM.finish_case_cells("pair", "third", n) == {c for c in SM.FINISH_CELLS if c[2] != "null"}
    bad = SM.run_finish_case(engine, "pair", "third", n, 2, check_states=False)
    assert not bad, bad


# -- c. forced modes -----------------------------------------------------------------------
def _run_child(mode):
    env = dict(os.environ)
    env["MSHA_LOAD_MODE"] = str(mode)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "stream_matrix.py"), "--child"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    except subprocess.TimeoutExpired:
        _child_fault.append("(MSHA_LOAD_MODE=%d) ran into its time limit" % mode)
        pytest.fail("the child with MSHA_LOAD_MODE=%d ran into its time limit" % mode)
    if r.returncode < 0:
        _child_fault.append("(MSHA_LOAD_MODE=%d) ended by signal %d" % (mode, -r.returncode))
        pytest.fail("the child with MSHA_LOAD_MODE=%d ended by signal %d\n%s" % (mode, -r.returncode, r.stderr[-2000:]))
    return r


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_forced_load_mode(mode):
    """MSHA_LOAD_MODE = kSingle / kPrefetch / kPair / kPipe in a process of its own:
    the device-form matrix at 421 lanes and a stream-set pass. Every launch of the
    set reports the forced mode (kPipe: kPrefetch, stream_mode's mapping); pick_mode's
    static is the process', so the device forms ran it too."""
    r = _run_child(mode)
    assert r.returncode == 0, "child exit status %d\n%s" % (r.returncode, r.stderr[-2000:])
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            c = json.loads(line)
            got[c["case"]] = c
    assert list(got) == SM.child_cases(), (list(got), r.stderr[-2000:])
    want = 1 if mode == 3 else mode
    for case, c in got.items():
        assert c["mode"] == mode
        assert not c["mismatch"], ("MSHA_LOAD_MODE=%d / %s" % (mode, case), c["mismatch"])
    launches = got["stream_set"]["launches"]
    assert [x["op"] for x in launches if x["op"].startswith("sum")] == ["sum %d" % k for k in range(4)]
    assert any(x["op"].startswith("write") for x in launches)
    assert {x["mode"] for x in launches} == {want}, (mode, launches)


# -- d. byte counts above 2^32 bits ------------------------------------------------------
def _blob(words, buf, length):
    return b"sha\x03" + struct.pack(">8I", *words) + bytes(buf).ljust(64, b"\x00") + struct.pack(">Q", length)


def _blobs(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 108)


def test_byte_counts_above_32_bits_of_bit_length(engine):
    """States built by hand and imported: totals of 2^29 - 64 .. 2^61 + 63 bytes.
    build_tail / length_block see prefix + work with bits past 2^32 (and 8 L past
    2^64, which wraps as Go's len <<= 3 does); the host's length arithmetic and the
    export's high word see them too."""
    rnd = random.Random(14)
    cases = [(B, t) for B in (2 ** 29 - 64, 2 ** 29, 2 ** 32, 2 ** 35, 2 ** 61 - 64, 2 ** 61)
             for t in (0, 1, 55, 56, 63)]
    n = len(cases)
    words = [[rnd.getrandbits(32) for _ in range(8)] for _ in cases]
    bufs = [rnd.randbytes(64) for _ in cases]
    L = [B + t for B, t in cases]
    assert max(L) + 200 < 2 ** 63
    ids = list(range(n))
    with StreamSet(engine, n) as ss:
        ss.import_state(ids, _blobs([_blob(w, b, k) for w, b, k in zip(words, bufs, L)]))
        got = ss.sum()
        for i, (B, t) in enumerate(cases):
            assert bytes(got[i]) == SM.resume_digest(words[i], bufs[i][:t], L[i]), ("sum", "B = %d" % B, "t = %d" % t)
        assert ss.lengths().tolist() == L
        ex = ss.export_state()
        for i, (B, t) in enumerate(cases):
            assert bytes(ex[i]) == _blob(words[i], bufs[i][:t], L[i]), ("export", "B = %d" % B, "t = %d" % t)
        # 200 more bytes: one absorb of the buffered tail + whole blocks, and a new tail
        extra = [rnd.randbytes(200) for _ in cases]
        before = ss.stats()["launches_absorb"]
        ss.write(ids, extra)
        assert ss.stats()["launches_absorb"] == before + 1
        got = ss.sum()
        assert ss.lengths().tolist() == [k + 200 for k in L]
        ex = ss.export_state()
        for i, (B, t) in enumerate(cases):
            what = ("after 200 more bytes", "B = %d" % B, "t = %d" % t)
            data = bufs[i][:t] + extra[i]
            assert bytes(got[i]) == SM.resume_digest(words[i], data, L[i] + 200), what
            raw = bytes(ex[i])
            assert struct.unpack(">II", raw[100:108]) == ((L[i] + 200) >> 32, (L[i] + 200) & 0xFFFFFFFF), what
            assert raw == _blob(SM.absorb(words[i], data), data[len(data) // 64 * 64:], L[i] + 200), what


# -- e. set operations in several pieces ---------------------------------------------------
@pytest.fixture(scope="module")
def set_inputs():
    """229 messages, their write bounds, and every stream's expected export."""
    msgs, bounds, used = SM.set_pass_inputs(N_SET, 5)
    assert used == set(SM.CUT_KINDS)
    blobs = [_blob(SM.midstate(m), m[len(m) // 64 * 64:], len(m)) for m in msgs]
    return msgs, bounds, blobs


def _pieces(k):
    return (k + 63) // 64


def _check_rows(got, exp, ids, what):
    bad = [(j, int(ids[j])) for j in range(len(ids)) if bytes(got[j]) != exp[j]]
    assert not bad, (what, "%d rows differ; first (row, id): %s" % (len(bad), bad[:6]))


def test_set_operations_in_four_pieces(engine, set_inputs):
    msgs, bounds, blobs = set_inputs
    sums = [SM.sha(m) for m in msgs]
    empty = SM.sha(b"")
    rnd = random.Random(15)
    perm = list(range(N_SET))
    rnd.shuffle(perm)
    subset = rnd.sample(range(N_SET), 150)                    # 3 pieces, in no order
    rep = [rnd.randrange(N_SET) for _ in range(200)]          # 4 pieces
    rep[70], rep[199] = rep[3], rep[3]                        # one id three times, in different pieces
    rep[5] = rep[4]                                           # and one twice in a row
    assert len(set(subset)) == 150 and len(set(rep)) < len(rep)
    all_ids = np.arange(N_SET, dtype=np.uint64)
    with StreamSet(engine, N_SET, staging_bytes=PIECE_STAGING) as a, \
            StreamSet(engine, N_SET, staging_bytes=PIECE_STAGING) as b:
        # the boundary matrix's write / sum cycle
        for r in range(4):
            a.write(all_ids, [m[c[r]:c[r + 1]] for m, c in zip(msgs, bounds)])
            f0 = a.stats()["launches_finish"]
            got = a.sum()
            assert a.stats()["launches_finish"] == f0 + 4, "sum() over 229 streams at 64 lanes a piece"
            _check_rows(got, [SM.sha(m[:c[r + 1]]) for m, c in zip(msgs, bounds)], all_ids, "sum, round %d" % r)
            assert a.lengths().tolist() == [c[r + 1] for c in bounds]
        # sum and export: row j belongs to ids[j]
        for name, ids in (("permuted", perm), ("subset", subset), ("repeated", rep)):
            f0 = a.stats()["launches_finish"]
            got = a.sum(ids)
            assert a.stats()["launches_finish"] == f0 + _pieces(len(ids)), name
            _check_rows(got, [sums[i] for i in ids], ids, "sum(%s)" % name)
            _check_rows(a.export_state(ids), [blobs[i] for i in ids], ids, "export_state(%s)" % name)
        _check_rows(a.export_state(), blobs, all_ids, "export_state()")
        # import into a second set: the named streams take the states, the others keep theirs
        other = [b"untouched %d" % i for i in range(N_SET)]
        for name, ids in (("permuted", perm), ("subset", subset)):
            b.reset()
            b.write(all_ids, other)
            b.import_state(ids, a.export_state(ids))
            named = set(ids)
            _check_rows(b.sum(), [sums[i] if i in named else SM.sha(other[i]) for i in range(N_SET)], all_ids,
                        "sum() after import_state(%s)" % name)
            assert b.lengths().tolist() == [len(msgs[i]) if i in named else len(other[i]) for i in range(N_SET)]
            _check_rows(b.export_state(ids), [blobs[i] for i in ids], ids, "export after import_state(%s)" % name)
            # and on from the imported states
            more = [b"+%d" % i * (1 + i % 40) for i in ids]
            b.write(ids, more)
            _check_rows(b.sum(ids), [SM.sha(msgs[i] + x) for i, x in zip(ids, more)], ids,
                        "sum(%s) after import and write" % name)
        # reset: a subset in no order, then all by a permuted list
        a.reset(subset)
        named = set(subset)
        _check_rows(a.sum(), [empty if i in named else sums[i] for i in range(N_SET)], all_ids,
                    "sum() after reset(subset)")
        assert a.lengths().tolist() == [0 if i in named else len(msgs[i]) for i in range(N_SET)]
        _check_rows(a.export_state(subset), [_blob(SM.IV, b"", 0)] * len(subset), subset, "export after reset(subset)")
        a.reset(perm)
        _check_rows(a.sum(perm), [empty] * N_SET, perm, "sum(permuted) after reset(permuted)")
        assert not a.lengths().any()


# -- f. a repeated id in one import ----------------------------------------------------------
def test_a_repeated_id_in_one_import_last_entry_wins(engine):
    """mirsha.h: an id repeated in one import is sequential UnmarshalBinary, the
    last entry wins for state, buffer and length alike. Two states for one id in the
    same wave of a piece, in different pieces, and in the partial last piece."""
    rnd = random.Random(16)
    filler = [i for i in range(N_SET) if i not in (5, 100, 7)]
    rnd.shuffle(filler)
    ids = filler[:100]
    for pos, s in ((0, 5), (3, 5), (10, 100), (80, 100), (70, 7), (95, 7), (99, 7)):
        ids[pos] = s
    assert len(ids) == 100 and len(set(ids)) == 96
    words = [[rnd.getrandbits(32) for _ in range(8)] for _ in ids]
    bufs = [rnd.randbytes(64) for _ in ids]
    lens = [64 * rnd.randrange(0, 1000) + (j * 7) % 64 for j in range(len(ids))]
    last = {s: j for j, s in enumerate(ids)}                  # sequential import: the last entry of an id
    assert (last[5], last[100], last[7]) == (3, 80, 99)
    with StreamSet(engine, N_SET, staging_bytes=PIECE_STAGING) as ss:
        ss.import_state(ids, _blobs([_blob(w, b, k) for w, b, k in zip(words, bufs, lens)]))
        named = sorted(last)
        want = [last[s] for s in named]
        _check_rows(ss.sum(named), [SM.resume_digest(words[j], bufs[j][:lens[j] % 64], lens[j]) for j in want], named,
                    "sum() after an import with repeated ids")
        _check_rows(ss.export_state(named), [_blob(words[j], bufs[j][:lens[j] % 64], lens[j]) for j in want], named,
                    "export_state() after an import with repeated ids")
        assert ss.lengths(named).tolist() == [lens[j] for j in want]
        others = [i for i in range(N_SET) if i not in last]
        _check_rows(ss.sum(others), [SM.sha(b"")] * len(others), others, "the streams the import did not name")
