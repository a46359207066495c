"""The vote maps in the C ABI (include/mirsha.h "Device digest maps that count voters"): the
new symbols declared, exported and bound, MSHA_HAS_DIGEST_VOTE_MAP, the ABI version still
10, the two new struct mirrors laid out as the header's and the older structs as they were,
the build lists naming the two new files, null handles rejected without a GPU, and
DeviceDigestMap refusing bad tensors and the wrong kind of map before anything reaches C.
No compute calls here (CPU suite)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_dmap_create_voters", "msha_dmap_vote_device", "msha_dmap_find_votes_device", "msha_dmap_read_voters",
               "msha_dmap_get_vote_stats"]
NEW_FILES = ["dmap_vote.hpp", "dmap_vote.hip"]
RESULT_FIELDS = ["n", "entries", "added", "full", "crossed", "listed", "max_count", "max_id", "counted", "repeats",
                 "bad_voters"]
STATS_FIELDS = ["votes", "vote_finds", "slots", "launches", "max_voters", "mask_words", "last_kernel_ms"]


def test_vote_symbols_declared_exported_and_bound():
    declared = set(L.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = L.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in L.SIGNATURES and hasattr(lib, s), s
    assert len(L.SIGNATURES["msha_dmap_create_voters"][1]) == 4
    assert len(L.SIGNATURES["msha_dmap_vote_device"][1]) == 14
    assert len(L.SIGNATURES["msha_dmap_find_votes_device"][1]) == 9
    assert len(L.SIGNATURES["msha_dmap_read_voters"][1]) == 4
    assert len(L.SIGNATURES["msha_dmap_add_device"][1]) == 12              # add is as it was


def test_header_constants_and_abi_version():
    text = open(L.HEADER_PATH).read()
    assert re.search(r"^#define MSHA_HAS_DIGEST_VOTE_MAP 1\s*$", text, re.M) and L.MSHA_HAS_DIGEST_VOTE_MAP == 1
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    section = text[text.index("Device digest maps that count voters (ABI 10"):text.index("#define MSHA_HAS_DIGEST_VOTE_MAP")]
    for site in ("client_hash_disseminator.go:814-832", "checkpoints.go:264-280", "sequence.go:218"):
        assert site in section, site
    for word in ("INVARIANT: count[id] == popcount(mask[id])", "COUNTED", "FULL: ALL OR NOTHING", "CANONICAL", "bad_voters",
                 "MSHA_DMAP_PAIR_FORCE_HOME", "TEN kernels", "linear chain of ten kernel nodes", "Out of scope: erase"):
        assert word in section, word
    # the launches the text states are the layout header's constant
    hpp = open(os.path.join(ROOT, "mirbft_amd", "csrc", "dmap_vote.hpp")).read()
    assert re.search(r"constexpr uint32_t kLaunches = 10;", hpp)
    # the plain maps' section points here and no longer rules deduplication out
    plain = text[text.index("Device digest maps (ABI 10"):text.index("#define MSHA_HAS_DIGEST_MAP")]
    assert "Device digest maps that count voters" in plain and "no erase" in plain and "tombstones" in plain
    assert "per-sender deduplication of votes are out of scope" not in plain


def test_struct_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    res_off = ", ".join("offsetof(msha_dmap_vote_result, %s)" % f for f in RESULT_FIELDS)
    st_off = ", ".join("offsetof(msha_dmap_vote_stats, %s)" % f for f in STATS_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'size_t a[] = {sizeof(msha_dmap_vote_result), %s};\n'
                   'size_t b[] = {sizeof(msha_dmap_vote_stats), %s};\n'
                   'for (unsigned i = 0; i < sizeof a / sizeof *a; ++i) printf("%%zu ", a[i]);\nprintf("\\n");\n'
                   'for (unsigned i = 0; i < sizeof b / sizeof *b; ++i) printf("%%zu ", b[i]);\nprintf("\\n");\n'
                   'printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(msha_dmap_result), sizeof(msha_dmap_stats), '
                   'sizeof(msha_group_result), sizeof(msha_group_stats), sizeof(msha_stats));\n'
                   'return MSHA_HAS_DIGEST_VOTE_MAP == 1 && MSHA_HAS_DIGEST_MAP == 1 ? 0 : 1;\n}\n' % (res_off, st_off))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    res, st, old = (list(map(int, ln.split())) for ln in
                    subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in L.MshaDmapVoteResult._fields_] == RESULT_FIELDS
    assert res == [88] + list(range(0, 88, 8)) == [ctypes.sizeof(L.MshaDmapVoteResult)] + [
        getattr(L.MshaDmapVoteResult, f).offset for f in RESULT_FIELDS]
    assert all(t is ctypes.c_uint64 for _, t in L.MshaDmapVoteResult._fields_)
    assert [f for f, _ in L.MshaDmapVoteStats._fields_] == STATS_FIELDS
    assert st == [56] + list(range(0, 56, 8)) == [ctypes.sizeof(L.MshaDmapVoteStats)] + [
        getattr(L.MshaDmapVoteStats, f).offset for f in STATS_FIELDS]
    assert L.MshaDmapVoteStats._fields_[-1][1] is ctypes.c_double
    # the older structs are as they were
    assert old == [64, 56, 40, 40, 192] == [ctypes.sizeof(L.MshaDmapResult), ctypes.sizeof(L.MshaDmapStats),
                                            ctypes.sizeof(L.MshaGroupResult), ctypes.sizeof(L.MshaGroupStats),
                                            ctypes.sizeof(L.MshaStats)]


def test_build_lists_name_the_new_files():
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*?)\n(?!\s)", text, re.M | re.S).group(1).replace("\\\n", " ").split()
    assert srcs == [f.replace(os.sep, "/") for f in L._SRC_FILES]
    for f in NEW_FILES:
        assert srcs.count(f) == 1 and os.path.exists(os.path.join(ROOT, "mirbft_amd", "csrc", f)), f
    assert "$(BUILD)/dmap_vote_kernels.o" in text
    kernels = open(os.path.join(ROOT, "mirbft_amd", "csrc", "kernels.hpp")).read()
    assert "struct DmapArgs {" in kernels and "struct DmapVoteArgs : DmapArgs {" in kernels
    assert L.build_id()["matches_tree"]


def test_bad_args_rejected_without_gpu():
    """A null context or a null map is refused whatever else is passed. (With a map each
    refusal has its own message: tests/test_gpu_dmap_votes.py.)"""
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert lib.msha_dmap_create_voters(None, 16, 4, ctypes.byref(h)) == bad and not h.value
    assert lib.msha_dmap_create_voters(None, 16, 4, None) == bad
    for n in (1, 0):
        assert lib.msha_dmap_vote_device(None, None, n, None, None, 0, None, None, None, None, None, 0, None, None) == bad
        assert lib.msha_dmap_find_votes_device(None, None, n, None, None, None, None, None, None) == bad
    assert lib.msha_dmap_read_voters(None, 0, 0, None) == bad
    s = L.MshaDmapVoteStats()
    assert lib.msha_dmap_get_vote_stats(None, ctypes.byref(s)) == bad


def _no_call_map(max_voters):
    """A DeviceDigestMap with no context behind it: validation runs before any C call."""
    from mirbft_amd.digest_map import DeviceDigestMap
    from mirbft_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng._dev_index = 0
    eng._ctx = None

    class NoCall:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    eng._lib = NoCall()
    m = DeviceDigestMap.__new__(DeviceDigestMap)
    m._engine, m._lib, m.max_keys, m.max_voters, m._h = eng, eng._lib, 16, max_voters, ctypes.c_void_p(1)
    return m


@pytest.fixture
def vote_map():
    m = _no_call_map(40)
    yield m
    m._h = None


@pytest.fixture
def plain_map():
    m = _no_call_map(0)
    yield m
    m._h = None


def _good(n=70):
    import torch
    digests = torch.zeros(32 * n, dtype=torch.uint8)
    assert digests.data_ptr() % 16 == 0
    return digests, torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), torch.zeros(11, dtype=torch.int64)


def test_map_rejects_a_wrong_device(vote_map):
    dig, voter, ids, res = _good()
    with pytest.raises(ValueError, match="cuda:0"):
        vote_map.vote_device(dig, voter, ids, res)          # host tensors
    with pytest.raises(ValueError, match="cuda:0"):
        vote_map.find_votes_device(dig, voter, ids, ids.clone())


def test_the_two_kinds_refuse_each_other_before_c(vote_map, plain_map, monkeypatch):
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    dig, voter, ids, res = _good()
    with pytest.raises(ValueError, match="add_device: this is a vote map"):
        vote_map.add_device(dig, ids, res[:8].clone())
    with pytest.raises(ValueError, match="vote_device: this map keeps no voters"):
        plain_map.vote_device(dig, voter, ids, res)
    with pytest.raises(ValueError, match="find_votes_device: this map keeps no voters"):
        plain_map.find_votes_device(dig, voter, ids, ids.clone())
    with pytest.raises(ValueError, match="read_voters: this map keeps no voters"):
        plain_map.read_voters(0, 0)
    with pytest.raises(AssertionError, match="msha_dmap_add_device called"):
        plain_map.add_device(dig, ids, res[:8].clone())      # a plain map adds as before
    with pytest.raises(AssertionError, match="msha_dmap_find_device called"):
        vote_map.find_device(dig, ids)                       # find works on both kinds


def test_map_validates_tensors_before_the_call(vote_map, monkeypatch):
    """Wrong dtype or length, a missing voter, a short result, a misaligned table: each
    raises before the C call. There is no GPU here, so host tensors are made to report the
    context's device; every other property checked is their own."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    m = vote_map
    dig, voter, ids, res = _good()
    i32 = lambda k: torch.zeros(k, dtype=torch.int32)                      # noqa: E731
    with pytest.raises(AssertionError, match="msha_dmap_vote_device called"):
        m.vote_device(dig, voter, ids, res)                  # the good calls are the only ones that get through
    with pytest.raises(AssertionError, match="msha_dmap_vote_device called"):
        m.vote_device(dig, voter, ids, res, scope=i32(70), threshold=3, counted=i32(70), before=i32(70), after=i32(70),
                      crossed_slots=i32(4))
    with pytest.raises(AssertionError, match="msha_dmap_find_votes_device called"):
        m.find_votes_device(dig, voter, ids, i32(70), scope=i32(70), count=i32(70))
    m.vote_device(dig[:0], voter[:0], ids[:0], res)          # nothing to vote on: no call
    m.find_votes_device(dig[:0], voter[:0], ids[:0], ids[:0])
    with pytest.raises(ValueError, match="voter must be a tensor"):
        m.vote_device(dig, None, ids, res)
    with pytest.raises(ValueError, match="voter must hold 4-byte"):
        m.vote_device(dig, voter.long(), ids, res)
    with pytest.raises(ValueError, match="voter has 69 entries, expected 70"):
        m.vote_device(dig, voter[:69], ids, res)
    with pytest.raises(ValueError, match="counted must hold 4-byte"):
        m.vote_device(dig, voter, ids, res, counted=torch.zeros(70, dtype=torch.uint8))
    with pytest.raises(ValueError, match="counted has 1 entries"):
        m.vote_device(dig, voter, ids, res, counted=i32(1))
    with pytest.raises(ValueError, match="ids must hold 4-byte"):
        m.vote_device(dig, voter, ids.long(), res)
    with pytest.raises(ValueError, match="before must hold 4-byte"):
        m.vote_device(dig, voter, ids, res, before=torch.zeros(70, dtype=torch.float32))
    with pytest.raises(ValueError, match="result must hold 11 words"):
        m.vote_device(dig, voter, ids, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="result must hold 8-byte"):
        m.vote_device(dig, voter, ids, res.int())
    with pytest.raises(ValueError, match="32-byte rows"):
        m.vote_device(dig[:-1], voter, ids, res)
    with pytest.raises(ValueError, match="threshold must fit 32 bits"):
        m.vote_device(dig, voter, ids, res, threshold=-1)
    with pytest.raises(ValueError, match="voter must be contiguous"):
        m.vote_device(dig, i32(140)[::2], ids, res)
    with pytest.raises(ValueError, match="digests must start on a 16-byte boundary"):
        m.vote_device(torch.zeros(32 * 70 + 8, dtype=torch.uint8)[8:], voter, ids, res)
    with pytest.raises(ValueError, match="voted has 3 entries, expected 70"):
        m.find_votes_device(dig, voter, ids, i32(3))
    with pytest.raises(ValueError, match="voter and voted must be tensors"):
        m.find_votes_device(dig, voter, ids, None)
    with pytest.raises(ValueError, match="count must hold 4-byte"):
        m.find_votes_device(dig, voter, ids, i32(70), count=torch.zeros(70, dtype=torch.int16))
    from mirbft_amd import MshaError
    m._h = None
    with pytest.raises(MshaError, match="device digest map is closed"):
        m.vote_device(dig, voter, ids, res)


def test_max_voters_is_checked_before_c():
    from mirbft_amd.digest_map import DeviceDigestMap
    from mirbft_amd.engine import Engine
    eng = Engine.__new__(Engine)

    class NoCall:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    eng._lib, eng._ctx = NoCall(), None
    for bad in (-1, 1025):
        with pytest.raises(ValueError, match="max_voters must be 0"):
            DeviceDigestMap(eng, 16, bad)


def test_package_has_the_vote_map():
    import mirbft_amd
    from mirbft_amd import DeviceDigestMap, GPUHasher, tally_votes_into_map_device
    assert "tally_votes_into_map_device" in mirbft_amd.__all__
    for name in ("vote_device", "find_votes_device", "read_voters", "vote_stats"):
        assert callable(getattr(DeviceDigestMap, name)), name
    assert list(inspect.signature(DeviceDigestMap.__init__).parameters) == ["self", "engine", "max_keys", "max_voters"]
    assert inspect.signature(DeviceDigestMap.__init__).parameters["max_voters"].default == 0
    assert list(inspect.signature(GPUHasher.new_device_vote_map).parameters) == ["self", "max_keys", "max_voters"]
    sig = inspect.signature(tally_votes_into_map_device)
    assert list(sig.parameters) == ["dmap", "digests", "voter", "scope", "quorum", "crossed_cap", "stream"]
    assert (sig.parameters["quorum"].default, sig.parameters["crossed_cap"].default) == (0, 64)
