"""Host-side mirror of the reference's hash plugin surface, backed by the GPU.

Reference interface (Go, /root/reference/pkg/processor/serial.go):

    type Hasher interface { New() hash.Hash }                              // :21-23
    func ProcessHashActions(hasher Hasher, actions *statemachine.ActionList)
            (*statemachine.EventList, error)                               // :180-198

with the action/event constructors of pkg/statemachine/actions.go:173-187 and
events.go:96-110 and the schema of protos/state/state.proto:78-109,168-171.

Names, argument meaning and error behaviour follow the reference:
``ProcessHashActions`` returns one ``HashResult`` per action, in list order,
whose ``origin`` is the *same object* as the action's; a non-hash action makes
it fail with "unexpected type for Hash action: <type>" (serial.go:192-194),
raised here as ``ProcessorError``. The whole list is hashed by ONE
``msha_hash_actions`` call (one H2D, one launch per GPU, one D2H).

An EpochChange payload the list already carries is packed once (as the Go
drop-in does, go/pkg/processor/gpuhash.go epochChangeAliases): actions whose
origin holds the same EpochChange object, or an equal payload from the same
origin node, share the first one's (off, len), so it crosses PCIe once.

``GPUHasher.new()`` keeps the per-message ``hash.Hash`` surface that
``Client.Propose`` (clients.go:189-192) and the testengine app chain
(recorder.go:288-359) use: writes are buffered and ``sum()`` submits a
one-message batch to the GPU. Nothing in this module hashes on the CPU.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Iterator, List, Optional, Sequence, Union

import numpy as np

from .encoding import EpochChange, RequestAck, checkpoint_hash_data
from .engine import Engine


class ProcessorError(RuntimeError):
    pass


# ---------------------------------------------------------------------------
# state.HashOrigin and friends (protos/state/state.proto:78-104)
# ---------------------------------------------------------------------------
@dataclass
class HashOriginBatch:
    source: int
    epoch: int
    seq_no: int
    request_acks: List[RequestAck] = field(default_factory=list)


@dataclass
class HashOriginVerifyBatch:
    source: int
    seq_no: int
    request_acks: List[RequestAck] = field(default_factory=list)
    expected_digest: bytes = b""


@dataclass
class HashOriginEpochChange:
    source: int
    origin: int
    epoch_change: Optional[EpochChange] = None


@dataclass
class HashOrigin:
    type: Union[HashOriginBatch, HashOriginVerifyBatch, HashOriginEpochChange, None] = None


@dataclass
class ActionHashRequest:
    """state.ActionHashRequest{repeated bytes data; HashOrigin origin} (state.proto:168-171)."""
    data: List[bytes]
    origin: Optional[HashOrigin]


@dataclass
class ActionHash:
    hash: ActionHashRequest


@dataclass
class Action:
    """state.Action: a oneof; only ActionHash is valid on the hash path."""
    type: Any


@dataclass
class EventHashResult:
    """state.EventHashResult{bytes digest; HashOrigin origin} (state.proto:106-109)."""
    digest: bytes
    origin: Optional[HashOrigin]


@dataclass
class EventHashResultType:
    hash_result: EventHashResult


@dataclass
class Event:
    type: Any


class ActionList:
    """statemachine.ActionList (a linked list in Go; order is what matters)."""

    def __init__(self, actions: Optional[Sequence[Action]] = None):
        self._l: List[Action] = list(actions or [])

    def push_back(self, a: Action) -> "ActionList":
        self._l.append(a)
        return self

    def hash(self, data: List[bytes], origin: Optional[HashOrigin]) -> "ActionList":
        """ActionList.Hash (actions.go:173-176)."""
        return self.push_back(action_hash(data, origin))

    def __iter__(self) -> Iterator[Action]:
        return iter(self._l)

    def __len__(self) -> int:
        return len(self._l)


class EventList:
    def __init__(self):
        self._l: List[Event] = []

    def push_back(self, e: Event) -> "EventList":
        self._l.append(e)
        return self

    def hash_result(self, digest: bytes, origin: Optional[HashOrigin]) -> "EventList":
        """EventList.HashResult (events.go:96-99)."""
        return self.push_back(Event(EventHashResultType(EventHashResult(digest, origin))))

    def __iter__(self) -> Iterator[Event]:
        return iter(self._l)

    def __len__(self) -> int:
        return len(self._l)


def action_hash(data: List[bytes], origin: Optional[HashOrigin]) -> Action:
    """statemachine.ActionHash (actions.go:178-187)."""
    return Action(ActionHash(ActionHashRequest(data=list(data), origin=origin)))


# ---------------------------------------------------------------------------
# Hasher
# ---------------------------------------------------------------------------
class _GPUHash:
    """hash.Hash over the GPU engine: Write appends, Sum(b) appends the digest
    of everything written so far without resetting (Go hash.Hash semantics)."""

    size = 32
    block_size = 64

    def __init__(self, engine: Engine):
        self._engine = engine
        self._buf = bytearray()

    def write(self, p: bytes) -> int:
        self._buf += p
        return len(p)

    def sum(self, b: bytes = b"") -> bytes:
        return bytes(b) + self._engine.hash_actions([[bytes(self._buf)]])[0]

    def reset(self) -> None:
        self._buf.clear()


class GPUHasher:
    """processor.Hasher backed by libmirsha; also exposes the batched surface
    ProcessHashActions uses."""

    def __init__(self, engine: Optional[Engine] = None, device_mask: int = 1):
        self.engine = engine if engine is not None else Engine(device_mask)

    def new(self) -> _GPUHash:
        return _GPUHash(self.engine)

    def new_streams(self, n: int, staging_bytes: int = 0):
        """n resumable hash.Hash streams on the GPU (StreamSet): for many concurrent
        running hashes, e.g. one NodeState.ActiveHash per node (recorder.go:288-359).
        new() stays the single buffered hash."""
        from .streams import StreamSet
        return StreamSet(self.engine, n, staging_bytes)

    def new_device_streams(self, n: int):
        """n resumable hash.Hash streams kept entirely in device memory
        (DeviceStreamSet): written from parts that already sit in HBM, summed and
        snapped there, one launch a call with no host wait."""
        from .streams_device import DeviceStreamSet
        return DeviceStreamSet(self.engine, n)

    def new_device_digest_map(self, max_keys: int):
        """A digest-keyed tally of up to max_keys keys kept in device memory across calls
        (DeviceDigestMap): stable entry ids, running counts, and for each call the keys
        whose count crossed a threshold."""
        from .digest_map import DeviceDigestMap
        return DeviceDigestMap(self.engine, max_keys)

    def new_device_vote_map(self, max_keys: int, max_voters: int):
        """A device digest map whose count for a key is the number of distinct voters, of
        max_voters (1 .. 1024) nodes, that voted for it (DeviceDigestMap with max_voters):
        the set of voters is kept in HBM beside the key, so a sender's second ack counts
        nothing. Filled with tally_votes_into_map_device."""
        from .digest_map import DeviceDigestMap
        return DeviceDigestMap(self.engine, max_keys, max_voters)

    def hash_batch(self, actions: Sequence[Sequence[bytes]]) -> List[bytes]:
        return self.engine.hash_actions(actions)

    def close(self) -> None:
        """Release the packing buffers (the engine stays open)."""
        for name in ("_arena", "_off", "_len", "_out"):
            buf = self.__dict__.pop(name, None)
            if buf is not None and getattr(self.engine, "_ctx", None):
                self.engine.pinned_free(buf)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _pinned(self, name: str, nbytes: int) -> np.ndarray:
        """A page-locked buffer of at least nbytes, grown on demand (the Go
        adapter's pinnedBuf)."""
        buf = getattr(self, name, None)
        if buf is None or buf.size < nbytes:
            if buf is not None:
                self.engine.pinned_free(buf)
            buf = self.engine.pinned_empty(max(nbytes + nbytes // 4, 4096))
            setattr(self, name, buf)
        return buf[:nbytes]

    def hash_requests(self, reqs: Sequence["ActionHashRequest"]) -> List[bytes]:
        """One digest per hash request, packed the way the Go drop-in packs an
        ActionList (gpuhash.go digests): each request's parts back to back,
        16-byte aligned, in a pinned arena; off/len and the digests pinned
        too; ONE msha_digest_batch. EpochChange payloads are packed once
        (_epoch_change_aliases). last_pack holds what was packed."""
        n = len(reqs)
        alias = _epoch_change_aliases(reqs)
        off = self._pinned("_off", 8 * n).view(np.uint64)
        ln = self._pinned("_len", 8 * n).view(np.uint64)
        chunks, pos = [], 0
        for i, r in enumerate(reqs):
            j = alias[i]
            if j >= 0:
                off[i], ln[i] = off[j], ln[j]
                continue
            data = b"".join(r.data)
            off[i], ln[i] = pos, len(data)
            chunks.append((pos, data))
            pos = (pos + len(data) + 15) & ~15
        arena = self._pinned("_arena", pos + 64)
        for p, data in chunks:
            arena[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)
        out = self._pinned("_out", 32 * n).reshape(n, 32)
        self.engine.digest_batch(arena, off, ln, out=out)
        self.last_pack = {"actions": n, "payloads": len(chunks), "packed_bytes": pos,
                          "payload_bytes": sum(len(d) for _, d in chunks),
                          "aliased": int(sum(1 for a in alias if a >= 0))}
        return [bytes(r) for r in out]

    def request_digests(self, requests: Sequence[bytes]) -> List[bytes]:
        """Batched request intake: the digest that
        Client.Propose computes per call (clients.go:189-192, ``h.Write(data);
        h.Sum(nil)``) for a whole batch of proposals, in one GPU call
        (msha_digest_batch over a packed arena)."""
        if not requests:
            return []
        lens = np.fromiter((len(r) for r in requests), dtype=np.uint64, count=len(requests))
        offs = np.zeros(len(requests), dtype=np.uint64)
        if len(requests) > 1:
            offs[1:] = np.cumsum(lens)[:-1]
        arena = np.frombuffer(b"".join(bytes(r) for r in requests), dtype=np.uint8)
        out = self.engine.digest_batch(arena, offs, lens)
        return [bytes(r) for r in out]


def checkpoint_hashes(hasher: GPUHasher, intervals: Sequence[tuple]) -> List[bytes]:
    """the testengine's app-level checkpoint value
    (NodeState.Snap, recorder.go:288-300) for many (node, interval) pairs in one
    GPU call. intervals[i] = (prev_checkpoint_hash or None, [committed request
    digests]); result[i] = ActiveHash.Sum(nil) at Snap = SHA-256 of
    checkpoint_hash_data(prev, digests). Every part is a 32-byte digest, so this
    is the digest-of-digests kernel over one table of all parts. A node's
    successive intervals form a chain (each starts from the previous result), so
    the batch dimension is across nodes / ready intervals."""
    if not intervals:
        return []
    parts: List[bytes] = []
    begin = [0]
    for prev, digests in intervals:
        for d in checkpoint_hash_data(prev, list(digests)):
            if len(d) != 32:
                raise ProcessorError("checkpoint_hashes: every part must be a 32-byte digest")
            parts.append(bytes(d))
        begin.append(len(parts))
    table = np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(-1, 32) if parts \
        else np.zeros((0, 32), dtype=np.uint8)
    idx = np.arange(len(parts), dtype=np.uint32)
    out = hasher.engine.digest_of_digests(table, idx, np.array(begin, dtype=np.uint64))
    return [bytes(r) for r in out]


def verify_batches_device(hasher: GPUHasher, table, idx, begin, expected, list_cap: int = 64, stream=None):
    """VerifyBatch in HBM (applyVerifyBatchHashResult, batch_tracker.go:175-195): batch i
    is the request digests table[idx[begin[i] : begin[i + 1]]], its digest (what
    digest_of_digests_device gives) is compared on the GPU with expected[32 i ..], and
    only the answer comes down. All four are torch tensors on the engine's GPU, laid out
    as Engine.digest_of_digests_device and Engine.verify_digests_device take them.
    Returns (bad, first_bad, bad_indices): how many batches differ, the first of them
    (the batch count when none does) and the first min(bad, list_cap) of them in
    ascending order. One 40-byte read, and, only when bad > 0, one read of the listed
    indices. stream: a torch.cuda.Stream of the caller's (None: the engine's own)."""
    import torch
    eng = hasher.engine
    n = begin.numel() - 1
    if n < 0:
        raise ProcessorError("verify_batches_device: begin must have at least one entry")
    if n == 0:
        return 0, 0, []
    dev = begin.device
    digests = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    mask = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    result = torch.empty(5, dtype=torch.int64, device=dev)
    bad_list = torch.empty(int(list_cap), dtype=torch.int32, device=dev) if list_cap > 0 else None
    # The two calls go on `stream`; None, or torch's default stream, means the engine's own
    # stream, which is no stream of torch's: then the whole device is waited for, before
    # (what torch still owes the inputs) and after. A stream of the caller's is waited
    # for alone.
    own = not eng._stream_ptr(stream)
    if own:
        torch.cuda.synchronize(dev)
    eng.digest_of_digests_device(table, idx, begin, digests, stream=stream)
    eng.verify_digests_device(digests, expected, mask, result, bad_list=bad_list, stream=stream)
    if own or not hasattr(stream, "synchronize"):
        torch.cuda.synchronize(dev)
    else:
        stream.synchronize()
    _, bad, first_bad, listed, _ = (int(x) for x in result.cpu().tolist())
    indices = []
    if bad > 0 and listed > 0:
        indices = [int(x) & 0xFFFFFFFF for x in bad_list[:listed].cpu().tolist()]
    return bad, first_bad, indices


def tally_digests_device(hasher: GPUHasher, digests, scope=None, group_cap: int = 64, stream=None):
    """The digest-keyed maps of the state machine in HBM (prepares and commits,
    sequence.go:73-74, 271-277; a checkpoint's values, checkpoints.go:264-290; the acks
    per (client, reqNo), client_hash_disseminator.go:415-504): slot i's key is
    (scope[i], the 32 bytes digests[32 i ..]), scope None meaning one map. digests is a
    uint8 tensor of 32 n bytes and scope an int32 tensor of n entries, both on the
    engine's GPU. Returns (groups, max_count, max_group, first, group, members,
    group_first, group_count): how many distinct keys there are, the size of the largest
    group and its number, and the tensors Engine.group_digests_device fills, the last two
    cut to min(groups, group_cap) entries. One 40-byte read. stream: a torch.cuda.Stream
    of the caller's (None: the engine's own)."""
    import torch
    eng = hasher.engine
    n = digests.numel() // 32
    dev = digests.device
    first, group, members = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    cap = int(group_cap)
    group_first = torch.empty(cap, dtype=torch.int32, device=dev) if cap > 0 else None
    group_count = torch.empty(cap, dtype=torch.int32, device=dev) if cap > 0 else None
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    if n == 0:
        return 0, 0, 0, first, group, members, empty, empty
    result = torch.empty(5, dtype=torch.int64, device=dev)
    # stream handling as in verify_batches_device: None, or torch's default stream, means
    # the engine's own stream, and then the whole device is waited for, before and after
    own = not eng._stream_ptr(stream)
    if own:
        torch.cuda.synchronize(dev)
    eng.group_digests_device(digests, first, group, result, scope=scope, members=members, group_first=group_first,
                             group_count=group_count, stream=stream)
    if own or not hasattr(stream, "synchronize"):
        torch.cuda.synchronize(dev)
    else:
        stream.synchronize()
    _, groups, listed, max_count, max_group = (int(x) for x in result.cpu().tolist())
    return (groups, max_count, max_group, first, group, members,
            group_first[:listed] if cap > 0 else empty, group_count[:listed] if cap > 0 else empty)


def tally_into_map_device(dmap, digests, scope=None, quorum: int = 0, crossed_cap: int = 64, stream=None):
    """The same maps filled message by message, over many ActionLists: the n digests of
    this call are counted into `dmap` (GPUHasher.new_device_digest_map), which keeps every
    key's entry id and running count in HBM. digests is a uint8 tensor of 32 n bytes and
    scope an int32 tensor of n entries (None: one map), both on the engine's GPU. Returns
    (entries, added, full, crossed_slots, ids, before, after): the keys the map holds now,
    how many of them are new, whether the call was refused whole because they do not fit,
    the leader slots (ascending, at most crossed_cap) of the keys whose count went from
    below quorum to at least quorum in this call -- the moment agreements :=
    s.prepares[string(s.digest)] reaches someCorrectQuorum / intersectionQuorum -- and per
    slot the key's id and its count before and after. One 64-byte read. stream: a
    torch.cuda.Stream of the caller's (None: the engine's own)."""
    import torch
    eng = dmap._engine
    n = digests.numel() // 32
    dev = digests.device
    ids, before, after = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    cap = int(crossed_cap)
    slots = torch.empty(cap, dtype=torch.int32, device=dev) if cap > 0 else None
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    if n == 0:
        return dmap.size(), 0, False, empty, ids, before, after
    result = torch.empty(8, dtype=torch.int64, device=dev)
    # stream handling as in tally_digests_device: None, or torch's default stream, means
    # the engine's own stream, and then the whole device is waited for, before and after
    own = not eng._stream_ptr(stream)
    if own:
        torch.cuda.synchronize(dev)
    dmap.add_device(digests, ids, result, scope=scope, threshold=quorum, before=before, after=after,
                    crossed_slots=slots, stream=stream)
    if own or not hasattr(stream, "synchronize"):
        torch.cuda.synchronize(dev)
    else:
        stream.synchronize()
    _, entries, added, full, _, listed, _, _ = (int(x) for x in result.cpu().tolist())
    return entries, added, bool(full), slots[:listed] if cap > 0 else empty, ids, before, after


def tally_votes_into_map_device(dmap, digests, voter, scope=None, quorum: int = 0, crossed_cap: int = 64, stream=None):
    """tally_into_map_device for maps that count NODES (the request acks,
    cr.agreements[source] = struct{}{}; a checkpoint's values): slot i is voter[i]'s vote
    for the key (scope[i], digest i), counted into the vote map `dmap`
    (GPUHasher.new_device_vote_map) unless that voter's vote for that key was counted
    before, in this call at a smaller slot or in an earlier one. voter is an int32 tensor
    of n node ids. Returns (entries, added, full, crossed_slots, ids, counted, before,
    after, repeats, bad_voters): as tally_into_map_device, the counts being distinct
    voters, plus per slot whether it was counted, the slots that were a repeat, and the
    slots whose voter the map has no bit for (>= max_voters). One 88-byte read."""
    import torch
    eng = dmap._engine
    n = digests.numel() // 32
    dev = digests.device
    ids, counted, before, after = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    cap = int(crossed_cap)
    slots = torch.empty(cap, dtype=torch.int32, device=dev) if cap > 0 else None
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    if n == 0:
        return dmap.size(), 0, False, empty, ids, counted, before, after, 0, 0
    result = torch.empty(11, dtype=torch.int64, device=dev)
    own = not eng._stream_ptr(stream)       # as in tally_into_map_device
    if own:
        torch.cuda.synchronize(dev)
    dmap.vote_device(digests, voter, ids, result, scope=scope, threshold=quorum, counted=counted, before=before,
                     after=after, crossed_slots=slots, stream=stream)
    if own or not hasattr(stream, "synchronize"):
        torch.cuda.synchronize(dev)
    else:
        stream.synchronize()
    _, entries, added, full, _, listed, _, _, _, repeats, bad = (int(x) for x in result.cpu().tolist())
    return (entries, added, bool(full), slots[:listed] if cap > 0 else empty, ids, counted, before, after,
            repeats, bad)


def dedupe_digests_device(hasher: GPUHasher, digests, stream=None):
    """(table, idx): the distinct digests among the 32 n bytes of `digests`, in order of
    first occurrence, as a [groups, 32] uint8 tensor, and int32 idx with
    table[idx[i]] == digest i -- what Engine.digest_of_digests_device and
    Engine.verify_digests_device(expected_idx=...) take. Everything stays on the GPU; the
    one read is tally_digests_device's 40 bytes (the table's length)."""
    n = digests.numel() // 32
    groups, _, _, _, idx, _, group_first, _ = tally_digests_device(hasher, digests, group_cap=max(n, 1),
                                                                   stream=stream)
    table = digests.view(-1, 32)[group_first[:groups].long()]
    return table, idx


def _epoch_change_aliases(reqs: Sequence[ActionHashRequest]) -> List[int]:
    """alias[i] = an earlier request carrying request i's EpochChange payload,
    else -1 (the Go drop-in's epochChangeAliases, gpuhash.go). Each origin's
    EpochChange is hashed once per ack (epoch_target.go:486-528,
    epoch_tracker.go:349-350). The testengine's acks hold the originator's
    message itself (recorder.go:39-47): the same object is the same payload.
    Acks off the wire hold equal copies: payloads from the same origin node
    with the same length are compared byte for byte (an altered copy is packed
    and hashed on its own), and so is a request whose object was seen before
    but whose Data differs in length."""
    alias = [-1] * len(reqs)
    by_obj: dict = {}       # id(EpochChange) -> request index (objects live as long as reqs)
    by_content: dict = {}   # (origin node, length) -> [(index, payload)]
    for i, r in enumerate(reqs):
        t = r.origin.type if r.origin is not None else None
        if not isinstance(t, HashOriginEpochChange):
            continue
        ec = t.epoch_change
        # the same object names the same payload only if the Data built from it is
        # the same (the contract is SHA-256(Data)): part for part the same object
        # or equal bytes (list == compares identity first), else the joined bytes
        data = None
        if ec is not None and id(ec) in by_obj:
            j = by_obj[id(ec)]
            if reqs[j].data == r.data or b"".join(reqs[j].data) == (data := b"".join(r.data)):
                alias[i] = j
                continue
        if data is None:
            data = b"".join(r.data)
        key = (t.origin, len(data))
        match = next((j for j, d in by_content.get(key, ()) if d == data), -1)
        if ec is not None:
            by_obj[id(ec)] = match if match >= 0 else i
        if match >= 0:
            alias[i] = match
        else:
            by_content.setdefault(key, []).append((i, data))
    return alias


def ProcessHashActions(hasher: GPUHasher, actions: ActionList) -> EventList:
    """processor.ProcessHashActions (serial.go:180-198), one GPU batch per list."""
    if not hasattr(hasher, "hash_requests"):
        raise TypeError("ProcessHashActions needs a GPU-backed hasher (GPUHasher); "
                        "this engine has no CPU hashing path")
    reqs: List[ActionHashRequest] = []
    for action in actions:
        t = action.type
        if not isinstance(t, ActionHash):
            raise ProcessorError(f"unexpected type for Hash action: {type(t).__name__}")
        reqs.append(t.hash)
    digests = hasher.hash_requests(reqs) if reqs else []
    events = EventList()
    for r, d in zip(reqs, digests):
        events.hash_result(d, r.origin)
    return events
