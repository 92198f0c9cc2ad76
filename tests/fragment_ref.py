"""Expected results of smol_csum_batch_fragment_emit, in numpy (include/smolcsum.h).

From the records, the plans, the frame stride and the caps: the smol_csum_fragout_t array and the
destination arena, which starts as a sentinel fill so that a stray store or a missing byte shows.  Per
record: oracle.batch_emit on a copy of the record (the status byte and every checksum), then
tests.pktgen.fragment_like_iface (the iface's cut), then the eligibility, cap and stride rules of the
header.  Nothing here computes a checksum of its own.
"""
from __future__ import annotations

import numpy as np

import oracle
from tests import pktgen as P

KIND_IP, KIND_ETH = 1, 2
SENTINEL = 0xA5

FRAGPLAN_DTYPE = np.dtype([("dst_offset", "<u8"), ("cap", "<u4"), ("ip_mtu", "<u2"), ("ident", "<u2")])
FRAGOUT_DTYPE = np.dtype([("count", "<u4"), ("frame_len", "<u4"), ("last_len", "<u4"), ("status", "u1"), ("written", "u1"),
                          ("reserved", "<u2")])


def emit_record(rec: bytes, kind: int, flags: int, caps):
    """(status byte, record bytes) after smol_csum_batch_emit's oracle on a copy of the record."""
    a = np.frombuffer(rec, np.uint8).copy()
    if a.size == 0:
        return int(oracle.batch_emit(np.zeros(1, np.uint8), None, 1, 0, 0, oracle.kind_flags(kind, flags), caps)[0]), b""
    st = oracle.batch_emit(a, None, 1, a.size, a.size, oracle.kind_flags(kind, flags), caps)
    return int(st[0]), a.tobytes()


def cut_io(rec: bytes, kind: int):
    """The Ethernet bytes in front of the IPv4 header (0 or 14) when the record is one this call cuts (an
    IPv4 header passing Ipv4Packet::check_len, src/wire/ipv4.rs:241-256, IHL 5, not itself a fragment), else
    None."""
    if kind == KIND_ETH:
        if len(rec) < 14 or rec[12:14] != b"\x08\x00":
            return None
        io = 14
    elif kind == KIND_IP:
        io = 0
    else:
        return None
    ip = rec[io:]
    if len(ip) < 20 or ip[0] >> 4 != 4:
        return None
    hl, total = (ip[0] & 15) * 4, int.from_bytes(ip[2:4], "big")
    if len(ip) < hl or hl > total or len(ip) < total or hl < 20:
        return None
    if hl != 20 or int.from_bytes(ip[6:8], "big") & 0x3FFF:
        return None
    return io


def frames_of(rec: bytes, kind: int, flags: int, ip_mtu: int, ident: int, caps):
    """(status, frames): the frames a cut record makes, each with its Ethernet header; frames is None for a
    record that is not cut."""
    st, out = emit_record(rec, kind, flags, caps)
    io = cut_io(rec, kind)
    if io is None or ip_mtu < 28:
        return st, None
    total = int.from_bytes(rec[io + 2:io + 4], "big")
    if total <= ip_mtu:  # the iface sends it as it is (src/iface/interface/mod.rs:1276)
        return st, [out[:io + total]]
    tx = int(caps[0]) in (0, 2)  # Checksum::tx(): Both or Tx
    return st, [out[:io] + f for f in P.fragment_like_iface(out[io:io + total], ip_mtu, ident, fill_header=tx)]


def expected(recs, kinds, flags, plans, frame_stride: int, caps, arena_size: int, sentinel: int = SENTINEL):
    """recs: the records as they stand in the batch (bytes each); kinds / flags: one per record; plans: a
    FRAGPLAN_DTYPE array, one per record.  Returns (out entries, arena)."""
    n = len(recs)
    out = np.zeros(n, FRAGOUT_DTYPE)
    arena = np.full(arena_size, sentinel, np.uint8)
    for i in range(n):
        pl = plans[i]
        st, frames = frames_of(recs[i], int(kinds[i]), int(flags[i]), int(pl["ip_mtu"]), int(pl["ident"]), caps)
        out[i]["status"] = st
        if frames is None:
            continue
        count, frame_len, last_len = len(frames), len(frames[0]), len(frames[-1])
        assert all(len(f) == frame_len for f in frames[:-1])
        out[i]["count"], out[i]["frame_len"], out[i]["last_len"] = count, frame_len, last_len
        S = frame_stride or frame_len
        if (count - 1) * S + last_len > int(pl["cap"]) or (frame_stride and frame_stride < frame_len):
            continue
        out[i]["written"] = 1
        o = int(pl["dst_offset"])
        for k, f in enumerate(frames):
            assert o + k * S + len(f) <= arena_size
            arena[o + k * S:o + k * S + len(f)] = np.frombuffer(f, np.uint8)
    return out, arena
