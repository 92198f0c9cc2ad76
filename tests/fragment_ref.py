"""Expected results of smol_csum_batch_fragment_emit, in numpy (include/smolcsum.h).

From the records, the plans, the frame stride and the caps: the smol_csum_fragout_t array and the
destination arena, which starts as a sentinel fill so that a stray store or a missing byte shows.  Per
record: oracle.batch_emit on a copy of the record (the status byte and every checksum), then
tests.pktgen.fragment_like_iface (the iface's cut) and the eligibility rules of the header; the cap and
stride rules and the arena are tests/cut_ref.py's.  Nothing here computes a checksum of its own.
"""
from __future__ import annotations

import numpy as np

from tests import pktgen as P
from tests.cut_ref import OUT_DTYPE as FRAGOUT_DTYPE
from tests.cut_ref import SENTINEL, emit_record, new_results, place  # noqa: F401  (re-exported)

KIND_IP, KIND_ETH = 1, 2

FRAGPLAN_DTYPE = np.dtype([("dst_offset", "<u8"), ("cap", "<u4"), ("ip_mtu", "<u2"), ("ident", "<u2")])


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
    out, arena = new_results(len(recs), arena_size, sentinel)
    for i, pl in enumerate(plans):
        st, frames = frames_of(recs[i], int(kinds[i]), int(flags[i]), int(pl["ip_mtu"]), int(pl["ident"]), caps)
        place(out, arena, i, st, frames, pl, frame_stride)
    return out, arena
