"""Expected results of smol_csum_batch_verify_reassemble's reassembly, in numpy (include/smolcsum.h).

From the records, the groups and the slots: the smol_csum_dgram_t array and the destination arena, which
starts as a sentinel fill so that a stray store or a missing byte shows.  This restates the fragment-group
contract and PacketAssembler::add's copy (src/iface/fragmentation.rs:139-151); it computes no checksum
and no status byte: those come from oracle.batch_verify_frag.
"""
from __future__ import annotations

import numpy as np

MAX_FRAGMENTS = 256
KIND_IP, KIND_ETH = 1, 2
REC_IPHDR_ONLY = 0x01
SENTINEL = 0xA5

DGRAM_DTYPE = np.dtype([("len", "<u4"), ("l4_len", "<u4"), ("l4_off", "<u2"), ("protocol", "u1"), ("copied", "u1"),
                        ("reserved", "<u4")])


def group_valid(first: int, count: int, reserved: int, n: int) -> bool:
    return first < n and 1 <= count <= MAX_FRAGMENTS and count <= n - first and reserved == 0


def parse_fragment(rec: bytes, kind: int):
    """(key, start, end, more_fragments, payload) of one record, or None when it is no IPv4 packet that
    passes Ipv4Packet::check_len (src/wire/ipv4.rs:241-256)."""
    if kind == KIND_ETH:
        if len(rec) < 14 or rec[12:14] != b"\x08\x00":
            return None
        ip = rec[14:]
    elif kind == KIND_IP:
        ip = rec
    else:
        return None
    if len(ip) < 20 or ip[0] >> 4 != 4:
        return None
    hl, total = (ip[0] & 15) * 4, int.from_bytes(ip[2:4], "big")
    if len(ip) < hl or hl > total or len(ip) < total or hl < 20:
        return None
    ff = int.from_bytes(ip[6:8], "big")
    start = (ff & 0x1FFF) * 8
    key = (ip[4:6], ip[12:16], ip[16:20], ip[9])  # ident, source, destination, protocol (get_key)
    return key, start, start + total - hl, bool(ff & 0x2000), ip[hl:total]


def reassemble_group(recs, kinds):
    """(T, protocol, datagram bytes) of a usable group, else None.  Usable: every record parses, all share
    one key, the non-empty payloads cover [0, T) exactly once, and exactly one fragment has MF clear: the
    one that ends at T."""
    frags = [parse_fragment(r, int(k)) for r, k in zip(recs, kinds)]
    if any(f is None for f in frags) or len({f[0] for f in frags}) != 1:
        return None
    frags.sort(key=lambda f: f[1])
    pos = 0
    for _, start, end, _, _ in frags:  # in offset order each starts where the one before ended
        if start != pos or end <= start:
            return None
        pos = end
    if [f[3] for f in frags] != [True] * (len(frags) - 1) + [False]:
        return None
    return pos, frags[0][0][3], b"".join(f[4] for f in frags)


def l4_span(protocol: int, dgram: bytes, raw: bool):
    """(l4_off, l4_len) of a datagram that reaches the UDP or TCP gate and passes its check_len and port
    tests (UdpPacket::payload udp.rs:153-157, TcpPacket::payload tcp.rs:419-423), else (0, 0)."""
    T = len(dgram)
    if raw:
        return 0, 0
    if protocol == 17 and T >= 8:
        ul = int.from_bytes(dgram[4:6], "big")
        if 8 <= ul <= T and dgram[2:4] != b"\0\0":
            return 8, ul - 8
    if protocol == 6 and T >= 20:
        thl = (dgram[12] >> 4) * 4
        if 20 <= thl <= T and dgram[0:2] != b"\0\0" and dgram[2:4] != b"\0\0":
            return thl, T - thl
    return 0, 0


def expected(recs, kinds, flags, groups, slot_offs, slot_caps, arena_size: int, sentinel: int = SENTINEL):
    """recs: the records as they stand in the batch (bytes each); kinds / flags: one per record; groups:
    (first, count, reserved) each; slot_offs / slot_caps: one per group.  Returns (dgrams, arena)."""
    n = len(recs)
    dg = np.zeros(len(groups), DGRAM_DTYPE)
    arena = np.full(arena_size, sentinel, np.uint8)
    for gi, (first, count, reserved) in enumerate(groups):
        first, count = int(first), int(count)
        if not group_valid(first, count, int(reserved), n):
            continue
        r = reassemble_group(recs[first:first + count], kinds[first:first + count])
        if r is None:
            continue
        T, protocol, data = r
        assert len(data) == T
        raw = any(int(f) & REC_IPHDR_ONLY for f in flags[first:first + count])
        dg[gi]["len"], dg[gi]["protocol"] = T, protocol
        dg[gi]["l4_off"], dg[gi]["l4_len"] = l4_span(protocol, data, raw)
        if T <= int(slot_caps[gi]):
            dg[gi]["copied"] = 1
            o = int(slot_offs[gi])
            arena[o:o + T] = np.frombuffer(data, np.uint8)
    return dg, arena
