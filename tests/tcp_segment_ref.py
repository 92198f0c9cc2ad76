"""Expected results of smol_csum_batch_tcp_segment_emit, in numpy (include/smolcsum.h).

From the header templates, the plans, the payload source, the frame stride and the caps: the
smol_csum_tcpout_t array and the destination arena, which starts as a sentinel fill so that a stray store
or a missing byte shows.  Per record: oracle.batch_emit on a copy of the template (the status byte), the
header's eligibility rules, then per frame the rewritten headers and the payload slice put together here
and oracle.batch_emit on that frame (every checksum); the cap and stride rules and the arena are
tests/cut_ref.py's.  Nothing here computes a checksum of its own.
"""
from __future__ import annotations

import numpy as np

from tests.cut_ref import OUT_DTYPE as TCPOUT_DTYPE
from tests.cut_ref import SENTINEL, emit_record, new_results, place  # noqa: F401  (re-exported)

KIND_IP, KIND_ETH = 1, 2
REC_IPHDR_ONLY = 0x01

TCPPLAN_DTYPE = np.dtype([("src_offset", "<u8"), ("len", "<u4"), ("mss", "<u2"), ("reserved", "<u2"), ("dst_offset", "<u8"),
                          ("cap", "<u4"), ("reserved2", "<u4")])

A4, B4 = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])
A6, B6 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
GARBAGE = 0xBEEF  # what the checksum fields hold before the call: never summed, always overwritten


def template(rng, v6: bool = False, eth: bool = False, doff: int = 5, flags: int = 0x18, seq: int = 0x01020304,
             ns: bool = False, ident: int = 0, tail: bytes = b"") -> bytes:
    """A header template as the stack emits a TCP segment with an empty payload: Ethernet header if asked,
    IPv4 (ident 0, DF, as Ipv4Repr::emit writes them) or IPv6 header, TCP header with random option bytes, the
    checksum fields holding garbage.  tail: bytes behind the headers that the IP length does not count."""
    from tests import pktgen as P

    t = bytearray(P.tcp(4001, 80, b"", csum=GARBAGE, doff=doff, flags=flags, seq=seq, ack=0x0A0B0C0D))
    t[20:] = P.rand_bytes(rng, 4 * doff - 20)
    if ns:
        t[12] |= 0x01
    t[18:20] = b"\x12\x34"  # urgent pointer
    ip = P.ipv6(A6, B6, 6, bytes(t)) if v6 else P.ipv4(A4, B4, 6, bytes(t), ident=ident, csum=GARBAGE)
    return (P.eth(ip, 0x86DD if v6 else 0x0800) if eth else ip) + tail


def not_cut_cases(rng):
    """(name, record, kind, flags, mss, len) for every kind of record the call does not cut."""
    from tests import pktgen as P

    good = template(rng)
    u = P.udp(7, 9, b"")
    t20 = good[20:40]
    hbh = P.ipv6(A6, B6, 0, P.hbh(6, 0, rng) + t20)
    return [
        ("syn", template(rng, flags=0x02), KIND_IP, 0, 536, 100),
        ("syn-ack", template(rng, eth=True, flags=0x12), KIND_ETH, 0, 536, 100),
        ("rst", template(rng, v6=True, flags=0x14), KIND_IP, 0, 536, 100),
        ("udp", P.ipv4(A4, B4, 17, u), KIND_IP, 0, 536, 100),
        ("udp6", P.ipv6(A6, B6, 17, u), KIND_IP, 0, 536, 100),
        ("gre", P.ipv4(A4, B4, 47, t20), KIND_IP, 0, 536, 100),
        ("ihl6", P.ipv4(A4, B4, 6, t20, ihl=6), KIND_IP, 0, 536, 100),
        ("frag-mf", P.ipv4(A4, B4, 6, t20, flags_frag=0x2000), KIND_IP, 0, 536, 100),
        ("frag-off", P.ipv4(A4, B4, 6, t20, flags_frag=0x0010), KIND_IP, 0, 536, 100),
        ("payload", P.ipv4(A4, B4, 6, t20 + b"abcd"), KIND_IP, 0, 536, 100),
        ("payload6", P.eth(P.ipv6(A6, B6, 6, t20 + b"x"), 0x86DD), KIND_ETH, 0, 536, 100),
        ("hbh", hbh, KIND_IP, 0, 536, 100),
        ("raw", good, 0, 0, 536, 100),
        ("arp", P.eth(good, 0x0806), KIND_ETH, 0, 536, 100),
        ("short-tcp", P.ipv4(A4, B4, 6, t20[:12]), KIND_IP, 0, 536, 100),
        ("short-opts", P.ipv4(A4, B4, 6, template(rng, doff=8)[20:44]), KIND_IP, 0, 536, 100),
        ("doff4", P.ipv4(A4, B4, 6, bytes(t20[:12]) + b"\x40" + bytes(t20[13:])), KIND_IP, 0, 536, 100),
        ("total-above", P.ipv4(A4, B4, 6, t20, total_len=41), KIND_IP, 0, 536, 100),
        ("short-ip", good[:19], KIND_IP, 0, 536, 100),
        ("short-eth", P.eth(good)[:13], KIND_ETH, 0, 536, 100),
        ("version5", bytes([0x55]) + good[1:], KIND_IP, 0, 536, 100),
        ("iphdr-only", good, KIND_IP, REC_IPHDR_ONLY, 536, 100),
        ("mss0", good, KIND_IP, 0, 0, 100),
        ("mss0-len0", template(rng, v6=True), KIND_IP, 0, 0, 0),
        ("overflow", template(rng, doff=15), KIND_IP, 0, 65535, 65535),
        ("overflow6", template(rng, v6=True, doff=6), KIND_IP, 0, 65535, 65520),
    ]


def template_geometry(rec: bytes, kind: int, flags: int):
    """(io, fam, thl) when the record is a header template this call cuts, as far as its own bytes say
    (emit's status byte must be 0 besides): TCP straight behind an IPv4 header of IHL 5 or an IPv6 header, the
    L4 length the IP header states equal to the TCP header length, SYN and RST clear; else None."""
    if flags & REC_IPHDR_ONLY:
        return None
    if kind == KIND_ETH:
        if len(rec) < 14 or rec[12:14] not in (b"\x08\x00", b"\x86\xdd"):
            return None
        io = 14
    elif kind == KIND_IP:
        io = 0
    else:
        return None
    ip = rec[io:]
    if len(ip) < 1:
        return None
    if ip[0] >> 4 == 4:
        if len(ip) < 20 or ip[0] & 15 != 5 or ip[9] != 6:
            return None
        fam, ihl, l4len = 4, 20, int.from_bytes(ip[2:4], "big") - 20
    elif ip[0] >> 4 == 6:
        if len(ip) < 40 or ip[6] != 6:
            return None
        fam, ihl, l4len = 6, 40, int.from_bytes(ip[4:6], "big")
    else:
        return None
    if l4len < 20 or len(ip) < ihl + l4len:
        return None
    thl = (ip[ihl + 12] >> 4) * 4
    if thl < 20 or l4len != thl or ip[ihl + 13] & 0x06:
        return None
    return io, fam, thl


def frames_of(rec: bytes, kind: int, flags: int, payload: bytes, mss: int, caps):
    """(status, frames): the frames a cut send makes; frames is None for a record that is not cut.  payload:
    the whole send's bytes."""
    st, _ = emit_record(rec, kind, flags, caps)
    geo = template_geometry(rec, kind, flags)
    n = len(payload)
    if st != 0 or geo is None or mss < 1:
        return st, None
    io, fam, thl = geo
    ihl = 20 if fam == 4 else 40
    if (ihl if fam == 4 else 0) + thl + min(mss, n) > 65535:
        return st, None
    hl, t = io + ihl + thl, io + ihl
    count = max(1, -(-n // mss))
    seq0 = int.from_bytes(rec[t + 4:t + 8], "big")
    frames = []
    for k in range(count):
        part = payload[k * mss:(k + 1) * mss]
        h = bytearray(rec[:hl])
        if fam == 4:
            h[io + 2:io + 4] = (20 + thl + len(part)).to_bytes(2, "big")
        else:
            h[io + 4:io + 6] = (thl + len(part)).to_bytes(2, "big")
        h[t + 4:t + 8] = ((seq0 + k * mss) & 0xFFFFFFFF).to_bytes(4, "big")
        if k + 1 < count:
            h[t + 13] &= ~0x09 & 0xFF  # FIN, PSH: on the last frame only
        fst, f = emit_record(bytes(h) + part, kind, 0, caps)
        assert fst == 0
        frames.append(f)
    return st, frames


def expected(recs, kinds, flags, plans, src, frame_stride: int, caps, arena_size: int, sentinel: int = SENTINEL):
    """recs: the templates as they stand in the batch (bytes each); kinds / flags: one per record; plans: a
    TCPPLAN_DTYPE array, one per record; src: the payload source (uint8 array).  Returns (out entries, arena)."""
    out, arena = new_results(len(recs), arena_size, sentinel)
    for i, pl in enumerate(plans):
        so, ln = int(pl["src_offset"]), int(pl["len"])
        # (a plan of a record that is not cut may name anything: it is cut as if it named nothing)
        payload = bytes(src[so:so + ln]) if so + ln <= len(src) else b""
        st, frames = frames_of(recs[i], int(kinds[i]), int(flags[i]), payload, int(pl["mss"]), caps)
        assert so + ln <= len(src) or frames is None
        place(out, arena, i, st, frames, pl, frame_stride)
    return out, arena
