"""Expected results of smol_csum_batch_verify_unreach_reply: this file's own restatement, in Python, of the
REFUSED rule, the address rule and the error frame's head of include/smolcsum.h.  No checksum is computed here:
the status bytes are the oracle's verify, and every reply checksum is the oracle's emit run on the frame built
here with zero checksum fields, under the same caps."""
from __future__ import annotations

import numpy as np

import oracle
from smoltcp_amd import engine as E
from tests import pktgen as P
from tests.cut_ref import SENTINEL
from tests.echo_ref import _hbh_drops, nonuni4, nonuni6

REFUSED, ANSWERED, WRITTEN, SEND, HOST, PORT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20  # SMOL_UNR_*
UNR_DTYPE = np.dtype([("frame_len", "<u4"), ("data_off", "<u2"), ("head_len", "u1"), ("flags", "u1")])
DATA_V4, DATA_V6 = 528, 1192  # icmp_reply_payload_len(len, IPV4_MIN_MTU | IPV6_MIN_MTU, 20 | 40)


def port_open(port_map, p: int) -> bool:
    return bool(port_map[p >> 3] >> (p & 7) & 1)


def _udp_ok(rec, l4: int, l4_len: int) -> bool:
    """UdpPacket::check_len and the destination-port test of UdpRepr::parse."""
    if l4_len < 8:
        return False
    ul = rec[l4 + 4] << 8 | rec[l4 + 5]
    return 8 <= ul <= l4_len and (rec[l4 + 2] | rec[l4 + 3]) != 0


def refusal_of(rec: bytes, kind: int, flags: int = 0, port_map=None):
    """(ver, ip offset, data offset, P, protocol / next header reached, hbh, port form) of a record the
    interface refuses, else None.  port_map: None, or the 8192 bytes of d_udp_open."""
    n, ip = len(rec), 0
    if kind == E.KIND_ETH:
        if n < 15:
            return None
        et = rec[12] << 8 | rec[13]
        if et not in (0x0800, 0x86DD) or rec[14] >> 4 != (4 if et == 0x0800 else 6):
            return None
        ip = 14
    elif kind != E.KIND_IP:
        return None
    lb = n - ip
    if lb < 1 or flags & E.REC_IPHDR_ONLY:
        return None
    ver = rec[ip] >> 4
    hbh = False
    if ver == 4:
        if lb < 20:
            return None
        hl, total = (rec[ip] & 15) * 4, rec[ip + 2] << 8 | rec[ip + 3]
        if hl < 20 or hl > total or lb < total:
            return None
        if (rec[ip + 6] << 8 | rec[ip + 7]) & 0x3FFF:  # more fragments, or a fragment offset
            return None
        proto, off, plen = rec[ip + 9], ip + hl, total - hl
        l4, l4_len = off, plen
    elif ver == 6:
        if lb < 40:
            return None
        plen = rec[ip + 4] << 8 | rec[ip + 5]
        if lb < 40 + plen:
            return None
        proto, off = rec[ip + 6], ip + 40
        l4, l4_len = off, plen
        if proto == 0:
            if l4_len < 8:
                return None
            ext = (rec[l4 + 1] + 1) * 8
            if l4_len < ext or _hbh_drops(rec, l4 + 2, l4 + ext):
                return None
            hbh, proto, l4, l4_len = True, rec[l4], l4 + ext, l4_len - ext
    else:
        return None
    closed = (proto == 17 and port_map is not None and _udp_ok(rec, l4, l4_len)
              and not port_open(port_map, rec[l4 + 2] << 8 | rec[l4 + 3]))
    port = form_of(ver, proto, hbh, closed)
    return None if port is None else (ver, ip, off, plen, proto, hbh, port)


def form_of(ver: int, proto: int, hbh: bool, udp_closed: bool):
    """Which refusal a record of this protocol / next header (the one reached behind a leading Hop-by-Hop
    header when hbh) meets: True the port form, False the protocol / next-header form, None neither.
    udp_closed: a well-formed UDP datagram whose destination port's bit in the port map is clear."""
    if proto == 17:
        return True if udp_closed else None
    if ver == 4:
        return None if proto in (1, 2, 6) else False
    # (the header's own 0 is the Hop-by-Hop header hbh names; reached behind one it is unrecognised)
    return None if proto in (6, 58) or (proto == 0 and not hbh) else False


def rule(kind: int, ver: int, mac_dst: bytes, mac_src: bytes, src: bytes, dst: bytes, hbh: bool, port: bool, bcast=None):
    """(SMOL_UNR_* flags, ICMP type, code) of a refused record under the wire-level address rule: REFUSED, PORT
    for the UDP form, and ANSWERED or HOST or neither."""
    f = REFUSED | (PORT if port else 0)
    t, c = ((3, 3) if port else (3, 2)) if ver == 4 else ((1, 4) if port else (4, 1))
    if ver == 4:
        if nonuni4(src, bcast) or nonuni4(dst, bcast):
            return f, t, c
        f |= ANSWERED
    else:
        if nonuni6(src):
            return f, t, c
        f |= HOST if nonuni6(dst) or hbh else ANSWERED
    if kind == E.KIND_ETH and f & ANSWERED and (mac_dst[0] | mac_src[0]) & 1:
        f = f & ~ANSWERED | HOST
    return f, t, c


def head(kind: int, ver: int, mac_dst: bytes, mac_src: bytes, ethertype: bytes, src: bytes, dst: bytes, hop: int, proto: int,
         plen: int, t: int, c: int) -> bytes:
    """The error frame's bytes in front of the data, every checksum field zero.  The arguments are the REQUEST's."""
    dlen = min(plen, DATA_V4 if ver == 4 else DATA_V6)
    h = (mac_src + mac_dst + ethertype) if kind == E.KIND_ETH else b""
    if ver == 4:
        h += bytes([0x45, 0]) + P.be16(48 + dlen) + bytes([0, 0, 0x40, 0, 64, 1, 0, 0]) + dst + src
        h += bytes([t, c, 0, 0, 0, 0, 0, 0])
        h += bytes([0x45, 0]) + P.be16(20 + plen) + bytes([0, 0, 0x40, 0, hop, proto, 0, 0]) + src + dst
    else:
        h += bytes([0x60, 0, 0, 0]) + P.be16(48 + dlen) + bytes([58, 64]) + dst + src
        h += bytes([t, c, 0, 0, 0, 0, 0, 40 if t == 4 else 0])
        h += bytes([0x60, 0, 0, 0]) + P.be16(plen) + bytes([proto, hop]) + src + dst
    return h


def reply_of(rec: bytes, kind: int, flags: int = 0, port_map=None, bcast=None):
    """(SMOL_UNR_* flags of the rules, data offset, error frame with zero checksum fields or None, head length)."""
    rf = refusal_of(rec, kind, flags, port_map)
    if rf is None:
        return 0, 0, None, 0
    ver, ip, off, plen, proto, hbh, port = rf
    al = 4 if ver == 4 else 16
    a0 = ip + (12 if ver == 4 else 8)
    src, dst = rec[a0:a0 + al], rec[a0 + al:a0 + 2 * al]
    f, t, c = rule(kind, ver, rec[0:6], rec[6:12], src, dst, hbh, port, bcast)
    if not f & ANSWERED:
        return f, off, None, 0
    h = head(kind, ver, rec[0:6], rec[6:12], rec[12:14], src, dst, rec[ip + (8 if ver == 4 else 7)], proto, plen, t, c)
    return f, off, h + rec[off:off + min(plen, DATA_V4 if ver == 4 else DATA_V6)], len(h)


def frame_lens(records, kinds, flags, port_map, cfg):
    """The error frame's length per record (0: not answered), to size the slots of a test before expected()."""
    n = len(records)
    kinds = np.broadcast_to(np.asarray(kinds, np.uint8), (n,))
    flags = np.broadcast_to(np.asarray(flags, np.uint8), (n,))
    out = np.zeros(n, np.int64)
    for i, r in enumerate(records):
        frame = reply_of(r, int(kinds[i]), int(flags[i]), port_map, cfg)[2]
        out[i] = len(frame) if frame is not None else 0
    return out


def expected(records, kinds, flags, caps, cfg, port_map, slots, arena_size: int):
    """(status, entries, arena) of one call.  records: the records as they stand in the batch; kinds / flags:
    per record; caps: the five smol_checksum_t values; cfg: None or the 4 bytes of bcast_v4; port_map: None or
    the 8192 bytes of d_udp_open; slots: an E.SLOT_DTYPE array; the arena starts filled with the sentinel."""
    n = len(records)
    kinds = np.broadcast_to(np.asarray(kinds, np.uint8), (n,))
    flags = np.broadcast_to(np.asarray(flags, np.uint8), (n,))
    buf, offs, lens = P.pack(records)
    status = oracle.batch_verify(buf, E.make_descriptors(offs, lens, kinds, flags), n, caps=caps) if n else np.zeros(0, np.uint8)
    entries = np.zeros(n, UNR_DTYPE)
    arena = np.full(arena_size, SENTINEL, np.uint8)
    frames, owners = [], []
    for i, r in enumerate(records):
        f, doff, frame, hl = reply_of(r, int(kinds[i]), int(flags[i]), port_map, cfg)
        if f:
            assert not status[i] & E.ST_MALFORMED, "refusal_of and the oracle's parse disagree"
            assert bool(status[i] & E.ST_UNSUPPORTED) == (not f & PORT), "refusal_of and the oracle's parse disagree"
        entries[i]["flags"], entries[i]["data_off"], entries[i]["head_len"] = f, doff, hl
        if frame is not None:
            frames.append(frame)
            owners.append(i)
    if frames:
        fb, fo, fl = P.pack(frames)
        est = oracle.batch_emit(fb, E.make_descriptors(fo, fl, kinds[owners], 0), len(frames), caps=caps)
        assert not (est & (E.ST_MALFORMED | E.ST_UNSUPPORTED)).any(), "an error frame the oracle's emit rejects"
        for i, o, ln in zip(owners, fo, fl):
            ln = int(ln)
            e = entries[i]
            e["frame_len"] = ln
            if ln <= int(slots[i]["cap"]):
                d = int(slots[i]["dst_offset"])
                assert d + ln <= arena_size
                arena[d:d + ln] = fb[int(o):int(o) + ln]
                e["flags"] |= WRITTEN | (SEND if status[i] & E.ST_ACCEPT else 0)
    return status, entries, arena
