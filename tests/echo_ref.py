"""Expected results of smol_csum_batch_verify_echo_reply: this file's own restatement, in Python, of the
REQUEST rule, the address rule and the reply head of include/smolcsum.h.  No checksum is computed here: the
status bytes are the oracle's verify, and every reply checksum is the oracle's emit run on the reply frame
built here with zero checksum fields, under the same caps."""
from __future__ import annotations

import numpy as np

import oracle
from smoltcp_amd import engine as E
from tests import pktgen as P
from tests.cut_ref import SENTINEL

REQUEST, ANSWERED, WRITTEN, SEND, HOST = 0x01, 0x02, 0x04, 0x08, 0x10  # SMOL_ECHO_*
ECHO_DTYPE = np.dtype([("frame_len", "<u4"), ("data_off", "<u2"), ("head_len", "u1"), ("flags", "u1")])


def _hbh_drops(rec, pos: int, end: int) -> bool:
    """process_hopbyhop (src/iface/interface/ipv6.rs:282-313) over the option bytes [pos, end)."""
    for i in range(5):
        if pos >= end:
            break
        t = rec[pos]
        if t == 0:
            pos += 1
            continue
        if end - pos == 1:
            return True
        dl = rec[pos + 1]
        if end - pos < 2 + dl or (t == 5 and dl != 2):
            return True
        if i < 4 and t not in (1, 5) and t & 0xC0:
            return True
        pos += 2 + dl
    return False


def request_of(rec: bytes, kind: int, flags: int = 0):
    """(ver, ip offset, L4 offset, data length) of a record that is an echo request, else None: the record
    reaches the ICMPv4 / ICMPv6 gate with no check_len, version, ethertype, fragment, SMOL_REC_IPHDR_ONLY or
    Hop-by-Hop rejection on the way, the type is 8 / 128 and the code 0.  The L4 buffer is IPv4 total
    length - IHL * 4, or the IPv6 payload length less a leading Hop-by-Hop header."""
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
    if ver == 4:
        if lb < 20:
            return None
        hl, total = (rec[ip] & 15) * 4, rec[ip + 2] << 8 | rec[ip + 3]
        if hl < 20 or hl > total or lb < total:
            return None
        if (rec[ip + 6] << 8 | rec[ip + 7]) & 0x3FFF:  # more fragments, or a fragment offset
            return None
        proto, l4, l4_len, want = rec[ip + 9], ip + hl, total - hl, (1, 8)
    elif ver == 6:
        if lb < 40:
            return None
        plen = rec[ip + 4] << 8 | rec[ip + 5]
        if lb < 40 + plen:
            return None
        proto, l4, l4_len, want = rec[ip + 6], ip + 40, plen, (58, 128)
        if proto == 0:
            if l4_len < 8:
                return None
            ext = (rec[l4 + 1] + 1) * 8
            if l4_len < ext or _hbh_drops(rec, l4 + 2, l4 + ext):
                return None
            proto, l4, l4_len = rec[l4], l4 + ext, l4_len - ext
    else:
        return None
    if proto != want[0] or l4_len < 8 or rec[l4] != want[1] or rec[l4 + 1] != 0:
        return None
    return ver, ip, l4, l4_len - 8


def bcast4(a: bytes, bcast) -> bool:
    return a == b"\xff\xff\xff\xff" or (bcast is not None and any(bcast) and a == bytes(bcast))


def nonuni4(a: bytes, bcast) -> bool:
    return bcast4(a, bcast) or a[0] >> 4 == 0xE or a == bytes(4)


def nonuni6(a: bytes) -> bool:
    return a[0] == 0xFF or a == bytes(16)


def rule(kind: int, ver: int, mac_dst: bytes, mac_src: bytes, src: bytes, dst: bytes, bcast=None) -> int:
    """The SMOL_ECHO_* flags of an echo request under the wire-level address rule: REQUEST, and ANSWERED or
    HOST or neither."""
    f = REQUEST
    if ver == 4:
        if nonuni4(src, bcast):
            return f
        if not nonuni4(dst, bcast):
            f |= ANSWERED
        elif bcast4(dst, bcast):
            f |= HOST
        else:
            return f
    else:
        if nonuni6(src):
            return f
        f |= HOST if nonuni6(dst) else ANSWERED
    if kind == E.KIND_ETH and f & ANSWERED and (mac_dst[0] | mac_src[0]) & 1:
        f = f & ~ANSWERED | HOST
    return f


def head(kind: int, ver: int, mac_dst: bytes, mac_src: bytes, ethertype: bytes, src: bytes, dst: bytes, idseq: bytes,
         dlen: int) -> bytes:
    """The reply's bytes in front of the data, both checksum fields zero.  The arguments are the REQUEST's."""
    h = (mac_src + mac_dst + ethertype) if kind == E.KIND_ETH else b""
    if ver == 4:
        h += bytes([0x45, 0]) + P.be16(28 + dlen) + bytes([0, 0, 0x40, 0, 64, 1, 0, 0]) + dst + src + bytes([0, 0, 0, 0])
    else:
        h += bytes([0x60, 0, 0, 0]) + P.be16(8 + dlen) + bytes([58, 64]) + dst + src + bytes([129, 0, 0, 0])
    return h + idseq


def reply_of(rec: bytes, kind: int, flags: int = 0, bcast=None):
    """(SMOL_ECHO_* flags of the address rule, data offset, reply frame with zero checksum fields or None)."""
    rq = request_of(rec, kind, flags)
    if rq is None:
        return 0, 0, None
    ver, ip, l4, dlen = rq
    al = 4 if ver == 4 else 16
    a0 = ip + (12 if ver == 4 else 8)
    src, dst = rec[a0:a0 + al], rec[a0 + al:a0 + 2 * al]
    f = rule(kind, ver, rec[0:6], rec[6:12], src, dst, bcast)
    if not f & ANSWERED:
        return f, l4 + 8, None
    h = head(kind, ver, rec[0:6], rec[6:12], rec[12:14], src, dst, rec[l4 + 4:l4 + 8], dlen)
    return f, l4 + 8, h + rec[l4 + 8:l4 + 8 + dlen]


def frame_lens(records, kinds, flags, cfg):
    """The reply's length per record (0: not answered), to size the slots of a test before expected()."""
    n = len(records)
    kinds = np.broadcast_to(np.asarray(kinds, np.uint8), (n,))
    flags = np.broadcast_to(np.asarray(flags, np.uint8), (n,))
    out = np.zeros(n, np.int64)
    for i, r in enumerate(records):
        frame = reply_of(r, int(kinds[i]), int(flags[i]), cfg)[2]
        out[i] = len(frame) if frame is not None else 0
    return out


def expected(records, kinds, flags, caps, cfg, slots, arena_size: int):
    """(status, entries, arena) of one call.  records: the records as they stand in the batch; kinds / flags:
    per record; caps: the five smol_checksum_t values; cfg: None or the 4 bytes of bcast_v4; slots: an
    E.SLOT_DTYPE array; the arena starts filled with the sentinel."""
    n = len(records)
    kinds = np.broadcast_to(np.asarray(kinds, np.uint8), (n,))
    flags = np.broadcast_to(np.asarray(flags, np.uint8), (n,))
    buf, offs, lens = P.pack(records)
    status = oracle.batch_verify(buf, E.make_descriptors(offs, lens, kinds, flags), n, caps=caps) if n else np.zeros(0, np.uint8)
    entries = np.zeros(n, ECHO_DTYPE)
    arena = np.full(arena_size, SENTINEL, np.uint8)
    frames, owners = [], []
    for i, r in enumerate(records):
        f, doff, frame = reply_of(r, int(kinds[i]), int(flags[i]), cfg)
        if f:
            assert not status[i] & (E.ST_MALFORMED | E.ST_UNSUPPORTED), "request_of and the oracle's parse disagree"
        entries[i]["flags"], entries[i]["data_off"] = f, doff
        if frame is not None:
            frames.append(frame)
            owners.append(i)
    if frames:
        fb, fo, fl = P.pack(frames)
        est = oracle.batch_emit(fb, E.make_descriptors(fo, fl, kinds[owners], 0), len(frames), caps=caps)
        assert not (est & (E.ST_MALFORMED | E.ST_UNSUPPORTED)).any(), "a reply frame the oracle's emit rejects"
        for i, o, ln in zip(owners, fo, fl):
            ln = int(ln)
            e = entries[i]
            ver = 4 if kinds[i] == E.KIND_IP and fb[int(o)] >> 4 == 4 or kinds[i] == E.KIND_ETH and fb[int(o) + 14] >> 4 == 4 else 6
            e["frame_len"], e["head_len"] = ln, (14 if kinds[i] == E.KIND_ETH else 0) + (20 if ver == 4 else 40) + 8
            if ln <= int(slots[i]["cap"]):
                d = int(slots[i]["dst_offset"])
                assert d + ln <= arena_size
                arena[d:d + ln] = fb[int(o):int(o) + ln]
                e["flags"] |= WRITTEN | (SEND if status[i] & E.ST_ACCEPT else 0)
    return status, entries, arena
