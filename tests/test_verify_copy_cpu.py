"""CPU-side checks of verify_copy (smol_csum_batch_verify_copy): the symbol, the slot and span structs in
their three spellings (C, ctypes, numpy), the argument errors, and `expected_span`, this file's own
restatement of the span rule of include/smolcsum.h, which the GPU tests (tests/test_gpu_verify_copy.py)
take their expected spans from.  No kernel is launched here."""
import ctypes
import json
import os
import re
import subprocess
import tempfile

import numpy as np

import smoltcp_amd
from smoltcp_amd import _lib
from smoltcp_amd import engine as E
from tests import pktgen as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V4A, V4B = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
V6A = bytes(range(0x20, 0x30))
V6B = bytes(range(0x40, 0x50))


def _hbh_drops(rec, pos: int, end: int) -> bool:
    """process_hopbyhop (src/iface/interface/ipv6.rs:282-313) over the option bytes [pos, end): an
    option that fails Ipv6Option::check_len or Repr::parse, or one of the first four whose unknown
    type asks for a discard, drops the packet; the fifth option ends the walk."""
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


def expected_span(rec: bytes, kind: int, flags: int = 0):
    """The payload span (off, len) of one record, or None when it has none: the record reaches the UDP
    or TCP gate and verify's parse rejects it nowhere (every check_len, the version and ethertype tests,
    fragments, SMOL_REC_IPHDR_ONLY, Hop-by-Hop drops, the port-0 rejections).  UDP: UdpPacket::payload
    (udp.rs:153-157), the length field's bytes after the 8-byte header; TCP: TcpPacket::payload
    (tcp.rs:419-423), the L4 buffer after the data offset.  The L4 buffer is IPv4 total length - IHL * 4,
    or the IPv6 payload length less a leading Hop-by-Hop header."""
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
    if lb < 1:
        return None
    ver = rec[ip] >> 4
    if ver == 4:
        if lb < 20:
            return None
        hl, total = (rec[ip] & 15) * 4, rec[ip + 2] << 8 | rec[ip + 3]
        if hl < 20 or hl > total or lb < total or flags & E.REC_IPHDR_ONLY:
            return None
        if (rec[ip + 6] << 8 | rec[ip + 7]) & 0x3FFF:  # more fragments, or a fragment offset
            return None
        proto, l4, l4_len = rec[ip + 9], ip + hl, total - hl
    elif ver == 6:
        if lb < 40:
            return None
        plen = rec[ip + 4] << 8 | rec[ip + 5]
        if lb < 40 + plen or flags & E.REC_IPHDR_ONLY:
            return None
        proto, l4, l4_len = rec[ip + 6], ip + 40, plen
        if proto == 0:
            if l4_len < 8:
                return None
            ext = (rec[l4 + 1] + 1) * 8
            if l4_len < ext or _hbh_drops(rec, l4 + 2, l4 + ext):
                return None
            proto, l4, l4_len = rec[l4], l4 + ext, l4_len - ext
    else:
        return None
    if proto == 17:
        if l4_len < 8:
            return None
        ul = rec[l4 + 4] << 8 | rec[l4 + 5]
        if ul < 8 or l4_len < ul or (rec[l4 + 2] | rec[l4 + 3]) == 0:
            return None
        return l4 + 8, ul - 8
    if proto == 6:
        if l4_len < 20:
            return None
        thl = (rec[l4 + 12] >> 4) * 4
        if thl < 20 or l4_len < thl or (rec[l4] | rec[l4 + 1]) == 0 or (rec[l4 + 2] | rec[l4 + 3]) == 0:
            return None
        return l4 + thl, l4_len - thl
    return None


def test_symbol_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = smoltcp_amd.lib()
    name = "smol_csum_batch_verify_copy"
    assert re.search(r"\b%s\s*\(" % name, text)
    assert hasattr(L, name) and name in _lib.ABI_SYMBOLS
    assert "smol_csum_slot_t" in text and "smol_csum_span_t" in text
    assert L.smol_csum_abi_version() == 6  # additive: the version stays


_C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "smolcsum.h"
int main(void) {
    smol_csum_slot_t s;
    smol_csum_span_t p;
    memset(&s, 0, sizeof s);
    memset(&p, 0, sizeof p);
    s.dst_offset = 0x0807060504030201ull, s.cap = 0x0c0b0a09u, s.reserved = 0x100f0e0du;
    p.len = 0x04030201u, p.off = 0x0605, p.copied = 7, p.reserved = 8;
    printf("{\"slot\": %zu, \"span\": %zu, \"slot_bytes\": [", sizeof s, sizeof p);
    for (size_t i = 0; i < sizeof s; ++i) printf("%s%u", i ? ", " : "", ((unsigned char*)&s)[i]);
    printf("], \"span_bytes\": [");
    for (size_t i = 0; i < sizeof p; ++i) printf("%s%u", i ? ", " : "", ((unsigned char*)&p)[i]);
    printf("]}\n");
    return 0;
}
"""


def test_structs_are_16_and_8_bytes_in_every_spelling():
    """C (compiled from the header), ctypes and numpy agree on size and field order: each struct filled
    so that its bytes count 1, 2, 3, ... in memory order."""
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        with open(src, "w") as f:
            f.write(_C_PROBE)
        subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src],
                       check=True)
        c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert c["slot"] == 16 and c["span"] == 8
    assert c["slot_bytes"] == list(range(1, 17)) and c["span_bytes"] == list(range(1, 9))
    assert ctypes.sizeof(_lib.SlotC) == 16 == E.SLOT_DTYPE.itemsize
    assert ctypes.sizeof(_lib.SpanC) == 8 == E.SPAN_DTYPE.itemsize
    s = _lib.SlotC(0x0807060504030201, 0x0C0B0A09, 0x100F0E0D)
    p = _lib.SpanC(0x04030201, 0x0605, 7, 8)
    assert list(bytes(s)) == list(range(1, 17)) and list(bytes(p)) == list(range(1, 9))
    a = np.frombuffer(bytes(s), dtype=E.SLOT_DTYPE)[0]
    assert (int(a["dst_offset"]), int(a["cap"]), int(a["reserved"])) == (0x0807060504030201, 0x0C0B0A09, 0x100F0E0D)
    b = np.frombuffer(bytes(p), dtype=E.SPAN_DTYPE)[0]
    assert (int(b["len"]), int(b["off"]), int(b["copied"]), int(b["reserved"])) == (0x04030201, 0x0605, 7, 8)
    m = E.make_slots([5, 1 << 40], [7, 9])
    assert m.dtype == E.SLOT_DTYPE and list(m["dst_offset"]) == [5, 1 << 40] and list(m["cap"]) == [7, 9]
    assert not m["reserved"].any() and list(E.make_slots([1, 2, 3], 64)["cap"]) == [64, 64, 64]


def test_verify_copy_argument_errors():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 1, 64, 64, 1
    caps = _lib.Caps()
    buf = (ctypes.c_uint8 * 64)()
    dst = (ctypes.c_uint8 * 64)()
    st = (ctypes.c_uint8 * 8)()
    raw = (ctypes.c_uint8 * 64)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: slots at al, spans at al + 16
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = L.smol_csum_batch_verify_copy
    B, C = ctypes.byref(b), ctypes.byref(caps)
    EINVAL = _lib.SMOL_EINVAL
    assert call(None, buf, B, C, dst, al, st, al + 16, None) == EINVAL  # NULL ctx
    assert call(ctx, buf, B, None, dst, al, st, al + 16, None) == EINVAL  # NULL caps
    assert call(ctx, buf, B, C, None, al, st, al + 16, None) == EINVAL  # NULL d_dst
    assert call(ctx, buf, B, C, dst, None, st, al + 16, None) == EINVAL  # NULL d_slots
    assert call(ctx, buf, B, C, dst, al, None, al + 16, None) == EINVAL  # NULL d_status
    assert call(ctx, buf, B, C, dst, al, st, None, None) == EINVAL  # NULL d_spans
    assert call(ctx, buf, B, C, dst, al + 8, st, al + 16, None) == EINVAL  # d_slots not 16-byte aligned
    assert call(ctx, buf, B, C, dst, al, st, al + 20, None) == EINVAL  # d_spans not 8-byte aligned
    assert call(ctx, None, B, C, dst, al, st, al + 16, None) == EINVAL  # NULL d_buf
    bad = _lib.Caps()
    bad.tcp = 4
    assert call(ctx, buf, B, ctypes.byref(bad), dst, al, st, al + 16, None) == EINVAL  # bad caps value
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as verify
    assert call(ctx, buf, B, C, dst, al, st, al + 16, None) == _lib.SMOL_ERANGE
    assert L.smol_csum_batch_verify(ctx, buf, B, C, st, None) == _lib.SMOL_ERANGE
    b.len, b.n = 64, 0  # nothing to do: OK whatever the arrays are, nothing launched
    assert call(ctx, None, B, C, None, None, None, None, None) == _lib.SMOL_OK
    assert L.smol_csum_tool_set_vcopy_stores(None, 0) == EINVAL


def _cases(rng):
    """(record, kind, payload offset, payload) of well-formed UDP / TCP packets over IPv4 / IPv6."""
    out = []
    for i in range(120):
        pay = P.rand_bytes(rng, int(rng.integers(0, 300)))
        ihl, doff = 5 + i % 11, 5 + (i // 3) % 11
        opts = bytes([1]) * (ihl * 4 - 20)  # IPv4 NOP options
        m = i % 6
        if m == 0:
            r, off = P.ipv4(V4A, V4B, 17, P.udp(7 + i, 9, pay), ihl=ihl, options=opts), ihl * 4 + 8
        elif m == 1:
            r, off = P.ipv4(V4A, V4B, 6, P.tcp(7 + i, 9, pay, doff=doff), ihl=ihl, options=opts), ihl * 4 + doff * 4
        elif m == 2:
            r, off = P.ipv6(V6A, V6B, 17, P.udp(7 + i, 9, pay)), 48
        elif m == 3:
            r, off = P.ipv6(V6A, V6B, 6, P.tcp(7 + i, 9, pay, doff=doff)), 40 + doff * 4
        elif m == 4:
            hb = P.hbh(17, i % 40, rng)
            r, off = P.ipv6(V6A, V6B, 0, hb + P.udp(7 + i, 9, pay)), 40 + len(hb) + 8
        else:
            hb = P.hbh(6, i % 40, rng)
            r, off = P.ipv6(V6A, V6B, 0, hb + P.tcp(7 + i, 9, pay, doff=doff)), 40 + len(hb) + doff * 4
        out.append((r, E.KIND_IP, off, pay))
        out.append((P.eth(r, 0x0800 if r[0] >> 4 == 4 else 0x86DD), E.KIND_ETH, off + 14, pay))
    return out


def test_expected_span_returns_the_payload_pktgen_put_in():
    rng = np.random.default_rng(5)
    for r, kind, off, pay in _cases(rng):
        sp = expected_span(r, kind)
        assert sp == (off, len(pay)), (sp, off, len(pay))
        assert r[sp[0]:sp[0] + sp[1]] == pay


def test_expected_span_follows_the_length_fields_not_the_record():
    pay = bytes(range(40))
    short = P.ipv4(V4A, V4B, 17, P.udp(7, 9, pay, length=8 + 25))  # the UDP length field ends early
    assert expected_span(short, E.KIND_IP) == (28, 25)
    padded = P.eth(P.ipv4(V4A, V4B, 6, P.tcp(7, 9, b"xyz"))) + bytes(17)  # Ethernet padding to 60 bytes
    assert len(padded) == 74 and expected_span(padded, E.KIND_ETH) == (54, 3)
    assert expected_span(P.ipv4(V4A, V4B, 17, P.udp(7, 9, b"")), E.KIND_IP) == (28, 0)


def test_expected_span_none_on_rejected_records(golden):
    pay = bytes(range(64))
    u4 = P.ipv4(V4A, V4B, 17, P.udp(7, 9, pay))
    none = [
        (P.ipv4(V4A, V4B, 17, P.udp(7, 0, pay)), E.KIND_IP, 0),           # destination port 0
        (P.ipv4(V4A, V4B, 6, P.tcp(0, 9, pay)), E.KIND_IP, 0),            # source port 0
        (P.ipv4(V4A, V4B, 17, P.udp(7, 9, pay, length=8 + 65)), E.KIND_IP, 0),  # UDP length past the buffer
        (P.ipv4(V4A, V4B, 6, P.tcp(7, 9, b"", doff=5)[:-4]), E.KIND_IP, 0),     # truncated TCP header
        (u4[:-1], E.KIND_IP, 0),                                          # record shorter than total length
        (P.ipv4(V4A, V4B, 17, P.udp(7, 9, pay), flags_frag=0x2000), E.KIND_IP, 0),  # first fragment
        (P.ipv4(V4A, V4B, 17, P.udp(7, 9, pay), flags_frag=0x0010), E.KIND_IP, 0),  # later fragment
        (P.ipv4(V4A, V4B, 1, P.icmp_echo(8, pay)), E.KIND_IP, 0),
        (P.ipv4(V4A, V4B, 2, bytes(8)), E.KIND_IP, 0),
        (P.ipv6(V6A, V6B, 58, P.icmp_echo(128, pay)), E.KIND_IP, 0),
        (u4, E.KIND_IP, E.REC_IPHDR_ONLY),
        (u4, E.KIND_RAW, 0),
        (P.eth(u4, 0x0806), E.KIND_ETH, 0),                               # ARP ethertype
        (P.eth(u4, 0x86DD), E.KIND_ETH, 0),                               # ethertype / version mismatch
        (P.ipv6(V6A, V6B, 0, P.hbh_opts(17, bytes([0xC2, 0])) + P.udp(7, 9, pay)), E.KIND_IP, 0),  # Hop-by-Hop drop
    ]
    for r, kind, flags in none:
        assert expected_span(r, kind, flags) is None
    assert expected_span(u4, E.KIND_IP) == (28, 64)
    seen = 0
    for f in golden["fuzz_corpus_frames"]:
        r = bytes.fromhex(f["bytes"])
        sp = expected_span(r, E.KIND_ETH)
        if f["name"].startswith(("icmp", "arp")):
            assert sp is None, f["name"]
            seen += 1
        else:
            assert sp is not None and sp[0] + sp[1] <= len(r), f["name"]
    assert seen == 5
