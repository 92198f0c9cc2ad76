"""CPU-side checks of verify_unreach_reply (smol_csum_batch_verify_unreach_reply): the symbol, the entry struct in
its three spellings (C, ctypes, numpy), the argument errors, and tests/unreach_ref.py on a real port-unreachable
frame, on a hand-checked datagram and on the reference's own size limits.  No kernel is launched here."""
import ctypes
import json
import os
import re
import subprocess
import tempfile

import numpy as np

import oracle
import smoltcp_amd
from smoltcp_amd import _lib
from smoltcp_amd import engine as E
from tests import pktgen as P
from tests import unreach_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smol_csum_batch_verify_unreach_reply"
NOCAPS = (0, 0, 0, 0, 0)
V4A, V4B = bytes([10, 1, 2, 3]), bytes([10, 4, 5, 6])
V6A, V6B = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
NONE_OPEN = E.make_port_map([])


def test_symbol_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "smolcsum.h")) as f:
        full = f.read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    L = smoltcp_amd.lib()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(L, NAME) and NAME in _lib.ABI_SYMBOLS
    assert "smol_csum_unreach_t" in text
    for flag, val in (("REFUSED", 1), ("ANSWERED", 2), ("WRITTEN", 4), ("SEND", 8), ("HOST", 16), ("PORT", 32)):
        m = re.search(r"#define\s+SMOL_UNR_%s\s+0x([0-9a-fA-F]+)u" % flag, text)
        assert m and int(m.group(1), 16) == val == getattr(E, "UNR_" + flag) == getattr(R, flag)
    assert L.smol_csum_abi_version() == 6  # additive: the version stays
    # the header says who must not pass a port map
    flat = re.sub(r"\s*\n \*\s*", " ", full)
    assert "DNS socket matches the SOURCE port" in flat and "passes NULL or sets every bit" in flat


def test_make_port_map():
    m = E.make_port_map([0, 7, 8, 53, 65535])
    assert m.dtype == np.uint8 and m.shape == (8192,)
    assert m[0] == 0x81 and m[1] == 0x01 and m[53 >> 3] == 1 << (53 & 7) and m[8191] == 0x80 and int(m.astype(np.int64).sum()) == 0x81 + 1 + 32 + 0x80
    assert [R.port_open(m, p) for p in (0, 1, 7, 8, 9, 53, 65534, 65535)] == [True, False, True, True, False, True, False, True]
    assert not E.make_port_map([]).any()


_C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "smolcsum.h"
int main(void) {
    smol_csum_unreach_t e;
    memset(&e, 0, sizeof e);
    e.frame_len = 0x04030201u, e.data_off = 0x0605, e.head_len = 7, e.flags = 8;
    printf("{\"unr\": %zu, \"echo\": %zu, \"offsets\": [%zu, %zu, %zu, %zu], \"bytes\": [", sizeof e, sizeof(smol_csum_echo_t),
           offsetof(smol_csum_unreach_t, frame_len), offsetof(smol_csum_unreach_t, data_off),
           offsetof(smol_csum_unreach_t, head_len), offsetof(smol_csum_unreach_t, flags));
    for (size_t i = 0; i < sizeof e; ++i) printf("%s%u", i ? ", " : "", ((unsigned char*)&e)[i]);
    printf("]}\n");
    return 0;
}
"""


def test_struct_is_8_bytes_in_every_spelling():
    """C (compiled from the header: sizeof, offsetof and the bytes), ctypes and numpy agree on size and field
    order: the struct filled so that its bytes count 1, 2, 3, ... in memory order."""
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        with open(src, "w") as f:
            f.write(_C_PROBE)
        subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src],
                       check=True)
        c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert c["unr"] == 8 == c["echo"] and c["offsets"] == [0, 4, 6, 7] and c["bytes"] == list(range(1, 9))
    assert ctypes.sizeof(_lib.UnreachC) == 8 == E.UNR_DTYPE.itemsize == R.UNR_DTYPE.itemsize
    e = _lib.UnreachC(0x04030201, 0x0605, 7, 8)
    assert list(bytes(e)) == list(range(1, 9))
    assert [_lib.UnreachC.frame_len.offset, _lib.UnreachC.data_off.offset, _lib.UnreachC.head_len.offset,
            _lib.UnreachC.flags.offset] == [0, 4, 6, 7]
    a = np.frombuffer(bytes(e), dtype=E.UNR_DTYPE)[0]
    assert (int(a["frame_len"]), int(a["data_off"]), int(a["head_len"]), int(a["flags"])) == (0x04030201, 0x0605, 7, 8)
    assert E.UNR_DTYPE == R.UNR_DTYPE == E.ECHO_DTYPE
    assert [E.UNR_DTYPE.fields[k][1] for k in ("frame_len", "data_off", "head_len", "flags")] == [0, 4, 6, 7]


def test_verify_unreach_reply_argument_errors():
    L = smoltcp_amd.lib()
    b = _lib.BatchC()
    b.n, b.stride, b.len, b.kind = 1, 64, 64, 1
    caps = _lib.Caps()
    cfg = _lib.EchoCfgC()
    buf = (ctypes.c_uint8 * 64)()
    dst = (ctypes.c_uint8 * 64)()
    st = (ctypes.c_uint8 * 8)()
    pm = (ctypes.c_uint8 * 8192)()
    raw = (ctypes.c_uint8 * 64)()
    al = (ctypes.addressof(raw) + 15) & ~15  # 16-byte aligned: slots at al, entries at al + 16
    ctx = ctypes.c_void_p(1)  # never dereferenced: every case below fails its argument checks first
    call = getattr(L, NAME)
    B, C, G = ctypes.byref(b), ctypes.byref(caps), ctypes.byref(cfg)
    EINVAL = _lib.SMOL_EINVAL
    for g in (G, None):  # cfg and the port map are nullable: the same errors with and without them
        for m in (pm, None):
            assert call(None, buf, B, C, g, m, dst, al, st, al + 16, None) == EINVAL  # NULL ctx
            assert call(ctx, buf, B, None, g, m, dst, al, st, al + 16, None) == EINVAL  # NULL caps
            assert call(ctx, buf, B, C, g, m, None, al, st, al + 16, None) == EINVAL  # NULL d_dst
            assert call(ctx, buf, B, C, g, m, dst, None, st, al + 16, None) == EINVAL  # NULL d_slots
            assert call(ctx, buf, B, C, g, m, dst, al, None, al + 16, None) == EINVAL  # NULL d_status
            assert call(ctx, buf, B, C, g, m, dst, al, st, None, None) == EINVAL  # NULL d_unr
            assert call(ctx, buf, B, C, g, m, dst, al + 8, st, al + 16, None) == EINVAL  # d_slots not 16-byte aligned
            assert call(ctx, buf, B, C, g, m, dst, al, st, al + 20, None) == EINVAL  # d_unr not 8-byte aligned
            assert call(ctx, None, B, C, g, m, dst, al, st, al + 16, None) == EINVAL  # NULL d_buf
    bad = _lib.Caps()
    bad.icmpv4 = 4
    assert call(ctx, buf, B, ctypes.byref(bad), G, pm, dst, al, st, al + 16, None) == EINVAL  # bad caps value
    bad = _lib.Caps()
    bad.reserved[1] = 1
    assert call(ctx, buf, B, ctypes.byref(bad), G, pm, dst, al, st, al + 16, None) == EINVAL  # bad caps padding
    for i in range(4):  # a non-zero cfg->reserved, with everything else in order
        badcfg = _lib.EchoCfgC()
        badcfg.reserved[i] = 1
        assert call(ctx, buf, B, C, ctypes.byref(badcfg), pm, dst, al, st, al + 16, None) == EINVAL
    b.len = (1 << 30) + 1  # past SMOL_MAX_RECORD_LEN, as verify
    assert call(ctx, buf, B, C, G, pm, dst, al, st, al + 16, None) == _lib.SMOL_ERANGE
    b.len, b.n = 64, 0  # nothing to do: OK whatever the arrays are, nothing launched
    assert call(ctx, None, B, C, None, None, None, None, None, None, None) == _lib.SMOL_OK
    assert call(ctx, None, B, C, G, pm, None, None, None, None, None) == _lib.SMOL_OK


def test_reference_reply_to_the_port_unreachable_corpus_frame(golden):
    """fuzz/corpus/packet_parser/icmpv4_unreachable.bin is a real Port Unreachable of the largest size: 576 bytes
    of IP that quote 528 bytes of a 1032-byte UDP datagram.  The datagram it answers, rebuilt from the quoted
    header and data: unreach_ref's frame carries the corpus frame's whole ICMP message byte for byte, both
    checksums in it included; the outer header differs where its sender's stack differs from Ipv4Repr::emit (DSCP,
    ident, DF)."""
    fr = [f for f in golden["fuzz_corpus_frames"] if f["name"] == "icmpv4_unreachable.bin"][0]
    gold = bytes.fromhex(fr["bytes"])
    assert len(gold) == 14 + 576 and gold[34:36] == b"\x03\x03"
    q = gold[42:62]                                   # the quoted header
    plen = (q[2] << 8 | q[3]) - 20
    assert plen == 1032 and q[9] == 17 and gold[62 + 4:62 + 6] == P.be16(plen)
    dport = gold[62 + 2] << 8 | gold[62 + 3]
    req = gold[6:12] + gold[0:6] + b"\x08\x00" + P.ipv4(q[12:16], q[16:20], 17, gold[62:] + bytes(plen - 528), ttl=q[8],
                                                        ident=0xBEEF, flags_frag=0)
    slots = E.make_slots([0], [600])
    for ports, refused in ((NONE_OPEN, True), (E.make_port_map([dport]), False), (None, False)):
        st, ent, arena = R.expected([req], [E.KIND_ETH], [0], NOCAPS, None, ports, slots, 640)
        if not refused:
            assert not ent.view(np.uint8).any() and (arena == R.SENTINEL).all()
            continue
        assert int(ent[0]["flags"]) == R.REFUSED | R.ANSWERED | R.WRITTEN | R.PORT  # (the request's own checksums are 0)
        assert (int(ent[0]["frame_len"]), int(ent[0]["head_len"]), int(ent[0]["data_off"])) == (590, 62, 34)
        f = bytes(arena[:590])
        assert f[0:14] == gold[0:14] and f[34:] == gold[34:]
        assert f[14:34] == bytes.fromhex("45000240000040004001") + f[24:26] + gold[26:34] and (f[24], f[25]) != (0, 0)
        assert (arena[590:] == R.SENTINEL).all()


def test_reference_reply_to_a_hand_checked_datagram():
    """192.168.1.1:49152 -> 192.168.1.2:4000, "Hello, World!", TTL 63, ident 0x1234, DF clear.  The literal: total
    lengths 0x45 = 48 + 21 and 0x29 = 20 + 21, TTL 64 / protocol 1 outside and 63 / 17 in the quoted header,
    ident 0 and DF in both, the addresses swapped outside only; each of the three sums folds to 0xffff."""
    req = P.ipv4(bytes([192, 168, 1, 1]), bytes([192, 168, 1, 2]), 17, P.udp(49152, 4000, b"Hello, World!"), ttl=63,
                 ident=0x1234, flags_frag=0)
    want = bytes.fromhex("45000045000040004001b764c0a80102c0a80101" "0303ec1a00000000"
                         "45000029000040003f11b870c0a80101c0a80102" "c0000fa000150000" "48656c6c6f2c20576f726c6421")
    st, ent, arena = R.expected([req], [E.KIND_IP], [0], NOCAPS, None, NONE_OPEN, E.make_slots([3], [69]), 80)
    assert bytes(arena[3:72]) == want and (arena[:3] == R.SENTINEL).all() and (arena[72:] == R.SENTINEL).all()
    assert (int(ent[0]["frame_len"]), int(ent[0]["head_len"]), int(ent[0]["data_off"])) == (69, 48, 20)
    assert int(ent[0]["flags"]) == R.REFUSED | R.ANSWERED | R.WRITTEN | R.PORT

    def fold(b):
        s = sum(b[i] << 8 | b[i + 1] for i in range(0, len(b) - 1, 2)) + (b[-1] << 8 if len(b) % 2 else 0)
        while s >> 16:
            s = (s & 0xFFFF) + (s >> 16)
        return s

    assert fold(want[:20]) == fold(want[28:48]) == fold(want[20:]) == 0xFFFF
    # with the request's checksums filled the frame is the same and is to be sent; one byte short: reported only
    full = np.frombuffer(req, np.uint8).copy()
    oracle.batch_emit(full, None, 1, len(req), len(req), E.KIND_IP)
    st2, ent2, arena2 = R.expected([full.tobytes()], [E.KIND_IP], [0], NOCAPS, None, NONE_OPEN, E.make_slots([3], [69]), 80)
    assert st2[0] & E.ST_ACCEPT and int(ent2[0]["flags"]) == R.REFUSED | R.ANSWERED | R.WRITTEN | R.SEND | R.PORT
    got2 = bytes(arena2[3:72])  # the quoted UDP checksum is the request's, and the ICMP checksum covers it
    assert {i for i in range(69) if got2[i] != want[i]} <= {22, 23, 54, 55} and got2[54:56] == full.tobytes()[26:28] != b"\0\0"
    _, ent3, arena3 = R.expected([req], [E.KIND_IP], [0], NOCAPS, None, NONE_OPEN, E.make_slots([3], [68]), 80)
    assert int(ent3[0]["flags"]) == R.REFUSED | R.ANSWERED | R.PORT and int(ent3[0]["frame_len"]) == 69 and (arena3 == R.SENTINEL).all()
    # tx off: all three fields zero, everything else the same
    _, _, arena4 = R.expected([req], [E.KIND_IP], [0], (1, 0, 0, 1, 0), None, NONE_OPEN, E.make_slots([3], [69]), 80)
    z = bytearray(want)
    z[10:12] = z[22:24] = z[38:40] = b"\0\0"
    assert bytes(arena4[3:72]) == bytes(z)


def test_data_length_constants_are_the_references():
    """icmp_reply_payload_len(len, MIN_MTU, header len) = min(len, MIN_MTU - 2 * header len - 8): the largest
    frames are 576 / 1280 bytes of IP, the sizes test_icmp_reply_size pins (src/iface/interface/tests/ipv4.rs:1390,
    ipv6.rs:1141)."""
    assert R.DATA_V4 == 576 - 2 * 20 - 8 == 528 and R.DATA_V6 == 1280 - 2 * 40 - 8 == 1192
    with open(os.path.join(ROOT, "smoltcp_amd", "csrc", "csum_unreach.h")) as f:
        text = f.read()
    assert "UNR_DATA_V4 = 576u - 2u * 20u - 8u" in text and "UNR_DATA_V6 = 1280u - 2u * 40u - 8u" in text
    for ver, cut, ip_max in ((4, R.DATA_V4, 576), (6, R.DATA_V6, 1280)):
        for kind, e in ((E.KIND_IP, 0), (E.KIND_ETH, 14)):
            for plen in (cut - 1, cut, cut + 1, 1472):
                for port in (False, True):
                    pay = P.udp(9, 4000, bytes(plen - 8)) if port else bytes(plen)
                    r = P.ipv4(V4A, V4B, 17 if port else 47, pay) if ver == 4 else P.ipv6(V6A, V6B, 17 if port else 47, pay)
                    r = P.eth(r, 0x0800 if ver == 4 else 0x86DD) if e else r
                    need = R.frame_lens([r], [kind], [0], NONE_OPEN, None)[0]
                    assert need - e == min(plen, cut) + (48 if ver == 4 else 88) <= ip_max
                    assert (need - e == ip_max) == (plen >= cut)


def test_a_reference_reply_parses_back():
    """The oracle's verify accepts every reference frame under default caps, the quoted IPv4 header included."""
    rng = np.random.default_rng(7)
    recs, kinds = [], []
    for i in range(64):
        ver, port, plen = 4 if i % 2 else 6, bool(i % 3), int(rng.integers(8, 1473))
        pay = P.udp(9, 4000, P.rand_bytes(rng, plen - 8)) if port else P.rand_bytes(rng, plen)
        r = P.ipv4(V4A, V4B, 17 if port else 99, pay, ttl=1 + i) if ver == 4 else P.ipv6(V6A, V6B, 17 if port else 99, pay, hop=1 + i)
        kinds.append(E.KIND_ETH if i % 4 < 2 else E.KIND_IP)
        recs.append(P.eth(r, 0x0800 if ver == 4 else 0x86DD) if kinds[-1] == E.KIND_ETH else r)
    need = R.frame_lens(recs, kinds, 0, NONE_OPEN, None)
    offs = np.concatenate([[0], np.cumsum(need)[:-1]])
    st, ent, arena = R.expected(recs, kinds, 0, NOCAPS, None, NONE_OPEN, E.make_slots(offs, need), int(need.sum()) + 16)
    assert ((ent["flags"] & R.WRITTEN) != 0).all() and (need > 0).all()
    back = oracle.batch_verify(arena, E.make_descriptors(offs, need, np.asarray(kinds, np.uint8), 0), 64)
    assert (back & E.ST_ACCEPT).all() and (back & E.ST_IP_VALID).all() and (back & E.ST_L4_VALID).all()
    assert not (back & (E.ST_MALFORMED | E.ST_UNSUPPORTED)).any()
    for i in range(64):  # the quoted IPv4 header is a valid one of its own
        e = 14 if kinds[i] == E.KIND_ETH else 0
        f = arena[int(offs[i]):int(offs[i] + need[i])]
        if f[e] >> 4 == 4:
            total = int(f[e + 30]) << 8 | int(f[e + 31])  # (the quoted length is the request's: pad up to it)
            q = np.concatenate([f[e + 28:e + 48], np.zeros(total - 20 + 16, np.uint8)])
            qs = oracle.batch_verify(q, E.make_descriptors([0], [total], E.KIND_IP, E.REC_IPHDR_ONLY), 1)
            assert qs[0] & E.ST_IP_VALID and not qs[0] & E.ST_MALFORMED
    # and no reply is refused in turn
    _, ent2, _ = R.expected([bytes(arena[int(o):int(o + n)]) for o, n in zip(offs, need)], kinds, 0, NOCAPS, None, NONE_OPEN,
                            E.make_slots(offs, 0), 16)
    assert not ent2.view(np.uint8).any()


def test_reference_classes_that_are_not_refused_have_zero_entries():
    src, dst = V4A, V4B
    pay = bytes(range(24))
    u4 = P.ipv4(src, dst, 17, P.udp(7, 4000, pay))
    recs = [
        (P.ipv4(src, dst, 6, P.tcp(7, 9, pay)), E.KIND_IP, 0),
        (P.ipv6(V6A, V6B, 6, P.tcp(7, 9, pay)), E.KIND_IP, 0),
        (P.ipv4(src, dst, 1, P.icmp_echo(8, pay)), E.KIND_IP, 0),
        (P.ipv6(V6A, V6B, 58, P.icmp_echo(128, pay)), E.KIND_IP, 0),
        (P.ipv4(src, dst, 2, bytes([0x11, 0, 0, 0, 224, 0, 0, 1])), E.KIND_IP, 0),
        (P.ipv4(src, dst, 17, u4[20:], flags_frag=0x2000), E.KIND_IP, 0),   # fragments
        (P.ipv4(src, dst, 47, pay, flags_frag=0x0001), E.KIND_IP, 0),
        (u4, E.KIND_IP, E.REC_IPHDR_ONLY),
        (P.ipv4(src, dst, 47, pay), E.KIND_IP, E.REC_IPHDR_ONLY),
        (P.ipv4(src, dst, 47, pay), E.KIND_RAW, 0),
        (P.eth(u4, 0x0806), E.KIND_ETH, 0),
        (P.ipv4(src, dst, 47, pay)[:19], E.KIND_IP, 0),                     # truncated
        (P.ipv4(src, dst, 17, u4[20:27]), E.KIND_IP, 0),
        (P.ipv4(src, dst, 17, P.udp(7, 0, pay)), E.KIND_IP, 0),             # destination port 0
        (P.ipv4(src, dst, 17, P.udp(7, 53, pay)), E.KIND_IP, 0),            # an open port
        (P.ipv6(V6A, V6B, 0, P.hbh_opts(17, bytes([0xC2, 0])) + P.udp(7, 4000, pay)), E.KIND_IP, 0),  # a Hop-by-Hop drop
    ]
    slots = E.make_slots(np.arange(len(recs)) * 100, 100)
    st, ent, arena = R.expected([r for r, _, _ in recs], [k for _, k, _ in recs], [f for _, _, f in recs], NOCAPS, None,
                                E.make_port_map([53]), slots, 100 * len(recs))
    assert not ent.view(np.uint8).any() and (arena == R.SENTINEL).all()
    # without a port map no UDP datagram is refused, and the protocol form still is
    both = [u4, P.ipv4(src, dst, 47, pay)]
    _, ent, _ = R.expected(both, E.KIND_IP, 0, NOCAPS, None, None, E.make_slots([0, 100], 100), 200)
    assert ent["flags"].tolist() == [0, R.REFUSED | R.ANSWERED | R.WRITTEN]  # (the request's header checksum is 0: no SEND)
    # behind a Hop-by-Hop header the reply is the host's
    hb = [P.ipv6(V6A, V6B, 0, P.hbh(17, 0, None) + P.udp(7, 4000, pay)), P.ipv6(V6A, V6B, 0, P.hbh(47, 0, None) + pay)]
    _, ent, arena = R.expected(hb, E.KIND_IP, 0, NOCAPS, None, NONE_OPEN, E.make_slots([0, 100], 100), 200)
    assert ent["flags"].tolist() == [R.REFUSED | R.HOST | R.PORT, R.REFUSED | R.HOST] and (arena == R.SENTINEL).all()
    assert ent["data_off"].tolist() == [40, 40] and not ent["frame_len"].any() and not ent["head_len"].any()
